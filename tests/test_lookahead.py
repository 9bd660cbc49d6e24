"""Lookahead in the device rollout (K0h, mpmpc_rollout_set_lookahead): every column of a car's horizon is built against its
movers' discs of the step at which the car is expected to get there (csrc/lookahead_core.hpp).

CPU: the host twin (tests/emul_lookahead, the same lookahead_core.hpp) against the numpy restatement of the law in
lookahead.py - leads and horizon discs, bit for bit, on both tracks; the argument checks; and "it matters": on the step-0
waypoints of the GPU fleets the anticipated rows differ from the plain ones for at least a quarter of the cars, none blocked.
GPU: the fleets of tests/test_movers.py (3 static discs, 2 movers along the path, 1 crossing mover per car).  Zero times and
frozen movers change nothing; infinite times are a plain rollout with step0 shifted; after every step the leads, the disc
table, the rows and the verdicts are the restated law's and the twin's - with walls, with routes, under perception; one call
equals the step-by-step loop; the refusals."""
import ctypes as C

import numpy as np
import pytest

import lookahead as LK
import mpmpc
import mpmpc_testlib as T
import scenarios
import test_movers as TM
import test_routes as TR
import twins

bp = C.POINTER(C.c_int8)
E_ARG, E_STATE = -1, -3
TS = TM.TS
SHAPES = dict(sim=(30, 64, 12, 71), real=(70, 32, 8, 72))      # N, B, steps, seed (the seeds: chosen on the CPU, see test 3)
MAX_LEAD = 40


_d, _i = T._d, T._i


@pytest.fixture(scope="module")
def twin():
    """The CPU twin of K0h and K0c<WALLS, LEAD> (tests/emul_lookahead)."""
    return twins.lookahead()


@pytest.fixture(scope="module")
def car_twin():
    """The CPU twin of K0c (tests/emul_car): test_movers' Fleet draws cars again whose plain step-0 row it finds blocked."""
    return twins.car()


# ------------------------------------------------------------------------------------------------ worlds and the two sides
class Ctx:
    """A map and a path table (one path, or routes laid end to end) and, on it, the twin's and the restated law's sides of a
    step.  route: None, or per car (first global row, length, circular)."""

    def __init__(self, grid, origin, res, sm, tab, cum, circular, v_ref, first=None, circ=None):
        self.grid, self.origin, self.res, self.sm = grid, (float(origin[0]), float(origin[1])), float(res), float(sm)
        self.a = {k: np.ascontiguousarray(tab[k], float) for k in ("x", "y", "psi", "ds_next", "border_ub", "border_lb")}
        self.cum = np.ascontiguousarray(cum, float)
        self.n_wp, self.circular = self.a["x"].size, bool(circular)
        self.seg_default = LK.Lookahead.seg_time_of(self.a["ds_next"], v_ref)
        self.first, self.circ = first, circ

    @classmethod
    def track(cls, track):
        g1, grid, origin, res = T.g1_world(track)
        tr = scenarios.sim_track() if track == "sim" else scenarios.real_track()
        return cls(grid, origin, res, T.safety_margin(track), g1, np.cumsum(g1["segment_lengths"]), track == "sim", tr.v_ref)

    def headers(self, route):
        """the device's car headers {first row, length - negated when open} of cars on routes `route`, or None"""
        if route is None:
            return None
        n = np.diff(self.first)
        return np.ascontiguousarray(np.stack([self.first[route], np.where(self.circ[route] != 0, n[route], -n[route])], 1), np.int32)

    def views(self, route, B):
        """per car: first row, length, circular"""
        if route is None:
            return np.zeros(B, np.int64), np.full(B, self.n_wp), np.full(B, self.circular)
        return self.first[route].astype(np.int64), np.diff(self.first)[route], self.circ[route] != 0

    # --- leads
    def leads_twin(self, twin, wp, N, seg, max_lead, route=None):
        wp = np.ascontiguousarray(wp, np.int32)
        out = np.full((wp.size, N), -7, np.int32)
        twin.look_emu_leads(wp.size, N, _i(wp), _i(self.headers(route)), self.n_wp, int(self.circular), _d(np.ascontiguousarray(seg, float)),
                            TS, int(max_lead), _i(out))
        return out

    def leads_law(self, wp, N, seg, max_lead, route=None):
        f, n, c = self.views(route, np.asarray(wp).size)
        return LK.leads(wp, N, seg, TS, max_lead, n_wp=n, circular=c, first=f)

    # --- horizon discs of a fleet (rows: one [k_b, 6] array per car) -> [movers, N, 3]
    def discs_twin(self, twin, rows, k, step0, lead, route=None):
        B, N = lead.shape
        moff = np.zeros(B + 1, np.int32)
        moff[1:] = np.cumsum([len(r) for r in rows])
        flat = np.concatenate(rows).reshape(-1, 6)
        kind, rad = (np.ascontiguousarray(flat[:, c], np.int32) for c in (0, 1))
        prm = np.ascontiguousarray(flat[:, 2:], float)
        out = np.full((flat.shape[0], N, 3), -7, np.int32)
        twin.look_emu_discs(B, N, _i(moff), _i(kind), _i(rad), _d(prm), int(k), int(step0), _i(np.ascontiguousarray(lead, np.int32)),
                            _i(self.headers(route)), self.grid.shape[0], self.grid.shape[1], self.origin[0], self.origin[1], self.res,
                            self.n_wp, _d(self.cum), _d(self.a["x"]), _d(self.a["y"]), _d(self.a["psi"]), int(self.circular), _i(out))
        return out

    def discs_law(self, rows, k, step0, lead, route=None):
        B, N = lead.shape
        f, n, c = self.views(route, B)
        out = []
        for b in range(B):           # (cars of one view could share a call; the fleets here are small)
            sl = slice(int(f[b]), int(f[b] + n[b]))
            out.append(LK.discs(rows[b], k, lead[b], step0, self.origin, self.res, self.grid.shape[1], self.grid.shape[0],
                                cum=self.cum[sl], x=self.a["x"][sl], y=self.a["y"][sl], psi=self.a["psi"][sl], circular=bool(c[b])))
        return np.concatenate(out)

    # --- K0c's rows: disc_lists the lists K0c plans from at the step; look = (rows, hz) or None; walls: per-car [k, 4] or None
    def rows_twin(self, twin, wp, N, disc_lists, look=None, walls=None, route=None):
        B = len(disc_lists)
        off, flat = T.csr(disc_lists, 3, pad=False)
        woff, wflat = T.csr(walls, 4, pad=False)
        car = hz = None
        if look is not None:
            rows, hz = look
            car = np.zeros((B + 1, 2), np.int32)
            car[1:, 0] = np.cumsum([len(r) for r in rows])
            car[:B, 1] = [len(disc_lists[b]) - len(rows[b]) for b in range(B)]      # (no traffic slots in these fleets)
            hz = np.ascontiguousarray(hz, np.int32)
        ub, lb, flag = np.zeros((B, N)), np.zeros((B, N)), np.zeros(B, np.int32)
        a = self.a
        rc = twin.look_emu_rows(self.grid.shape[0], self.grid.shape[1], self.grid.ctypes.data_as(bp), self.origin[0], self.origin[1], self.res,
                                self.n_wp, _d(a["x"]), _d(a["y"]), _d(a["psi"]), _d(a["ds_next"]), int(self.circular), _d(a["border_ub"]),
                                _d(a["border_lb"]), N, 2 * self.sm, self.sm, B, _i(np.ascontiguousarray(wp, np.int32)), _i(off), _i(flat),
                                _i(woff), _i(wflat), _i(self.headers(route)), _i(car), _i(hz), _d(ub), _d(lb), _i(flag))
        assert rc == 0
        return ub, lb, flag


_CTX = {}


def ctx(track):
    if track not in _CTX:
        _CTX[track] = Ctx.track(track)
    return _CTX[track]


_FLEETS = {}


def fleet(track, car_twin):
    """test_movers' Fleet at this file's shapes: 3 static discs, 2 along-path movers, 1 crossing line mover per car"""
    if track not in _FLEETS:
        N, B, steps, seed = SHAPES[track]
        _FLEETS[track] = TM.Fleet(track, N, B, steps, seed, car_twin)
    return _FLEETS[track]


def true_lists(fl, k):
    """per car: static discs, then the movers' discs of step k"""
    return fl.discs_at(k)


# ------------------------------------------------------------------------------------------------------------ CPU
def _seg_variants(c, rng):
    z = c.seg_default.copy()
    z[rng.random(z.size) < 0.3] = 0.0
    inf = c.seg_default.copy()
    inf[rng.random(inf.size) < 0.05] = np.inf
    return [("default", c.seg_default, MAX_LEAD), ("zeros", z, MAX_LEAD), ("inf", inf, 9), ("lead1", c.seg_default, 1),
            ("all_zero", np.zeros(c.n_wp), 5), ("all_inf", np.full(c.n_wp, np.inf), 7), ("slow", 7.3 * c.seg_default, 1 << 20)]


@pytest.mark.parametrize("track", ["sim", "real"])
def test_twin_equals_the_restated_law_bit_exact(track, twin, car_twin):
    c = ctx(track)
    N = SHAPES[track][0]
    fl = fleet(track, car_twin)
    rng = np.random.default_rng(11)
    wp = fl.starts.copy()
    # a circular route started 3 waypoints before the wrap / an open route started closer than N to its end
    wp[:4] = [c.n_wp - 3, c.n_wp - 1, 0, c.n_wp - 2] if c.circular else [c.n_wp - N + 5, c.n_wp - 2, 0, c.n_wp - N // 2]
    seen = set()
    for tag, seg, max_lead in _seg_variants(c, rng):
        lead = c.leads_twin(twin, wp, N, seg, max_lead)
        assert np.array_equal(lead, c.leads_law(wp, N, seg, max_lead)), tag
        assert lead.min() >= 0 and lead.max() <= max_lead and np.all(np.diff(lead, axis=1) >= 0)
        seen.update(np.unique(lead).tolist())
        if tag == "all_zero":
            assert not lead.any()
        if tag in ("all_inf",):
            assert np.all(lead == max_lead)
        if tag == "lead1":
            assert set(np.unique(lead).tolist()) <= {0, 1} and lead.max() == 1
        for k, step0 in ((0, 0), (5, -3)):
            got = c.discs_twin(twin, fl.rows, k, step0, lead)
            assert np.array_equal(got, c.discs_law(fl.rows, k, step0, lead)), (tag, k)
            if tag == "all_zero":        # lead 0: the discs of the step itself, at every column
                now = np.concatenate([TM._np_discs(r, k - step0, fl.w) for r in fl.rows])
                assert np.array_equal(got, np.repeat(now[:, None], N, 1))
    assert len(seen) > 20


def test_routes_views_of_the_law(twin):
    """route fleets: seg_time by global row, wrap / clamp inside the car's route"""
    c, first, circ = _route_ctx()
    N = 30
    n = np.diff(first)
    route = np.array([0, 0, 1, 1, 1, 0], np.int32)
    wp = np.array([n[0] - 3, 17, n[1] - 5, 0, n[1] - N + 2, n[0] - 1], np.int32)
    lead = c.leads_twin(twin, wp, N, c.seg_default, MAX_LEAD, route)
    assert np.array_equal(lead, c.leads_law(wp, N, c.seg_default, MAX_LEAD, route))
    # the open route's last columns all read its last waypoint's row; the circular one wraps to its own first row
    rows = LK.column_rows(wp, N, n[route], circ[route] != 0, 0)
    assert np.all(rows[2, 5:] == n[1] - 1) and rows[0, 3] == 0 and rows[0, 2] == n[0] - 1
    movers = [np.array([(1, 6, c.cum[first[r] + (w + 8) % n[r] if circ[r] else first[r] + min(w + 8, n[r] - 2)], 0.02, 0.02, 0.0)]) for r, w in zip(route, wp)]
    got = c.discs_twin(twin, movers, 3, 0, lead, route)
    assert np.array_equal(got, c.discs_law(movers, 3, 0, lead, route)) and np.any(got[:, :, 2] > 0)


def test_setting_validation_without_device(twin, built_library):
    lib = mpmpc.load_library(built_library)
    assert lib.mpmpc_rollout_set_lookahead(None, 1, None, 1) == E_ARG
    assert lib.mpmpc_rollout_lookahead(None, 1, None, None) == E_ARG
    assert "mpmpc_rollout_set_lookahead" in mpmpc.EXPORTS and "mpmpc_rollout_lookahead" in mpmpc.EXPORTS
    raw = C.CDLL(built_library)
    assert hasattr(raw, "mpmpc_rollout_set_lookahead") and hasattr(raw, "mpmpc_rollout_lookahead")

    def check(seg, max_lead=3, n_wp=None, path_n=None):
        seg = np.ascontiguousarray(seg, float)
        return twin.look_emu_check(seg.size if n_wp is None else n_wp, seg.size if path_n is None else path_n, _d(seg), max_lead)
    ok = np.array([0.0, 0.1, np.inf, 1e300])
    assert check(ok) == 0 and check(ok, 1) == 0 and check(ok, 1 << 20) == 0
    assert check(ok, 0) == E_ARG and check(ok, -1) == E_ARG and check(ok, (1 << 20) + 1) == E_ARG
    assert check(ok, n_wp=3) == E_ARG and check(ok, path_n=5) == E_ARG and check(ok, path_n=0) == E_ARG
    for bad in (np.nan, -1e-300, -np.inf, -0.5):
        seg = ok.copy()
        seg[1] = bad
        assert check(seg) == E_ARG, bad
    assert check([-0.0, 0.0]) == 0
    assert twin.look_emu_table_bytes(3 * 64, 30) == 3 * 64 * 30 * 12
    # the Python front end
    assert np.array_equal(LK.Lookahead.seg_time_of([1.0, 2.0, 0.5, 1.0], [2.0, 0.0, -1.0, 4.0]), [0.5, np.inf, np.inf, 0.25])
    la = LK.Lookahead(5)
    assert la.max_lead == 5 and la.seg_time is None and np.array_equal(la.table([1.0], [2.0]), [0.5])
    assert np.array_equal(LK.Lookahead(2, [0.25, 0.5]).table([1.0, 1.0], [2.0, 2.0]), [0.25, 0.5])
    for bad in (0, -3, (1 << 20) + 1):
        with pytest.raises(ValueError):
            LK.Lookahead(bad)


def _step0_rows(track, twin, car_twin):
    c, fl = ctx(track), fleet(track, car_twin)
    N = SHAPES[track][0]
    lists = true_lists(fl, 0)
    lead = c.leads_law(fl.starts, N, c.seg_default, MAX_LEAD)
    hz = c.discs_law(fl.rows, 0, 0, lead)
    plain = c.rows_twin(twin, fl.starts, N, lists)
    ahead = c.rows_twin(twin, fl.starts, N, lists, look=(fl.rows, hz))
    return plain, ahead


@pytest.mark.parametrize("track", ["sim", "real"])
def test_it_matters_at_step_0(track, twin, car_twin):
    """The seeds of SHAPES were chosen here, on the CPU: the anticipated step-0 rows differ from the plain ones for at least a
    quarter of the cars, and no car's anticipated row is blocked or overflows (the plain ones: test_movers' Fleet sees to it)."""
    plain, ahead = _step0_rows(track, twin, car_twin)
    B = SHAPES[track][1]
    assert not plain[2].any() and not ahead[2].any()
    differ = np.any((plain[0] != ahead[0]) | (plain[1] != ahead[1]), 1)
    # (the two sides of that comparison differ by the lookahead alone: with every lead 0 the anticipated rows are the plain ones)
    c, fl, N = ctx(track), fleet(track, car_twin), SHAPES[track][0]
    hz0 = c.discs_law(fl.rows, 0, 0, np.zeros((B, N), np.int32))
    same = c.rows_twin(twin, fl.starts, N, true_lists(fl, 0), look=(fl.rows, hz0))
    assert np.array_equal(same[0], plain[0]) and np.array_equal(same[1], plain[1]) and not same[2].any()
    shifted = int(np.sum(np.any(hz0 != c.discs_law(fl.rows, 0, 0, c.leads_law(fl.starts, N, c.seg_default, MAX_LEAD)), (1, 2))))
    print("movers whose disc moves within the horizon: %d of %d" % (shifted, hz0.shape[0]))
    print("%s: %d of %d cars' step-0 rows differ" % (track, differ.sum(), B))
    assert differ.sum() * 4 >= B
    # the plain twin is K0c's own twin
    flag = TM._twin_flags(car_twin, track, true_lists(fleet(track, car_twin), 0), fleet(track, car_twin).starts, SHAPES[track][0])
    assert not flag.any()


# ------------------------------------------------------------------------------------------------------------ GPU
def _set_world(h, fl, rows=None, walls=None, step0=0):
    if walls is not None:
        h.rollout_set_walls(walls)
    h.rollout_set_obstacles(fl.static)
    h.rollout_set_movers(fl.rows if rows is None else rows, step0=step0)


def _run(h, fl, steps):
    fl.init(h)
    h.rollout_step(steps)
    return h.rollout_state(), h.rollout_corridor()


def _same_run(a, b):
    TM._same(a[0], b[0])
    for k in ("x0", "u"):
        assert np.array_equal(a[0][k], b[0][k]), k
    assert np.array_equal(a[1][0], b[1][0], equal_nan=True) and np.array_equal(a[1][1], b[1][1], equal_nan=True)      # rows, and NaN rows: the verdicts


@pytest.fixture(scope="module")
def plain_runs(car_twin):
    """per track, computed once: the rollout without lookahead, with the fleet's movers and with them frozen"""
    cache = {}

    def get(track):
        if track not in cache:
            N, B, steps, _ = SHAPES[track]
            fl = fleet(track, car_twin)
            h, _ = TM._handle(track, N, B)
            _set_world(h, fl)
            moving = _run(h, fl, steps)
            _set_world(h, fl, rows=fl.frozen_rows())
            frozen = _run(h, fl, steps)
            h.close()
            cache[track] = dict(moving=moving, frozen=frozen)
        return cache[track]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("track", ["sim", "real"])
def test_zero_times_change_nothing(track, plain_runs, car_twin):
    N, B, steps, _ = SHAPES[track]
    c, fl = ctx(track), fleet(track, car_twin)
    h, _ = TM._handle(track, N, B)
    _set_world(h, fl)
    for max_lead in (1, 13):
        h.rollout_set_lookahead(np.zeros(c.n_wp), max_lead)
        got = _run(h, fl, steps)
        _same_run(got, plain_runs(track)["moving"])
        lead, discs = h.rollout_lookahead()
        assert not lead.any() and discs.shape == (3 * B, N, 3)
    TM._enough_alive(got[0])
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("track", ["sim", "real"])
def test_frozen_movers_change_nothing(track, plain_runs, car_twin):
    N, B, steps, _ = SHAPES[track]
    c, fl = ctx(track), fleet(track, car_twin)
    h, _ = TM._handle(track, N, B)
    _set_world(h, fl, rows=fl.frozen_rows())
    h.rollout_set_lookahead(c.seg_default, MAX_LEAD)
    got = _run(h, fl, steps)
    _same_run(got, plain_runs(track)["frozen"])
    assert h.rollout_lookahead()[0].max() > 5          # the columns did look ahead
    # ... and the moving fleet's run does differ from the plain one
    _set_world(h, fl)
    moved = _run(h, fl, steps)
    assert not np.array_equal(moved[0]["s"], plain_runs(track)["moving"][0]["s"])
    h.rollout_set_lookahead(None)                      # off again: the plain run
    _same_run(_run(h, fl, steps), plain_runs(track)["moving"])
    with pytest.raises(mpmpc.MpmpcError):
        h.rollout_lookahead()                          # that step did not look ahead
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 7])
def test_saturated_leads_are_a_shifted_plain_rollout(L, car_twin):
    """seg_time all inf: every column's lead is max_lead = L, so a step's rows are those of a plain rollout whose movers run
    L steps ahead - device against device.  Handle 2 is teacher-forced: re-initialised from handle 1's state in front of every
    step, its movers set with step0 = -(k + L), so that only K0c's inputs differ.  (A mover that is off the grid at step k
    stays absent at every column on handle 1 - the gate - and may be back at k + L on handle 2: cars with such a mover are
    left out, and counted.)"""
    track = "sim"
    N, B, steps, _ = SHAPES[track]
    c, fl = ctx(track), fleet(track, car_twin)
    h1, _ = TM._handle(track, N, B)
    h2, _ = TM._handle(track, N, B)
    _set_world(h1, fl)
    h1.rollout_set_lookahead(np.full(c.n_wp, np.inf), L)
    fl.init(h1)
    h2.rollout_set_obstacles(fl.static)
    compared = 0
    for k in range(steps):
        st = h1.rollout_state()
        h2.rollout_init(TS, fl.cum, st["s"], st["pose"], cc0=st["cc"])
        h2.rollout_set_counters(np.minimum(st["counter"], N - 2))
        h2.rollout_set_movers(fl.rows, step0=-(k + L))
        h1.rollout_step(1)
        h2.rollout_step(1)
        a, b = h1.rollout_corridor(), h2.rollout_corridor()
        after = h1.rollout_state()
        assert np.all(h1.rollout_lookahead()[0] == L)
        present = np.array([np.all(TM._np_discs(fl.rows[i], k, fl.w)[:, 2] > 0) for i in range(B)])
        sel = (st["alive"] == 1) & np.isin(after["alive"], (1, -1, -3, -4)) & present
        assert np.array_equal(after["wp_id"][sel], h2.rollout_state()["wp_id"][sel])
        assert np.array_equal(a[0][sel], b[0][sel], equal_nan=True) and np.array_equal(a[1][sel], b[1][sel], equal_nan=True), k
        compared += int(sel.sum())
    h1.close()
    h2.close()
    assert compared * 10 >= 8 * B * steps, compared


def _check_steps(h, c, twin, rows, N, B, steps, seg, max_lead, walls=None, route=None, gate=None, step0=0):
    """after every step of a step-by-step run: rollout_lookahead() against the restated law on the step's wp_id, and
    rollout_corridor() and the verdicts against the twin's rows on those inputs (cars the step planned for).  gate(k, true
    lists) -> the lists K0c planned from (perception), else the true ones.  -> cars compared, cars whose rows differ from
    the plain twin's"""
    compared = mattered = 0
    for k in range(steps):
        before = h.rollout_state()
        h.rollout_step(1)
        st = h.rollout_state()
        lead, hz = h.rollout_lookahead()
        assert lead.dtype == np.int32 and np.array_equal(lead, c.leads_law(st["wp_id"], N, seg, max_lead, route)), k
        assert np.array_equal(hz, c.discs_law(rows, k, step0, lead, route)), k
        true = h.rollout_obstacles()
        lists = true if gate is None else gate(k, true)
        ub, lb, flag = c.rows_twin(twin, st["wp_id"], N, lists, look=(rows, hz), walls=walls, route=route)
        got_ub, got_lb = h.rollout_corridor()
        planned = (before["alive"] == 1) & np.isin(st["alive"], (1, -1, -3, -4))
        assert np.array_equal(got_ub[planned], ub[planned], equal_nan=True) and np.array_equal(got_lb[planned], lb[planned], equal_nan=True), k
        assert np.array_equal(st["alive"][planned & (flag == 1)], np.full((planned & (flag == 1)).sum(), -3))
        assert np.array_equal(st["alive"][planned & (flag == 2)], np.full((planned & (flag == 2)).sum(), -4))
        assert not np.any(np.isin(st["alive"][planned & (flag == 0)], (-3, -4)))
        plain = c.rows_twin(twin, st["wp_id"], N, lists, walls=walls, route=route)
        mattered += int((planned & np.any((plain[0] != ub) | (plain[1] != lb), 1) & (flag == 0) & (plain[2] == 0)).sum())
        compared += int(planned.sum())
    return compared, mattered


def _walls_of(c, fl, rng):
    """one wall per car across part of the road, 7 .. 10 waypoints ahead (test_perception's recipe)"""
    walls = []
    for b in range(fl.B):
        w = (int(fl.starts[b]) + 7 + int(rng.integers(0, 4))) % c.n_wp
        (ux, uy), (lx, ly) = c.a["border_ub"][w], c.a["border_lb"][w]
        pts = [(ux + t * (lx - ux), uy + t * (ly - uy)) for t in (0.05, 0.35)]
        walls.append(np.array([[int(np.floor((p - o) / c.res)) for pt in pts for p, o in zip(pt, c.origin)]], np.int32))
    return walls


@pytest.mark.gpu
@pytest.mark.parametrize("track,with_walls", [("sim", False), ("real", False), ("sim", True)])
def test_every_step_equals_the_law_and_the_twin(track, with_walls, twin, car_twin):
    N, B, steps, _ = SHAPES[track]
    c, fl = ctx(track), fleet(track, car_twin)
    walls = _walls_of(c, fl, np.random.default_rng(5)) if with_walls else None
    h, _ = TM._handle(track, N, B)
    _set_world(h, fl, walls=walls)
    h.rollout_set_lookahead(c.seg_default, MAX_LEAD)
    fl.init(h)
    compared, mattered = _check_steps(h, c, twin, fl.rows, N, B, steps, c.seg_default, MAX_LEAD, walls=walls)
    st = h.rollout_state()
    h.close()
    print("%s walls=%s: %d car-steps compared, %d with rows the lookahead changed; alive %s" %
          (track, with_walls, compared, mattered, dict(zip(*np.unique(st["alive"], return_counts=True)))))
    assert compared * 2 >= B * steps and mattered * 8 >= compared


@pytest.mark.gpu
@pytest.mark.parametrize("track", ["sim", "real"])
def test_one_call_equals_single_steps(track, car_twin):
    N, B, steps, _ = SHAPES[track]
    c, fl = ctx(track), fleet(track, car_twin)
    h, _ = TM._handle(track, N, B)
    _set_world(h, fl)
    h.rollout_set_lookahead(c.seg_default, MAX_LEAD)
    one = _run(h, fl, steps)
    look_one = h.rollout_lookahead()
    fl.init(h)
    for _ in range(steps):
        h.rollout_step(1)
    single = (h.rollout_state(), h.rollout_corridor())
    look_single = h.rollout_lookahead()
    h.close()
    _same_run(one, single)
    assert np.array_equal(look_one[0], look_single[0]) and np.array_equal(look_one[1], look_single[1])
    TM._enough_alive(one[0])


def _route_ctx():
    own, cat, first, circ, grid, sm = TR._route_tables(scenarios.sim_track(), ["L", "Bo"])
    c = Ctx(grid, (-1.0, -2.0), 0.005, sm, cat, cat["cum_lengths"], False, cat["v_ref"], first=np.asarray(first, np.int64), circ=np.asarray(circ))
    c.cat = cat
    return c, np.asarray(first, np.int64), np.asarray(circ)


@pytest.mark.gpu
def test_routes_every_step_equals_the_law_and_the_twin(twin):
    """two routes in one fleet, the lap (circular) and the open second half of it, along-path movers on both"""
    N, B, steps = 30, 32, 10
    c, first, circ = _route_ctx()
    n = np.diff(first)
    rng = np.random.default_rng(31)
    route = (np.arange(B) % 2).astype(np.int32)
    wp = np.array([rng.integers(0, n[p] - N - 8 if not circ[p] else n[p]) for p in route], np.int32)
    wp[0], wp[1] = n[0] - 3, n[1] - N - 4              # the wrap within the horizon; the open end within the run
    g = first[route] + wp
    s, poses = c.cum[g], np.stack([c.a["x"][g], c.a["y"][g], c.a["psi"][g]], 1)
    tr = scenarios.sim_track()
    rows = []
    for b in range(B):
        ahead = lambda a: (wp[b] + a) % n[route[b]] if circ[route[b]] else min(wp[b] + a, n[route[b]] - 2)
        rows.append(np.array([(1, int(rng.integers(6, 11)), c.cum[first[route[b]] + ahead(int(rng.integers(6, 20)))], rng.uniform(-0.08, 0.08),
                               rng.uniform(1 / 3, 2 / 3) * tr.v_ref[0] * TS, 0.0) for _ in range(2)], float))
    h = mpmpc.Handle(T.stock_config(N, max_batch=B, circular=False), mpmpc.default_settings())
    h.set_path(c.cat["kappa"], c.cat["v_ref"], c.cat["ds_next"])
    h.set_routes(first, circ)
    h.set_map(c.grid, c.origin, c.res)
    h.set_path_geometry(c.a["x"], c.a["y"], c.a["psi"], c.a["border_ub"], c.a["border_lb"])
    assert h.build_corridor(N, 2 * c.sm, c.sm, want_tables=False)[2] == 0
    h.set_car_routes(route)
    h.rollout_warm_start(False)
    h.rollout_set_movers(rows)
    h.rollout_set_lookahead(c.seg_default, MAX_LEAD)
    h.rollout_init(TS, c.cum, s, poses)
    compared, mattered = _check_steps(h, c, twin, rows, N, B, steps, c.seg_default, MAX_LEAD, route=route)
    st = h.rollout_state()
    # the routes change: the setting is void, like the per-car ones
    h.set_routes(first, circ[::-1].copy())
    with pytest.raises(mpmpc.MpmpcError):
        h.rollout_step(1)
    h.close()
    print("routes: %d car-steps compared, %d changed by the lookahead; alive %s" % (compared, mattered, dict(zip(*np.unique(st["alive"], return_counts=True)))))
    assert compared * 2 >= B * steps and mattered >= 1 and (st["alive"] == -2).any()


@pytest.mark.gpu
def test_perception_gates_the_movers(twin, car_twin):
    """hold = 2: a car anticipates exactly the movers it knows at the step - the known mask recomputed from
    rollout_perception()'s books by the restated per_known (a static disc once seen, a mover for `hold` steps after it was
    last seen), the twin's rows with the lists gated by it"""
    track, B, hold = "sim", 32, 2
    N, _, steps, _ = SHAPES[track]
    c = ctx(track)
    fl = TM.Fleet(track, N, B, steps, 73, car_twin)
    h, _ = TM._handle(track, N, B)
    _set_world(h, fl)
    h.rollout_set_perception(np.linspace(-np.pi / 2, np.pi / 2, 181), 0.3, hold)
    h.rollout_set_lookahead(c.seg_default, MAX_LEAD)
    fl.init(h)
    seen = dict(unknown=0, known=0)

    def gate(k, true):
        per = h.rollout_perception()
        out = []
        for b in range(B):
            last = per["disc_last"][b, :6]
            known = np.array([last[q] >= 0 if q < 3 else (last[q] >= 0 and k - last[q] <= hold) for q in range(6)])
            assert sum(int(v) << q for q, v in enumerate(known)) == int(per["disc_known"][b]), (k, b)
            seen["unknown"] += int((~known[3:]).sum())
            seen["known"] += int(known[3:].sum())
            out.append(np.where(known[:, None], true[b], 0).astype(np.int32))
        return out
    compared, mattered = _check_steps(h, c, twin, fl.rows, N, B, steps, c.seg_default, MAX_LEAD, gate=gate)
    h.close()
    print("perception: %d car-steps compared, %d changed by the lookahead, movers known / unknown %s" % (compared, mattered, seen))
    assert compared * 2 >= B * steps and seen["unknown"] > 0 and seen["known"] > 0 and mattered >= 1


@pytest.mark.gpu
def test_refusals(car_twin):
    track = "sim"
    N, B, steps, _ = SHAPES[track]
    c, fl = ctx(track), fleet(track, car_twin)
    h, _ = TM._handle(track, N, B)
    with pytest.raises(mpmpc.MpmpcError):
        h.rollout_lookahead()                                        # the getter before any step
    ok = c.seg_default
    for seg, max_lead, what in ((ok[:-1], 3, "n_wp"), (np.r_[ok[:-1], np.nan], 3, "NaN"), (np.r_[-1.0, ok[1:]], 3, "negative"),
                                (ok, 0, "max_lead"), (ok, (1 << 20) + 1, "max_lead")):
        with pytest.raises(mpmpc.MpmpcError, match=what):
            h.rollout_set_lookahead(seg, max_lead)
    h.rollout_set_lookahead(np.r_[ok[:-1], np.inf], 3)               # +inf is allowed
    _set_world(h, fl)
    fl.init(h)
    with pytest.raises(mpmpc.MpmpcError):
        h.rollout_lookahead()                                        # no step yet
    h.rollout_step(1)
    lead, discs = h.rollout_lookahead()
    assert lead.shape == (B, N) and discs.shape == (3 * B, N, 3)
    h.rollout_set_movers(fl.rows)                                    # a per-car setting anew: the last step's table is no longer its
    with pytest.raises(mpmpc.MpmpcError):
        h.rollout_lookahead()
    h.rollout_step(1)
    h.rollout_lookahead()
    tr = scenarios.sim_track()
    h.set_path(tr.kappa, tr.v_ref, tr.ds_next)                       # the path set anew: every setting is void
    assert h.lib.mpmpc_rollout_step(h._h, B, 1) == E_STATE
    h.rollout_set_movers(None)
    h.rollout_set_obstacles(None)                                    # ... the lookahead on its own too
    with pytest.raises(mpmpc.MpmpcError, match="set_lookahead"):
        h.rollout_step(1)
    h.rollout_set_lookahead(ok, 3)
    h.rollout_step(1)                                                # the shared table: nothing looks ahead
    with pytest.raises(mpmpc.MpmpcError):
        h.rollout_lookahead()
    h.close()


@pytest.mark.gpu
def test_batch_mpc_rollout_takes_lookahead():
    import movers
    from MPC import BatchMPC
    from scipy import sparse
    m, rp, car = T.build_world()
    Q, R, QN = sparse.diags([1.0, 0.0, 0.0]), sparse.diags([0.5, 0.0]), sparse.diags([1.0, 0.0, 0.0])
    ic = {'umin': np.array([0.0, -np.tan(0.66) / car.length]), 'umax': np.array([1.0, np.tan(0.66) / car.length])}
    sc = {'xmin': np.array([-np.inf] * 3), 'xmax': np.array([np.inf] * 3)}
    B, N = 8, 30
    bm = BatchMPC(car, N, Q, R, QN, sc, ic, 4.0, max_batch=B, corridor="device")
    starts = np.arange(B) * 20
    cum = np.cumsum(rp.segment_lengths)
    poses = np.array([[rp.waypoints[w].x, rp.waypoints[w].y, rp.waypoints[w].psi] for w in starts])
    mv = [[movers.Mover.along_path(cum[(w + 12) % cum.size], 0.03, 0.3, 0.04)] for w in starts]
    plain = bm.rollout(cum[starts], poses, 6, movers=mv)
    with pytest.raises(mpmpc.MpmpcError):
        bm.handle.rollout_lookahead()                                       # that rollout did not look ahead
    got = bm.rollout(cum[starts], poses, 6, movers=mv, lookahead=LK.Lookahead(25))
    lead, discs = bm.handle.rollout_lookahead()
    kappa, v_ref, ds = rp.tables()
    seg = LK.Lookahead.seg_time_of(ds, v_ref)
    assert np.array_equal(lead, LK.leads(got["wp_id"], N, seg, car.Ts, 25, n_wp=cum.size, circular=rp.circular))
    rows = [np.array([q.row(car.Ts, m.resolution) for q in c]) for c in mv]
    wps = rp.waypoints
    want = np.concatenate([LK.discs(rows[b], 5, lead[b], 0, m.origin, m.resolution, m.width, m.height, cum=cum, x=[w.x for w in wps],
                                    y=[w.y for w in wps], psi=[w.psi for w in wps], circular=rp.circular) for b in range(B)])
    assert np.array_equal(discs, want) and lead.max() > 5 and np.any(discs[:, 0] != discs[:, -1])
    again = bm.rollout(cum[starts], poses, 6, movers=mv)                    # a later rollout does not look ahead again
    assert all(np.array_equal(again[k], plain[k]) for k in plain)
    other = bm.rollout(cum[starts], poses, 6, movers=mv, lookahead=LK.Lookahead(3, np.zeros(cum.size)))      # a table of one's own
    assert all(np.array_equal(other[k], plain[k]) for k in plain) and not bm.handle.rollout_lookahead()[0].any()
    bm.close()
