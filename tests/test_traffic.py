"""Traffic in the device rollout (K0t, mpmpc_rollout_set_traffic): the cars of a group see each other as discs, computed on
the device every step from the fleet's own poses.

CPU: the host twin of K0t (tests/emul_traffic, the same traffic_core.hpp) against a restatement of the law written here
from the header in plain Python ints, the product's numpy evaluation against the twin, the three-way layout, the argument
checks.  GPU: the selection's edges on one step, one multi-step call against the step-by-step loop that uploads every car's
discs (what cars reacting to each other cost before), all three settings together, off means off, a change of law mid-run,
the recorder's rows from the trace alone."""
import ctypes as C
import math

import numpy as np
import pytest

import mpmpc
import mpmpc_testlib as T
import scenarios
import twins
from map import Map, Obstacle

E_ARG, E_STATE = -1, -3
TS = 0.05
KEYS = ("s", "pose", "cc", "wp_id", "status", "counter", "alive")


_d, _i, _i32, _g1, _sm = T._d, T._i, T._i32, T.g1_world, T.safety_margin


@pytest.fixture(scope="module")
def twin():
    """The CPU twin of K0t (tests/emul_traffic)."""
    return twins.traffic()


@pytest.fixture(scope="module")
def car_twin():
    """The CPU twin of K0c (tests/emul_car): the step-0 condition on the fleets, the recorder's rows."""
    return twins.car()


class Frame:
    """what the law reads of the map: the grid's frame"""

    def __init__(self, track):
        g1, grid, origin, res = _g1(track)
        self.ox, self.oy, self.res, self.W, self.H = origin[0], origin[1], res, int(grid.shape[1]), int(grid.shape[0])


# ------------------------------------------------------------------------------------ the law, restated from the header
def _ranked(pose, alive, group, rad, f):
    """per car b: None when b is not present, else the visible cars c != b of b's group as (d2, c, cx, cy, r), ordered by
    (d2, c) - Python ints and math.floor, in traffic_core.hpp's order"""
    B = len(alive)
    cell = [None] * B
    for c in range(B):
        if int(alive[c]) != 1 or int(group[c]) < 0:
            continue
        vx, vy = (float(pose[c][0]) - f.ox) / f.res, (float(pose[c][1]) - f.oy) / f.res
        if not (math.isfinite(vx) and math.isfinite(vy)):
            continue
        qx, qy = math.floor(vx), math.floor(vy)
        if abs(qx) > 2 ** 30 or abs(qy) > 2 ** 30:
            continue
        cell[c] = (qx, qy)
    seen = {}
    for c in range(B):
        if cell[c] is None:
            continue
        (cx, cy), r = cell[c], int(rad[c])
        if cx - r < 0 or cy - r < 0 or cx + r > f.W or cy + r > f.H:
            continue
        seen.setdefault(int(group[c]), []).append((c, cx, cy, r))
    out = [None] * B
    for b in range(B):
        if cell[b] is None:
            continue
        bx, by = cell[b]
        out[b] = sorted(((cx - bx) ** 2 + (cy - by) ** 2, c, cx, cy, r) for c, cx, cy, r in seen.get(int(group[b]), ()) if c != b)
    return out


def _slots(ranked, S, range_cells):
    out = np.zeros((len(ranked), S, 3), np.int32)
    for b, cand in enumerate(ranked):
        if cand is None:
            continue
        if range_cells >= 0:
            cand = [k for k in cand if k[0] <= range_cells * range_cells]
        for t, k in enumerate(cand[:S]):
            out[b, t] = k[2:5]
    return out


def _law(pose, alive, group, rad, S, range_cells, f):
    return _slots(_ranked(pose, alive, group, rad, f), S, range_cells)


def _twin_slots(twin, pose, alive, group, rad, S, range_cells, f):
    pose = np.ascontiguousarray(pose, float)
    B = pose.shape[0]
    out = np.full((B, S, 3), -7, np.int32)
    rc = twin.tr_emu_slots(B, _d(pose), _i(_i32(alive)), _i(_i32(group)), _i(_i32(rad)), S, range_cells, f.H, f.W, f.ox, f.oy,
                           f.res, _i(out))
    assert rc == 0
    return out


SIZES = (1024, 129, 65, 64, 63, 2, 1)
_CASES = {}


def _law_case(track):
    """one seeded fleet per track that covers the law's branches: groups of SIZES and negative groups over shuffled car
    indices, cars at the path's waypoints (a few hundred: many share a cell, and cars at the same distance on either
    side tie in d2), every value of alive, and the special cars listed below.  -> dict with the restated ranking"""
    if track in _CASES:
        return _CASES[track]
    g1, grid, origin, res = _g1(track)
    f = Frame(track)
    rng = np.random.default_rng(201 if track == "sim" else 202)
    n_neg = 40
    B = sum(SIZES) + n_neg
    group = np.concatenate([np.full(n, 7 * q + 3) for q, n in enumerate(SIZES)] + [rng.integers(-9, 0, n_neg)])
    rng.shuffle(group)
    wp = rng.integers(0, g1["x"].size, B)
    pose = np.stack([g1["x"][wp], g1["y"][wp], g1["psi"][wp]], 1)
    pose[:, :2] += rng.uniform(-0.4, 0.4, (B, 2)) * res                     # within the cell's neighbourhood
    rad = rng.integers(0, 12 if track == "sim" else 5, B)
    rad[rng.random(B) < 0.3] = 0                                            # radius 0: seen, occupies no cell
    alive = rng.choice([1, 1, 1, 1, 1, 1, 0, -1, -2, -3], B)
    big = np.nonzero(group == 3)[0]                                         # the group of 1024
    special = dict(nan=big[5], far31=big[6], far30=big[7], leaves=big[8], negative=np.nonzero(group < 0)[0][0],
                   alone=np.nonzero(group == 7 * 6 + 3)[0][0])
    alive[[special[k] for k in special]] = 1
    alive[group == 7 * 5 + 3] = 1                                           # the group of two: one candidate each
    pose[special["nan"], 0] = np.nan
    pose[special["far31"], 0] = origin[0] + res * 2.0 ** 31                 # 2^31 cells away: not present
    pose[special["far30"], 1] = origin[1] - res * (2.0 ** 30 - 3)           # within 2^30: present, not visible, d2 ~ 2^60
    rad[special["leaves"]] = f.W                                            # its square leaves the grid: it still sees
    _CASES[track] = dict(f=f, B=B, pose=pose, alive=alive, group=group, rad=rad, special=special,
                         ranked=_ranked(pose, alive, group, rad, f))
    return _CASES[track]


SETTINGS = dict(sim=((5, 60), (1, -1), (64, -1), (3, 0), (6, 9)), real=((5, 12), (1, -1), (64, -1), (3, 0), (6, 2)))


# ------------------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("track", ["sim", "real"])
def test_twin_equals_the_restated_law(track, twin):
    c = _law_case(track)
    rk, sp, grp = c["ranked"], c["special"], c["group"]
    for S, rng_cells in SETTINGS[track]:
        got = _twin_slots(twin, c["pose"], c["alive"], grp, c["rad"], S, rng_cells, c["f"])
        assert np.array_equal(got, _slots(rk, S, rng_cells)), (S, rng_cells)
    # ... and the cases are what they claim to be
    assert sorted(np.unique(grp[grp >= 0], return_counts=True)[1].tolist()) == sorted(SIZES)
    assert set(np.unique(c["alive"]).tolist()) == {1, 0, -1, -2, -3}
    for k in ("nan", "far31", "negative"):
        assert rk[sp[k]] is None
    assert rk[sp["alone"]] == []                                             # a group of one: present, sees nobody
    assert len(rk[sp["far30"]]) > 64 and rk[sp["far30"]][0][0] > 2 ** 59     # int64 distances
    assert len(rk[sp["leaves"]]) > 64                                        # not visible, yet it sees ...
    assert not any(k[1] in (sp["leaves"], sp["far30"]) for r in rk if r for k in r)      # ... and nobody sees it
    present = [r for r in rk if r is not None]
    assert any(len(r) > 5 for r in present) and any(0 < len(r) < 5 for r in present)      # more candidates than S, fewer
    ties = sum(1 for r in present if len(r) > 1 and r[0][0] == r[1][0])
    same_cell = sum(1 for r in present if r and r[0][0] == 0)
    assert ties >= 20 and same_cell >= 20                                    # the index decides
    S, cut = SETTINGS[track][0]
    n_in = [sum(1 for k in r if k[0] <= cut * cut) for r in present]
    assert any(0 < n < len(r) for n, r in zip(n_in, present))                # the range cuts some off
    assert any(k[4] == 0 for r in present for k in r[:1])                    # radius 0 is seen
    assert any(np.any(c["alive"][[k[1] for k in r]] != 1) for r in present) is False      # ended cars are not seen


@pytest.mark.parametrize("track", ["sim", "real"])
def test_product_traffic_discs_equal_the_twin(track, twin):
    import traffic
    c = _law_case(track)
    f = c["f"]
    for S, rng_cells in SETTINGS[track]:
        got = traffic.traffic_discs(c["pose"], c["alive"], c["group"], c["rad"], S, rng_cells, (f.ox, f.oy), f.res, f.W, f.H)
        want = _twin_slots(twin, c["pose"], c["alive"], c["group"], c["rad"], S, rng_cells, f)
        assert got.dtype == np.int32 and got.shape == (c["B"], S, 3) and np.array_equal(got, want), (S, rng_cells)
    # the front end: metres become cells as Mover.row does
    t = traffic.Traffic([0, 0, -1], [0.043, 0.0, 0.1], 4, range=0.31)
    grp, rad, S, rng_cells = t.cells(f.res)
    assert grp.tolist() == [0, 0, -1] and rad.tolist() == [int(np.ceil(v / f.res)) for v in (0.043, 0.0, 0.1)]
    assert S == 4 and rng_cells == math.floor(0.31 / f.res) and traffic.Traffic([0], 0.05, 1).cells(f.res)[3] == -1
    # a trace's record: present is "the pose is finite"
    pose = np.where((c["alive"] == 1)[:, None], c["pose"], np.nan)
    ok = np.all(np.isfinite(pose), 1)
    got = traffic.trace_discs(dict(pose=pose[None]), 0, c["group"], c["rad"], 5, -1, (f.ox, f.oy), f.res, f.W, f.H)
    assert np.array_equal(got, _law(pose, ok.astype(int), c["group"], c["rad"], 5, -1, f))


def test_three_way_layout_by_hand(twin):
    off, dst = np.zeros(5, np.int32), np.zeros(4, np.int32)
    st, mv = np.array([0, 2, 2, 5, 5], np.int32), np.array([0, 1, 3, 3, 4], np.int32)
    # car 0: 2 static, 1 mover, 2 slots | car 1: 0, 2, 2 | car 2: 3, 0, 2 | car 3: 0, 1, 2
    twin.tr_emu_combine(4, _i(st), _i(mv), 2, _i(off), _i(dst))
    assert off.tolist() == [0, 5, 9, 14, 17] and dst.tolist() == [2, 5, 6, 14]
    twin.tr_emu_combine(4, _i(st), _i(mv), 0, _i(off), _i(dst))               # no traffic: the two-way layout
    assert off.tolist() == [0, 3, 5, 8, 9] and dst.tolist() == [2, 3, 4, 8]
    twin.tr_emu_combine(4, None, None, 3, _i(off), _i(dst))                   # traffic alone
    assert off.tolist() == [0, 3, 6, 9, 12]
    twin.tr_emu_combine(4, _i(st), None, 1, _i(off), _i(dst))
    assert off.tolist() == [0, 3, 4, 8, 9]
    # the groups: dense numbers ascending in the group's value, members in ascending car index
    dense, goff, mem = np.full(5, -7, np.int32), np.full(6, -7, np.int32), np.full(5, -7, np.int32)
    assert twin.tr_emu_layout(5, _i(np.array([7, -1, 3, 7, 3], np.int32)), _i(dense), _i(goff), _i(mem)) == 2
    assert dense.tolist() == [1, -1, 0, 1, 0] and goff[:3].tolist() == [0, 2, 4] and mem[:4].tolist() == [2, 4, 0, 3]
    assert twin.tr_emu_layout(2, _i(np.array([-1, -2], np.int32)), _i(dense), _i(goff), _i(mem)) == 0 and goff[0] == 0


def test_set_traffic_validation_without_device(twin, built_library):
    lib = mpmpc.load_library(built_library)
    one = np.zeros(1, np.int32)
    assert lib.mpmpc_rollout_set_traffic(None, 1, _i(one), _i(one), 1, -1) == E_ARG       # no handle

    def check(group, rad, slots=2, B=None, max_batch=2048, built=1, sB=0, so=None, mB=0, mo=None):
        group, rad = _i32(group), _i32(rad)
        return twin.tr_emu_check(group.size if B is None else B, max_batch, _i(group), _i(rad), slots, built, sB, _i(_i32(so)),
                                 mB, _i(_i32(mo)))
    assert check([0, 0, -1], [3, 0, 2]) == 0
    assert check([0], [3], B=0) == E_ARG and check([0, 0, 0], [1, 1, 1], max_batch=2) == E_ARG       # B outside [1, max_batch]
    assert check([0, 0], [3, -1]) == E_ARG                                                            # a negative radius
    assert check([0, 0], [3, 1], slots=0) == E_ARG and check([0, 0], [3, 1], slots=65) == E_ARG
    assert check([0, 0], [3, 1], slots=1) == 0 and check([0, 0], [3, 1], slots=64) == 0
    assert twin.tr_emu_check(2, 8, _i(_i32([0, 0])), None, 2, 1, 0, None, 0, None) == E_ARG            # radius_cells NULL
    assert check([0, 0], [3, 1], built=0) == E_STATE                                                  # no build of this map
    assert check([5] * 1024 + [6], [0] * 1025) == 0                                                   # the cap itself
    assert check([5] * 1025, [0] * 1025) == E_ARG                                                     # a group over it
    assert check([5] * 1025 + [-1] * 3, [0] * 1028, max_batch=4096) == E_ARG
    assert check([-1] * 1500, [0] * 1500) == 0                                                        # (negative: no group)
    # static discs + movers + slots share the 64 entries of a car; all settings for the same B
    assert check([0, 0], [1, 1], slots=4, sB=2, so=[0, 60, 60]) == 0
    assert check([0, 0], [1, 1], slots=5, sB=2, so=[0, 60, 60]) == E_ARG
    assert check([0, 0], [1, 1], slots=4, sB=2, so=[0, 30, 60], mB=2, mo=[0, 30, 60]) == 0
    assert check([0, 0], [1, 1], slots=5, sB=2, so=[0, 30, 60], mB=2, mo=[0, 29, 59]) == E_ARG       # the second car: 30 + 30 + 5
    assert check([0, 0], [1, 1], slots=4, sB=2, so=[0, 30, 60], mB=2, mo=[0, 29, 60]) == E_ARG       # 30 + 31 + 4
    assert check([0, 0], [1, 1], slots=64) == 0 and check([0, 0], [1, 1], slots=64, mB=2, mo=[0, 0, 1]) == E_ARG
    assert check([0, 0], [1, 1], sB=3, so=[0, 1, 2, 3]) == E_STATE and check([0, 0], [1, 1], mB=1, mo=[0, 1]) == E_STATE
    # ... and the same rules from the other two setters' side
    comb = lambda sB, so, mB, mo, tB, S: twin.tr_emu_check_combined(sB, _i(_i32(so)), mB, _i(_i32(mo)), tB, S)
    assert comb(1, [0, 60], 0, None, 1, 4) == 0 and comb(1, [0, 61], 0, None, 1, 4) == E_ARG
    assert comb(1, [0, 30], 1, [0, 30], 1, 4) == 0 and comb(1, [0, 30], 1, [0, 31], 1, 4) == E_ARG
    assert comb(2, [0, 1, 2], 0, None, 1, 4) == E_STATE and comb(0, None, 2, [0, 1, 2], 3, 4) == E_STATE
    assert comb(2, [0, 1, 2], 0, None, 0, 4) == 0 and comb(1, [0, 61], 1, [0, 3], 0, 9) == 0 and comb(1, [0, 61], 1, [0, 4], 0, 0) == E_ARG
    line = np.array([[0.5, 0.5, 0.01, 0.0]] * 5)
    kind, rad = np.zeros(5, np.int32), np.full(5, 3, np.int32)
    mov = lambda n, sB, so, tB, S: twin.tr_emu_check_movers(1, 8, _i(_i32([0, n])), _i(kind), _i(rad), _d(line), 1, sB,
                                                            _i(_i32(so)), tB, S)
    assert mov(4, 1, [0, 50], 1, 10) == 0 and mov(5, 1, [0, 50], 1, 10) == E_ARG and mov(5, 0, None, 1, 59) == 0
    assert mov(5, 0, None, 1, 60) == E_ARG and mov(1, 0, None, 2, 4) == E_STATE


def test_set_traffic_is_exported(built_library):
    assert "mpmpc_rollout_set_traffic" in mpmpc.EXPORTS
    assert hasattr(C.CDLL(built_library), "mpmpc_rollout_set_traffic")
    assert hasattr(mpmpc.Handle, "rollout_set_traffic")


# ------------------------------------------------------------------------------------------------------------ GPU
def _handle(track, N, B, warm=False):
    tr = scenarios.sim_track() if track == "sim" else scenarios.real_track()
    g1, grid, origin, res = _g1(track)
    h = mpmpc.Handle(T.stock_config(N, max_batch=B, track=None if track == "sim" else tr), mpmpc.default_settings())
    h.set_path(tr.kappa, tr.v_ref, tr.ds_next)
    h.set_map(grid, origin, res)
    h.set_path_geometry(g1["x"], g1["y"], g1["psi"], g1["border_ub"], g1["border_lb"])
    h.rollout_warm_start(warm)
    sm = _sm(track)
    tabs = h.build_corridor(N, 2 * sm, sm)
    return h, tabs


def _twin_rows(car_twin, track, disc_lists, wp_ids, N):
    """(ub, lb, flag) of K0c's twin for one disc list and waypoint per car"""
    g1, grid, origin, res = _g1(track)
    sm = _sm(track)
    arrs = [np.ascontiguousarray(g1[k], float) for k in ("x", "y", "psi", "ds_next", "border_ub", "border_lb")]
    off, flat = T.csr(disc_lists, 3, pad=False)
    B = len(disc_lists)
    wp = np.ascontiguousarray(wp_ids, np.int32)
    ub, lb, flag = np.zeros((B, N)), np.zeros((B, N)), np.zeros(B, np.int32)
    rc = car_twin.car_emu_rows(grid.shape[0], grid.shape[1], grid.ctypes.data_as(C.POINTER(C.c_int8)), origin[0], origin[1],
                               res, arrs[0].size, *[_d(a) for a in arrs[:4]], 1 if track == "sim" else 0, _d(arrs[4]),
                               _d(arrs[5]), N, 2 * sm, sm, B, _i(wp), _i(off), _i(flat), _d(ub), _d(lb), _i(flag))
    assert rc == 0
    return ub, lb, flag


BASE = dict(sim=[(0.0, 0.0, 0.05), (-0.8, -0.5, 0.08), (-0.7, -1.5, 0.05), (-0.3, -1.0, 0.08), (0.27, -1.0, 0.05),
                 (0.78, -1.47, 0.05), (0.73, -0.9, 0.07), (1.2, 0.0, 0.08), (0.67, -0.05, 0.06)])

# per track: N, B, steps, seed, the big group (cars, of which with a real radius), the small groups, singletons
SHAPES = dict(sim=(30, 192, 40, 71, (130, 12), (2, 3, 4, 6, 8, 12), 12),
              real=(70, 64, 20, 72, (0, 0), (10, 8, 6, 5, 4, 3, 2, 2), 12))
GAPS = (4, 11)       # waypoints between neighbours of a small group (rng.integers: 4 .. 10)
S7 = 6


class Fleet:
    """B cars on a track.  One big group at random waypoints of which a dozen have a real radius (the rest radius 0: a
    group that size with real discs at 0.044 m waypoint spacing blocks itself), small groups whose cars follow each other
    GAPS waypoints apart in the same lane, singletons, and cars with a negative group; headings jittered.  The range is
    the median distance of the big group's cars to their (S + 1)-th nearest visible neighbour: about half of them have more
    than S candidates in range, half fewer.  extras: also 2 static discs and 2 movers along the path per car.  Cars
    whose step-0 row the K0c twin finds blocked are drawn again (same generator)."""

    def __init__(self, track, car_twin, extras=False, shape=None):
        N, B, steps, seed, (n_big, n_real), small, n_single = shape or SHAPES[track]
        self.track, self.N, self.B, self.steps = track, N, B, steps
        g1, grid, origin, res = _g1(track)
        self.f = Frame(track)
        self.origin, self.res = origin, res
        sim = track == "sim"
        tr = scenarios.sim_track() if sim else scenarios.real_track()
        self.cum = np.cumsum(g1["segment_lengths"])
        n_wp = g1["x"].size
        rng = np.random.default_rng(seed)
        hi = n_wp if sim else n_wp - N - steps // 2 - 5
        rr = (0.03, 0.05) if sim else (0.15, 0.25)
        cells = lambda radius: int(np.ceil(radius / res))
        group, rad, lead = np.full(B, -1), np.zeros(B, int), np.full(B, -1)
        starts = rng.integers(0, hi, B)
        group[:n_big] = 0
        rad[:n_real] = [cells(rng.uniform(*rr)) for _ in range(n_real)]
        b = n_big
        for q, n in enumerate(small):
            w0 = int(rng.integers(0, hi if sim else max(1, hi - 10 * n)))
            for k in range(n):
                group[b], rad[b], lead[b] = 1 + q, cells(rng.uniform(*rr)), b - k
                starts[b] = w0 if k == 0 else starts[b - 1] + int(rng.integers(*GAPS))
                b += 1
        for k in range(n_single):
            group[b], rad[b] = 100 + k, cells(rng.uniform(*rr))
            b += 1
        group[b:] = -1 - rng.integers(0, 3, B - b)
        rad[b:] = cells(rr[0])
        starts = starts % n_wp if sim else np.minimum(starts, hi - 1)
        self.group, self.rad = group.astype(np.int32), rad.astype(np.int32)
        self.jitter = rng.uniform(-0.05, 0.05, B)
        m = Map.from_grid(grid, origin, res)

        def extras_of(b_):
            w0 = int(starts[b_])
            pick = rng.choice(len(BASE["sim"]), 2, replace=False)
            static = m.obstacle_discs([Obstacle(BASE["sim"][q][0] + rng.uniform(-0.05, 0.05), BASE["sim"][q][1] + rng.uniform(-0.05, 0.05),
                                                BASE["sim"][q][2] * rng.uniform(0.8, 1.2)) for q in pick])
            rows = [(1, cells(rng.uniform(*rr)), self.cum[(w0 + int(rng.integers(5, 26))) % n_wp], rng.uniform(-0.08, 0.08),
                     rng.uniform(1 / 3, 2 / 3) * tr.v_ref[w0] * TS, 0.0) for _ in range(2)]
            return static, np.array(rows, float)
        self.extras = extras
        self.world = None
        if extras:
            import movers
            self.world = dict(cum=self.cum, x=g1["x"], y=g1["y"], psi=g1["psi"], circular=True)
            self._mv = lambda rows, j: movers.mover_discs_rows(rows, j, origin, res, self.f.W, self.f.H, **self.world)
            ex = [extras_of(b_) for b_ in range(B)]
        big = np.arange(n_big)
        for _ in range(30):
            self.starts = starts
            self.poses = np.stack([g1["x"][starts], g1["y"][starts], g1["psi"][starts] + self.jitter], 1)
            rk = _ranked(self.poses, np.ones(B, int), group, rad, self.f)
            self.range_cells = int(math.isqrt(int(np.median([rk[c][S7][0] for c in big])))) if n_big else (60 if sim else 40)
            if extras:
                self.static, self.rows = [e[0] for e in ex], [e[1] for e in ex]
            flag = _twin_rows(car_twin, track, self.discs_of(dict(pose=self.poses, alive=np.ones(B, int)), 0, S7, self.range_cells),
                              starts, N)[2]
            bad = np.nonzero(flag != 0)[0]
            if bad.size == 0:
                break
            starts = starts.copy()
            for b_ in bad:
                if lead[b_] >= 0 and lead[b_] != b_:
                    n = int(np.sum(lead == lead[b_]))
                    starts[b_] = starts[lead[b_]] + int(rng.integers(GAPS[0], GAPS[1] * n))
                else:
                    starts[b_] = int(rng.integers(0, hi))
                starts[b_] = starts[b_] % n_wp if sim else min(starts[b_], hi - 1)
                if extras:
                    ex[b_] = extras_of(b_)
        assert bad.size == 0          # no car's row is blocked (or overflows) at step 0

    def traffic_of(self, st, S, range_cells):
        """[B, S, 3]: the slots of the state a step finds (the restated law)"""
        return _law(st["pose"], st["alive"], self.group, self.rad, S, range_cells, self.f)

    def discs_of(self, st, k, S, range_cells, traffic=True):
        """per car: its static discs, its movers' discs of step k (extras), then its traffic slots"""
        tr = self.traffic_of(st, S, range_cells) if traffic else np.zeros((self.B, 0, 3), np.int32)
        if not self.extras:
            return [tr[b] for b in range(self.B)]
        return [np.concatenate([self.static[b], self._mv(self.rows[b], k), tr[b]]) for b in range(self.B)]

    def init(self, h):
        h.rollout_init(TS, self.cum, self.cum[self.starts], self.poses)

    def set_traffic(self, h, S=S7, range_cells=None):
        h.rollout_set_traffic(self.group, self.rad, S, self.range_cells if range_cells is None else range_cells)

    def loop(self, h, steps, law, k0=0):
        """the step-by-step loop: law(k) -> (S, range_cells) of step k, or None for no traffic; the discs of every step
        computed on the host from rollout_state() and uploaded as static discs.  -> the last step's disc lists"""
        for k in range(k0, k0 + steps):
            lw = law(k)
            discs = self.discs_of(h.rollout_state(), k, *(lw or (0, -1)), traffic=lw is not None)
            h.rollout_set_obstacles(discs)
            h.rollout_step(1)
        return discs


def _same(a, b):
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k


def _rows_same(a, b):
    assert np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1], equal_nan=True)


def legs(fl, law, steps, calls=None):
    """A: set_traffic + one call per entry of `calls` [(steps, S, range_cells)]; L: the loop on a second handle"""
    h, _ = _handle(fl.track, fl.N, fl.B)
    if fl.extras:
        h.rollout_set_obstacles(fl.static)
        h.rollout_set_movers(fl.rows)
    fl.init(h)
    for n, S, rc in calls or [(steps, S7, fl.range_cells)]:
        fl.set_traffic(h, S, rc)
        h.rollout_step(n)
    out = dict(A=h.rollout_state(), A_rows=h.rollout_corridor(), A_discs=h.rollout_obstacles(), h=h)
    h2, _ = _handle(fl.track, fl.N, fl.B)
    fl.init(h2)
    out["L_discs"] = fl.loop(h2, steps, law)
    out["L"], out["L_rows"] = h2.rollout_state(), h2.rollout_corridor()
    h2.close()
    return out


@pytest.fixture(scope="module")
def runs(car_twin):
    """per track, computed once: A one call with traffic; L the step-by-step loop on a second handle; W the same fleet
    without traffic on the first handle (per-car rows without discs)"""
    cache = {}

    def get(track):
        if track not in cache:
            fl = Fleet(track, car_twin)
            out = legs(fl, lambda k: (S7, fl.range_cells), fl.steps)
            h = out.pop("h")
            h.rollout_set_traffic(None)
            h.rollout_set_obstacles([np.zeros((0, 3), np.int32)] * fl.B)
            fl.init(h)
            h.rollout_step(fl.steps)
            out["W"], out["W_rows"] = h.rollout_state(), h.rollout_corridor()
            h.close()
            out["fleet"] = fl
            cache[track] = out
        return cache[track]
    return get


@pytest.mark.gpu
def test_selection_edges_on_one_step():
    """B = 1 400 cars at random waypoints of Sim_Track's 200 (seven to a waypoint: ties and shared cells), groups of 1024,
    129, 65, 64, 63, 2, 1 and negative ones over shuffled indices, radius 0 (no row is blocked): lane striding past 64 and
    128 members, the LDS cap, the tie-break"""
    N, B = 10, 1400
    g1, grid, origin, res = _g1("sim")
    f = Frame("sim")
    rng = np.random.default_rng(81)
    group = np.concatenate([np.full(n, 11 * q) for q, n in enumerate(SIZES)] + [rng.integers(-4, 0, B - sum(SIZES))])
    rng.shuffle(group)
    wp = rng.integers(0, g1["x"].size, B)
    poses = np.stack([g1["x"][wp], g1["y"][wp], g1["psi"][wp] + rng.uniform(-0.05, 0.05, B)], 1)
    cum = np.cumsum(g1["segment_lengths"])
    rad = np.zeros(B, np.int32)
    rk = _ranked(poses, np.ones(B, int), group, rad, f)
    assert sum(1 for r in rk if r and len(r) > 1 and r[0][0] == r[1][0]) >= 500
    h, _ = _handle("sim", N, 1408)
    one = [np.array([[10, 10, 0]], np.int32)] * B                            # a static disc that occupies no cell
    for S, rng_cells, static in ((1, -1, one), (5, 14, one), (5, -1, one), (1, 14, one), (64, -1, None), (64, 30, None)):
        h.rollout_set_obstacles(static)
        h.rollout_set_traffic(group, rad, S, rng_cells)
        h.rollout_init(TS, cum, cum[wp], poses)
        h.rollout_step(1)
        got = h.rollout_obstacles()
        want = _slots(rk, S, rng_cells)
        if rng_cells >= 0:
            n_in = [sum(1 for k in r if k[0] <= rng_cells ** 2) for r in rk if r]
            assert any(0 < n < len(r) for n, r in zip(n_in, [r for r in rk if r]))           # the range cuts
        for b in range(B):
            mine = got[b] if static is None else got[b][1:]
            assert got[b].shape == (S + (static is not None), 3) and np.array_equal(mine, want[b]), (S, rng_cells, b)
            assert static is None or np.array_equal(got[b][0], (10, 10, 0))
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("track", ["sim", "real"])
def test_one_call_equals_the_step_by_step_loop(track, runs):
    r = runs(track)
    fl = r["fleet"]
    L, W = r["L"], r["W"]
    differs = np.zeros(fl.B, bool)
    for k in KEYS:
        differs |= np.any((L[k] != W[k]).reshape(fl.B, -1), 1)
    for q in (0, 1):
        differs |= ~np.all((r["L_rows"][q] == r["W_rows"][q]) | (np.isnan(r["L_rows"][q]) & np.isnan(r["W_rows"][q])), 1)
    print("alive (L):", dict(zip(*[a.tolist() for a in np.unique(L["alive"], return_counts=True)])), "differ from W:", int(differs.sum()))
    _same(r["A"], L)
    _rows_same(r["A_rows"], r["L_rows"])
    # the conditions, on the comparison leg
    assert np.isin(L["alive"], (0, 1)).sum() * 2 >= fl.B
    assert not np.any(L["alive"] == -4)
    assert differs.sum() >= 16
    if track == "sim":
        rk = _ranked(fl.poses, np.ones(fl.B, int), fl.group, fl.rad, fl.f)
        n_in = [sum(1 for k in rk[b] if k[0] <= fl.range_cells ** 2) for b in range(130)]
        assert any(n > S7 for n in n_in) and any(n < S7 for n in n_in)


@pytest.mark.gpu
def test_all_three_settings_together(car_twin):
    fl = Fleet("sim", car_twin, extras=True)
    r = legs(fl, lambda k: (S7, fl.range_cells), fl.steps)
    r.pop("h").close()
    _same(r["A"], r["L"])
    _rows_same(r["A_rows"], r["L_rows"])
    assert len(r["A_discs"]) == fl.B
    for b in range(fl.B):                                     # the last step's lists: static, movers, traffic
        assert r["A_discs"][b].dtype == np.int32 and np.array_equal(r["A_discs"][b], r["L_discs"][b]), b
        assert np.array_equal(r["A_discs"][b][:2], fl.static[b]) and r["A_discs"][b].shape[0] == 4 + S7
    assert np.isin(r["L"]["alive"], (0, 1)).sum() * 2 >= fl.B


@pytest.mark.gpu
def test_off_means_off(runs):
    r = runs("sim")
    fl = r["fleet"]
    h, _ = _handle("sim", fl.N, fl.B)
    fl.set_traffic(h)
    fl.init(h)
    h.rollout_step(5)
    h.rollout_set_traffic(None)
    fl.init(h)
    h.rollout_step(fl.steps)
    off = h.rollout_state()
    with pytest.raises(mpmpc.MpmpcError):
        h.rollout_corridor()                                  # no per-car setting: the shared table
    with pytest.raises(mpmpc.MpmpcError):
        h.rollout_obstacles()
    # refusals leave the setting in force
    fl.set_traffic(h)
    with pytest.raises(mpmpc.MpmpcError, match="64"):
        h.rollout_set_obstacles([np.tile([[10, 10, 0]], (64 - S7 + 1, 1))] * fl.B)
    with pytest.raises(mpmpc.MpmpcError, match="different numbers of cars"):
        h.rollout_set_obstacles([np.zeros((0, 3), np.int32)] * (fl.B - 1))
    with pytest.raises(mpmpc.MpmpcError, match="slots"):
        h.rollout_set_traffic(fl.group, fl.rad, 65, -1)
    with pytest.raises(mpmpc.MpmpcError, match="negative"):
        h.rollout_set_traffic(fl.group, -1 - fl.rad, 3, -1)
    fl.init(h)
    h.rollout_step(fl.steps)
    _same(h.rollout_state(), r["A"])
    h.close()
    h2, _ = _handle("sim", fl.N, fl.B)                        # a handle that never set traffic
    fl.init(h2)
    h2.rollout_step(fl.steps)
    never = h2.rollout_state()
    h2.close()
    _same(off, never)
    _same(off, r["W"])                                        # (and per-car rows without discs are the table's rows)


@pytest.mark.gpu
def test_changing_traffic_mid_run(runs):
    fl = runs("sim")["fleet"]
    other = (3, 2 * fl.range_cells)
    r = legs(fl, lambda k: (S7, fl.range_cells) if k < 10 else other, 20, calls=[(10, S7, fl.range_cells), (10,) + other])
    r.pop("h").close()
    _same(r["A"], r["L"])
    _rows_same(r["A_rows"], r["L_rows"])
    for b in range(fl.B):
        assert np.array_equal(r["A_discs"][b], r["L_discs"][b]), b
    assert np.isin(r["L"]["alive"], (0, 1)).sum() * 2 >= fl.B


@pytest.mark.gpu
def test_recorded_rows_follow_from_the_trace_alone(car_twin):
    import traffic
    shape = (30, 64, 12, 73, (0, 0), (2, 3, 4, 6, 8, 12), 12)
    fl = Fleet("sim", car_twin, shape=shape)
    f = fl.f
    h, _ = _handle("sim", fl.N, fl.B)
    h.rollout_record(fl.steps, rows=True, B=fl.B)
    fl.set_traffic(h)
    fl.init(h)
    h.rollout_step(fl.steps)
    tr = h.rollout_trace()
    h.close()
    n_rows = n_seen = 0
    for k in range(fl.steps):
        discs = traffic.trace_discs(tr, k, fl.group, fl.rad, S7, fl.range_cells, (f.ox, f.oy), f.res, f.W, f.H)
        have = ~np.isnan(tr["ub"][k][:, 0])
        ub, lb, flag = _twin_rows(car_twin, "sim", [discs[b] for b in range(fl.B)], np.maximum(tr["wp_id"][k], 0), fl.N)
        assert np.all(flag[have] == 0)
        assert np.array_equal(tr["ub"][k][have], ub[have]) and np.array_equal(tr["lb"][k][have], lb[have]), k
        n_rows += int(have.sum())
        n_seen += int(np.any(discs[have][:, :, 2] > 0, 1).sum())
    assert n_rows * 2 >= fl.B * fl.steps and n_seen * 8 >= n_rows      # (and the rows were worth comparing)


@pytest.mark.gpu
def test_batch_mpc_rollout_takes_traffic():
    import traffic
    from MPC import BatchMPC
    from scipy import sparse
    m, rp, car = T.build_world()
    Q, R, QN = sparse.diags([1.0, 0.0, 0.0]), sparse.diags([0.5, 0.0]), sparse.diags([1.0, 0.0, 0.0])
    ic = {'umin': np.array([0.0, -np.tan(0.66) / car.length]), 'umax': np.array([1.0, np.tan(0.66) / car.length])}
    sc = {'xmin': np.array([-np.inf] * 3), 'xmax': np.array([np.inf] * 3)}
    B = 8
    bm = BatchMPC(car, 30, Q, R, QN, sc, ic, 4.0, max_batch=B, corridor="device")
    starts = np.arange(B) * 20
    cum = np.cumsum(rp.segment_lengths)
    poses = np.array([[rp.waypoints[w].x, rp.waypoints[w].y, rp.waypoints[w].psi] for w in starts])
    plain = bm.rollout(cum[starts], poses, 6)
    tf = traffic.Traffic([0, 0, 0, 0, 1, 1, -1, 2], 0.04, 2, range=2.0)
    bm.rollout(cum[starts], poses, 1, traffic=tf)
    got = bm.handle.rollout_obstacles()
    grp, rad, S, rc = tf.cells(m.resolution)
    assert rad.tolist() == [8] * B and S == 2 and rc == 400
    want = traffic.traffic_discs(poses, np.ones(B, int), grp, rad, S, rc, m.origin, m.resolution, m.width, m.height)
    assert np.array_equal(np.array(got), want) and np.array_equal(want, _law(poses, np.ones(B, int), grp, rad, S, rc, Frame("sim")))
    assert (want[:4, :, 2] > 0).any() and not want[6:].any()
    with pytest.raises(ValueError):
        bm.rollout(cum[starts], poses, 1, traffic=traffic.Traffic([0, 0], 0.04, 2))
    again = bm.rollout(cum[starts], poses, 6)                               # a later rollout has no traffic again
    assert all(np.array_equal(again[k], plain[k]) for k in plain)
