"""Route fleets (mpmpc_set_routes / mpmpc_set_car_routes): the path tables of a handle are the concatenation of several routes
and every instance names the route it is on; wp_id is local to the route.

Two oracles, neither the code under test.  A = solo handles: the cars of each route through a single-path handle on that
route's own tables - the code path that existed before routes.  B = copies: P identical copies of one path concatenated, cars
dealt round-robin, against the whole fleet on a single-path handle.

Fixture routes, all from the committed goldens on Sim_Track: L = the lap (200 waypoints, circular), A = its rows 0 .. 119 as
an open route, Bo = rows 100 .. 199 as an open route, S = rows 0 .. 19 as a circular route (n <= N at N = 30: the modulo
branch of the wrap).

Tolerances: the project's own.  K1's output and corridor tables are compared array_equal (the same arithmetic on the same
table entries: only the indices differ).  A solve: status and iters equal, u0 and z to 1e-9 - the permutation test of
tests/test_gpu_parity.py: an instance's answer may depend on its place in the wave through the wave-wide reductions of the
packed layouts, to rounding.  Against the solo handles on the fixture routes the solves came out bit-equal at every shape
tried (max |du0| = max |dz| = 0, MI355X), so those are asserted array_equal; the end-to-end test keeps the 1e-9.  A rollout:
wp_id, status, alive, counter (and the audit's and perception's step indices and masks) equal; s, pose, u and every other real
of the state, the audit and the trace to 1e-8 - the device-against-host rollout bound of DESIGN (K3)."""
import ctypes as C
import os

import numpy as np
import pytest

import mpmpc
import mpmpc_testlib as T
import scenarios
import twins

bp = C.POINTER(C.c_int8)
E_ARG, E_STATE = -1, -3
NF = mpmpc.NUM_FIELDS


_d, _i = T._d, T._i


# ------------------------------------------------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def twin():
    """The CPU twin of the route view (tests/emul_routes)."""
    return twins.routes()


SPANS = {"L": (0, 200, 1), "A": (0, 120, 0), "Bo": (100, 200, 0), "S": (0, 20, 1)}      # rows [lo, hi) of the lap, circular


class Routes:
    """Some of the fixture routes: each route's own tables (what a solo handle gets) and their concatenation."""

    def __init__(self, track, names, n_cols=30):
        self.names = list(names)
        self.P = len(self.names)
        self.circular = np.array([SPANS[k][2] for k in self.names], np.int32)
        self.own = []
        for k in self.names:
            lo, hi, _ = SPANS[k]
            cum = np.cumsum(track.segment_lengths)[lo:hi]
            self.own.append(dict(kappa=track.kappa[lo:hi].copy(), v_ref=track.v_ref[lo:hi].copy(), ds_next=track.ds_next[lo:hi].copy(),
                                 ub=np.ascontiguousarray(track.ub_free[lo:hi, :n_cols]), lb=np.ascontiguousarray(track.lb_free[lo:hi, :n_cols]),
                                 x=track.x[lo:hi].copy(), y=track.y[lo:hi].copy(), psi=track.psi[lo:hi].copy(), cum_lengths=cum))
        self.all, self.first = mpmpc.concat_routes(self.own)
        self.n = np.diff(self.first)

    def header(self, route):
        """PathTables::route of the cars: {first row, length - negated on an open route}"""
        route = np.asarray(route)
        return np.ascontiguousarray(np.stack([self.first[route], np.where(self.circular[route] != 0, 1, -1) * self.n[route]], 1), np.int32)


@pytest.fixture(scope="module")
def track():
    return scenarios.sim_track()


def edge_waypoints(n, N):
    """local wp 0, 1, n-N-1, n-N, n-2, n-1 of a route of n waypoints (those that exist)"""
    return sorted({w for w in (0, 1, n - N - 1, n - N, n - 2, n - 1) if 0 <= w < n})


def cars(B, N, seed, track):
    """x0 [B, 3] and previous plans cc [B, 2N] of B cars: small lateral and heading errors, half the plans cold (zeros)"""
    rng = np.random.default_rng(seed)
    x0 = np.stack([0.02 * rng.uniform(-1, 1, B), rng.uniform(-0.2, 0.2, B), np.zeros(B)], 1)
    cc = np.zeros((B, 2 * N))
    warm = np.arange(B) % 2 == 1
    cc[:, 0::2] = np.where(warm[:, None], rng.uniform(0.3, 1.0, (B, N)), 0.0)
    cc[:, 1::2] = np.where(warm[:, None], rng.uniform(-0.3, 0.3, (B, N)), 0.0)
    return np.ascontiguousarray(x0), cc


# ------------------------------------------------------------------------------------------------------------ CPU: the twin
def _twin_fields(twin, cfg, tab, header, group, pair, wp, x0, cc):
    B, N = wp.size, cfg.N
    out = np.full((B, N + 1, NF), np.nan)
    rc = twin.routes_emu_fields(C.byref(cfg), tab["kappa"].size, _d(tab["kappa"]), _d(tab["v_ref"]), _d(tab["ds_next"]), tab["ub"].shape[1],
                                _d(tab["ub"]), _d(tab["lb"]), _i(header), B, group, pair, _i(wp), _d(x0), _d(cc), _d(out))
    assert rc == 0
    return out


@pytest.mark.parametrize("N", [10, 30])
def test_twin_route_view_matches_each_routes_own_table(N, twin, track):
    """assemble_fields<LaneEmu> with the route view on L+A+Bo+S against the same code WITHOUT a view on each route's own tables
    (n_wp := n, circular := the route's): all 27 fields of every stage bit-equal, at local wp 0, 1, n-N-1, n-N, n-2, n-1 of every
    route, with one, two and four instances per emulated wave and with two stages per lane.  (The twin skips the upload's
    "Reached end of path!" check: the clamp of an open route is exercised up to its last waypoint.)"""
    R = Routes(track, ["L", "A", "Bo", "S"], n_cols=N)
    per = [edge_waypoints(int(n), N) for n in R.n]
    reps = max(len(w) for w in per)
    route = np.array([p for _ in range(reps) for p in range(R.P)], np.int32)          # interleaved: neighbours differ in route
    wp = np.array([per[p][j % len(per[p])] for j in range(reps) for p in range(R.P)], np.int32)
    x0, cc = cars(route.size, N, 11, track)
    want = np.full((route.size, N + 1, NF), np.nan)
    for p in range(R.P):
        idx = np.flatnonzero(route == p)
        cfg = T.stock_config(N, max_batch=idx.size, circular=bool(R.circular[p]))
        want[idx] = _twin_fields(twin, cfg, R.own[p], None, 64, 0, np.ascontiguousarray(wp[idx]), np.ascontiguousarray(x0[idx]),
                                 np.ascontiguousarray(cc[idx]))
    assert not np.isnan(want).any()          # every stage of every car was written (the state boxes are infinite: not NaN)
    for circ in (False, True):          # the handle-wide flag is ignored while routes are set
        cfg = T.stock_config(N, max_batch=route.size, circular=circ)
        for group, pair in ((64, 0), (32, 0), (16, 0), (16, 1)) if N == 10 else ((64, 0), (32, 0), (16, 1)):
            got = _twin_fields(twin, cfg, R.all, R.header(route), group, pair, wp, x0, cc)
            assert np.array_equal(got, want), (circ, group, pair)


def test_twin_waypoint_arithmetic_on_route_slices(twin, track):
    """ro_current_waypoint and ro_past_open_end on a route's slice of the concatenated cum_lengths against the solo call on the
    route's own array: every waypoint of every route, at arc length 0, at each cum midpoint -1 / 0 / +1 ulp and at the route's
    length -1 / 0 / +1 ulp."""
    R = Routes(track, ["L", "A", "Bo", "S"])
    cum = np.ascontiguousarray(R.all["cum_lengths"])
    for p in range(R.P):
        own = np.ascontiguousarray(R.own[p]["cum_lengths"] - R.own[p]["cum_lengths"][0])
        n, f = int(R.n[p]), int(R.first[p])
        assert np.array_equal(cum[f:f + n], own) and own[0] == 0.0
        mids = (own[1:] + own[:-1]) / 2
        probes = [0.0] + [v for m in list(mids) + [own[-1]] for v in (np.nextafter(m, -np.inf), m, np.nextafter(m, np.inf))]
        for s in probes:
            assert twin.routes_emu_current_waypoint(_d(cum), f, n, s) == twin.routes_emu_current_waypoint(_d(own), 0, n, s), (p, s)
        for N in (10, 30):
            for w in range(n):
                assert twin.routes_emu_past_open_end(n, N, int(R.circular[p]), w) == int(not R.circular[p] and w + N >= n)


def _g1_world(name="obstacles"):
    g1 = np.load(os.path.join(T.GOLDEN, "g1_path_sim_track.npz"))
    g3 = np.load(os.path.join(T.GOLDEN, "g3_corridor.npz"))
    h, w = g1["grid_shape"]
    grid = np.ascontiguousarray(np.unpackbits(g1["grid_" + name])[:h * w].reshape(h, w).astype(np.int8))
    return g1, grid, float(g3["safety_margin"][0])


def _geometry(g1, names):
    own = []
    for k in names:
        lo, hi, _ = SPANS[k]
        own.append({key: np.ascontiguousarray(g1[key][lo:hi], float) for key in ("x", "y", "psi", "ds_next", "kappa", "border_ub", "border_lb")})
    return own


def test_twin_corridor_walk_through_route_views(twin, emu):
    """cor_forced / cor_select through the per-route PathGeom view - offset base pointers into the concatenated geometry and
    into K0a's caches by global row, the route's length and circular flag - against the emulation's single-path corridor build
    on each route's own arrays: every start waypoint of L+A+Bo, 30 columns, on the map with obstacles; array_equal (NaN rows
    included)."""
    g1, grid, sm = _g1_world()
    names = ["L", "A", "Bo"]
    own = _geometry(g1, names)
    cat, first = mpmpc.concat_routes(own)
    circ = np.array([SPANS[k][2] for k in names], np.int32)
    n_cols, n = 30, int(first[-1])
    ub, lb = np.zeros((n, n_cols)), np.zeros((n, n_cols))
    bad = twin.routes_emu_corridor(grid.shape[0], grid.shape[1], grid.ctypes.data_as(bp), -1.0, -2.0, 0.005, n, _d(cat["x"]), _d(cat["y"]),
                                   _d(cat["psi"]), _d(cat["ds_next"]), len(names), _i(first), _i(circ), _d(cat["border_ub"]),
                                   _d(cat["border_lb"]), n_cols, 2 * sm, sm, _d(ub), _d(lb))
    assert bad >= 0
    bad_solo = 0
    for p, o in enumerate(own):
        m = o["x"].size
        u1, l1 = np.zeros((m, n_cols)), np.zeros((m, n_cols))
        b = emu.lib.emu_corridor(C.c_int(grid.shape[0]), C.c_int(grid.shape[1]), grid.ctypes.data_as(bp), C.c_double(-1.0), C.c_double(-2.0),
                                 C.c_double(0.005), C.c_int(m), _d(o["x"]), _d(o["y"]), _d(o["psi"]), _d(o["ds_next"]), C.c_int(int(circ[p])),
                                 _d(o["border_ub"]), _d(o["border_lb"]), C.c_int(n_cols), C.c_double(2 * sm), C.c_double(sm), _d(u1), _d(l1), None)
        assert b >= 0
        bad_solo += b
        f = int(first[p])
        assert np.array_equal(ub[f:f + m], u1, equal_nan=True) and np.array_equal(lb[f:f + m], l1, equal_nan=True), names[p]
    assert bad == bad_solo


def test_concat_routes(track):
    R = Routes(track, ["L", "A", "Bo", "S"])
    assert R.first.tolist() == [0, 200, 320, 420, 440] and R.first.dtype == np.int32
    for key in ("kappa", "v_ref", "ds_next", "x", "ub"):
        assert np.array_equal(R.all[key], np.concatenate([o[key] for o in R.own]))
    for p in range(R.P):
        seg = R.all["cum_lengths"][R.first[p]:R.first[p + 1]]
        assert seg[0] == 0.0 and np.array_equal(seg, R.own[p]["cum_lengths"] - R.own[p]["cum_lengths"][0])
    # scalars and arrays of another length are left out; a tuple from ReferencePath.tables() goes in as a dict
    tabs, first = mpmpc.concat_routes([dict(kappa=np.zeros(3), n_wp=3, length=1.5, other=np.zeros(5)), dict(kappa=np.ones(2), n_wp=2, length=2.5, other=np.zeros(5))])
    assert sorted(tabs) == ["kappa"] and first.tolist() == [0, 3, 5]
    tabs, first = mpmpc.concat_routes([(np.zeros(3), np.ones(3), np.ones(3)), (np.ones(2), np.ones(2), np.zeros(2))])
    assert sorted(tabs) == ["ds_next", "kappa", "v_ref"] and first.tolist() == [0, 3, 5] and tabs["ds_next"].tolist() == [1, 1, 1, 0, 0]
    with pytest.raises(ValueError):
        mpmpc.concat_routes([])


def test_route_argument_checks_without_a_device(built_library):
    """mpmpc_check_routes - the checks mpmpc_set_routes runs on its arguments - through the C ABI; the library loads without a
    GPU.  (The checks that depend on a handle's state - routes before a path, a B mismatch, a local wp_id beyond its route, set_path
    clearing the routes, P = 0: test_route_state_checks_without_a_device on the state object the handle owns, and
    test_route_argument_checks_on_a_handle through a handle, which mpmpc_create only makes on a device.)"""
    lib = mpmpc.load_library()
    good, circ = np.array([0, 200, 320, 420, 440], np.int32), np.array([1, 0, 0, 1], np.int32)
    assert lib.mpmpc_check_routes(440, 4, _i(good), _i(circ)) == 0
    for first, n_wp, why in (([1, 200, 320, 420, 440], 440, "first[0] must be 0"), ([0, 200, 200, 420, 440], 440, "strictly increasing"),
                             ([0, 200, 150, 420, 440], 440, "strictly increasing"), ([0, 200, 320, 420, 440], 441, "first[P]"),
                             ([0, 200, 320, 420, 439], 440, "first[P]"), ([0, 1, 320, 420, 440], 440, "at least 2 waypoints")):
        f = np.array(first, np.int32)
        assert lib.mpmpc_check_routes(n_wp, 4, _i(f), _i(circ)) == E_ARG, first
        assert why in lib.mpmpc_last_error().decode(), (first, lib.mpmpc_last_error())
    assert lib.mpmpc_check_routes(440, 0, _i(good), _i(circ)) == E_ARG
    assert lib.mpmpc_check_routes(440, 4, None, _i(circ)) == E_ARG and lib.mpmpc_check_routes(440, 4, _i(good), None) == E_ARG
    assert lib.mpmpc_set_routes(None, 4, _i(good), _i(circ)) == E_ARG and lib.mpmpc_set_car_routes(None, 1, _i(circ)) == E_ARG
    with pytest.raises(mpmpc.MpmpcError):
        mpmpc.check_routes(440, [0, 200, 100, 440], [1, 1, 1])
    mpmpc.check_routes(440, good, circ)


def test_route_state_checks_without_a_device(twin, track):
    """The handle's route state (csrc/route_state.hpp, the object the handle owns and every entry point asks) driven without a
    handle: routes before a path, first[0] != 0, non-increasing first, first[P] != n_wp, a route id out of range, a B mismatch,
    a local wp_id >= n of its route, set_path clearing the routes, P = 0 restoring single-path mode - the codes and messages the
    library returns (test_route_argument_checks_on_a_handle sees the same through a handle on the device)."""
    N = 30
    R = Routes(track, ["L", "A", "Bo", "S"])
    t = twin.routes_state_new(N, 1, 8)
    ch = np.zeros(1, np.int32)
    hdr = np.zeros(16, np.int32)

    def routes(first, circ=R.circular):
        f, c = np.ascontiguousarray(first, np.int32), np.ascontiguousarray(circ, np.int32)
        return twin.routes_state_set_routes(t, c.size, _i(f) if c.size else None, _i(c) if c.size else None, _i(ch))

    def deal(route):
        r = np.ascontiguousarray(route, np.int32)
        return twin.routes_state_set_car_routes(t, r.size, _i(r), _i(hdr))

    def upload(wp):
        w = np.ascontiguousarray(wp, np.int32)
        return twin.routes_state_check_upload(t, w.size, _i(w))
    try:
        assert routes(R.first) == E_STATE and b"no path set" in twin.routes_state_why(t)              # routes before a path
        assert deal([0, 0, 0, 0]) == E_STATE
        twin.routes_state_set_path(t, 440)
        assert upload([439, 5, 60, 3]) == 0                                                            # one path: global ids
        for first, why in (([1, 200, 320, 420, 440], b"first[0]"), ([0, 200, 200, 420, 440], b"strictly increasing"),
                           ([0, 200, 150, 420, 440], b"strictly increasing"), ([0, 200, 320, 420, 441], b"first[P]")):
            assert routes(first) == E_ARG and why in twin.routes_state_why(t) and ch[0] == 0, first
        assert upload([439, 5, 60, 3]) == 0                                                            # a refused call changed nothing
        assert routes(R.first) == 0 and ch[0] == 1
        assert upload([0, 5, 60, 3]) == E_STATE and b"mpmpc_set_car_routes" in twin.routes_state_why(t)      # no car routes yet
        for bad in ([0, 1, 2, 4], [0, -1, 2, 3]):
            assert deal(bad) == E_ARG and b"route id out of range" in twin.routes_state_why(t), bad
        assert deal(np.zeros(9, np.int32)) == E_ARG                                                    # B above max_batch
        assert deal([0, 1, 2, 3]) == 0
        assert hdr[:8].tolist() == [0, 200, 200, -120, 320, -100, 420, 20]                             # {first, n, negated when open}
        assert upload([0, 5, 60, 3]) == 0 and upload([199, 89, 69, 19]) == 0
        assert upload([0, 5, 60]) == E_STATE and twin.routes_state_check_batch(t, 3) == E_STATE        # B mismatch
        for bad, why in (([0, 5, 60, 20], b"wp_id out of range"), ([200, 5, 60, 3], b"wp_id out of range"),
                         ([0, 120, 60, 3], b"wp_id out of range"), ([0, 5, 60, -1], b"wp_id out of range"),
                         ([0, 90, 60, 3], b"Reached end of path!"), ([0, 5, 70, 3], b"Reached end of path!")):
            assert upload(bad) == E_ARG and why in twin.routes_state_why(t), bad
        assert deal([3, 1, 2, 0]) == 0 and upload([199, 89, 69, 19]) == E_ARG                          # re-dealt: 199 is not on S
        twin.routes_state_set_path(t, 440)                                                             # a new path clears the routes
        assert deal([0, 1, 2, 3]) == E_STATE and upload([439, 5, 60, 3]) == 0 and twin.routes_state_check_batch(t, 7) == 0
        assert routes(R.first) == 0 and deal([0, 1, 2, 3]) == 0 and upload([439, 5, 60, 3]) == E_ARG
        assert routes([], []) == 0 and ch[0] == 1                                                      # P = 0: one path again
        assert upload([439, 5, 60, 3]) == 0 and deal([0, 1, 2, 3]) == E_STATE
        assert routes([], []) == 0 and ch[0] == 0                                                      # ... and nothing changes twice
    finally:
        twin.routes_state_free(t)


# ------------------------------------------------------------------------------------------------------------ GPU
def _fleet_handle(R, N, B, **kw):
    h = mpmpc.Handle(T.stock_config(N, max_batch=B, **kw), mpmpc.default_settings())
    h.set_path(R.all["kappa"], R.all["v_ref"], R.all["ds_next"])
    h.set_corridor(R.all["ub"], R.all["lb"])
    h.set_routes(R.first, R.circular)
    return h


def _solo_handle(R, p, N, B):
    h = mpmpc.Handle(T.stock_config(N, max_batch=B, circular=bool(R.circular[p])), mpmpc.default_settings())
    o = R.own[p]
    h.set_path(o["kappa"], o["v_ref"], o["ds_next"])
    h.set_corridor(o["ub"], o["lb"])
    return h


def _rc(h, name, *args):
    return getattr(h.lib, name)(h._h, *args)


@pytest.mark.gpu
def test_route_argument_checks_on_a_handle(track):
    N = 30
    R = Routes(track, ["L", "A", "Bo", "S"])
    h = mpmpc.Handle(T.stock_config(N, max_batch=8), mpmpc.default_settings())
    try:
        assert _rc(h, "mpmpc_set_routes", R.P, _i(R.first), _i(R.circular)) == E_STATE            # routes before a path
        assert _rc(h, "mpmpc_set_car_routes", 4, _i(np.zeros(4, np.int32))) == E_STATE
        h.set_path(R.all["kappa"], R.all["v_ref"], R.all["ds_next"])
        h.set_corridor(R.all["ub"], R.all["lb"])
        for first in ([1, 200, 320, 420, 440], [0, 200, 200, 420, 440], [0, 200, 320, 420, 441]):
            assert _rc(h, "mpmpc_set_routes", R.P, _i(np.array(first, np.int32)), _i(R.circular)) == E_ARG, first
        wp, (x0, cc) = np.array([0, 5, 60, 3], np.int32), cars(4, N, 1, track)
        single = h.assemble(wp, x0, cc)                                                             # one path: global ids
        h.set_routes(R.first, R.circular)
        assert _rc(h, "mpmpc_upload", 4, _i(wp), _d(x0), _d(cc), None, None) == E_STATE             # no car routes yet
        for bad in ([0, 1, 2, 4], [0, -1, 2, 3]):
            assert _rc(h, "mpmpc_set_car_routes", 4, _i(np.array(bad, np.int32))) == E_ARG, bad     # route id out of range
        h.set_car_routes([0, 1, 2, 3])
        h.assemble(wp, x0, cc)
        assert _rc(h, "mpmpc_upload", 3, _i(wp), _d(x0), _d(cc), None, None) == E_STATE             # B differs from the car routes'
        assert _rc(h, "mpmpc_solve_resident", 3) == E_STATE
        for bad, why in (([0, 5, 60, 20], "wp_id out of range"), ([200, 5, 60, 3], "wp_id out of range"), ([0, 120, 60, 3], "wp_id out of range"),
                         ([0, 90, 60, 3], "Reached end of path!"), ([0, 5, 70, 3], "Reached end of path!"), ([0, 5, 60, -1], "wp_id out of range")):
            assert _rc(h, "mpmpc_upload", 4, _i(np.array(bad, np.int32)), _d(x0), _d(cc), None, None) == E_ARG, bad
            assert why in h.lib.mpmpc_last_error().decode(), bad
        h.assemble(np.array([199, 89, 69, 19], np.int32), x0, cc)                                   # the last valid local id of every route
        # a resident batch was checked against the routes its cars had: re-dealing the cars, or new routes, asks for a new upload
        # (wp 199 is fine on L and far outside S: its corridor row would be read out of bounds)
        last = np.array([199, 89, 69, 19], np.int32)
        h.upload(last, x0, cc)
        h.solve_resident(4)
        h.sync()
        h.set_car_routes([3, 1, 2, 0])
        assert _rc(h, "mpmpc_solve_resident", 4) == E_STATE and "uploaded" in h.lib.mpmpc_last_error().decode()
        assert _rc(h, "mpmpc_upload", 4, _i(last), _d(x0), _d(cc), None, None) == E_ARG
        h.set_car_routes([0, 1, 2, 3])
        h.upload(last, x0, cc)
        h.set_routes(R.first, R.circular)
        assert _rc(h, "mpmpc_set_car_routes", 4, _i(np.array([0, 1, 2, 3], np.int32))) == 0
        assert _rc(h, "mpmpc_solve_resident", 4) == E_STATE and "uploaded" in h.lib.mpmpc_last_error().decode()
        # the closed loop takes the cars' routes too: another number of cars than they were given for is refused
        h.set_path_geometry(R.all["x"], R.all["y"], R.all["psi"], np.zeros((440, 2)), np.zeros((440, 2)))
        cum = np.ascontiguousarray(R.all["cum_lengths"])
        s, pose = np.zeros(3), np.zeros((3, 3))
        assert _rc(h, "mpmpc_rollout_init", 3, C.c_double(0.05), _d(cum), _d(s), _d(pose), None) == E_STATE
        assert "mpmpc_set_car_routes" in h.lib.mpmpc_last_error().decode()
        assert _rc(h, "mpmpc_rollout_step", 3, 1) == E_STATE
        # a new path clears the routes; P = 0 does too
        h.set_path(R.all["kappa"], R.all["v_ref"], R.all["ds_next"])
        assert _rc(h, "mpmpc_set_car_routes", 4, _i(np.zeros(4, np.int32))) == E_STATE
        assert np.array_equal(h.assemble(wp, x0, cc), single)
        h.set_routes(R.first, R.circular)
        h.set_car_routes([0, 0, 0, 0])
        assert np.array_equal(h.assemble(wp, x0, cc), single)                                       # route 0 starts at row 0: same rows
        h.set_routes([], [])
        assert np.array_equal(h.assemble(wp, x0, cc), single)
        assert np.array_equal(h.assemble(np.array([439, 5, 60, 3], np.int32), x0, cc)[:, 1:], single[:, 1:])      # global ids again
    finally:
        h.close()


def _fleet(R, B, N, seed):
    """B cars dealt route = i % P; local waypoints cover wp 0, 1, n-N-1, n-N, n-2, n-1 of every route as far as an upload takes
    them (an open route ends at wp + N >= n), the rest drawn from the valid range"""
    rng = np.random.default_rng(seed)
    route = (np.arange(B) % R.P).astype(np.int32)
    wp = np.zeros(B, np.int32)
    for p in range(R.P):
        idx = np.flatnonzero(route == p)
        n = int(R.n[p])
        top = n - 1 if R.circular[p] else n - N - 1
        edges = [w for w in edge_waypoints(n, N) if w <= top]
        w = rng.integers(0, top + 1, idx.size)
        w[:len(edges)] = edges
        wp[idx] = w
    return route, wp


@pytest.mark.gpu
@pytest.mark.parametrize("B,packing", [(192, 0), (192, 32), (2048, 0)])
def test_assemble_and_solve_against_solo_handles(B, packing, track):
    """Oracle A on L+A+Bo+S at N = 30, cars interleaved route = i % 4: B = 2 048 packs two instances per wavefront on its own,
    B = 192 with 32 lanes per instance forces it - neighbours in a wave are on different routes."""
    N = 30
    R = Routes(track, ["L", "A", "Bo", "S"])
    route, wp = _fleet(R, B, N, 5)
    x0, cc = cars(B, N, 6, track)
    h = _fleet_handle(R, N, B, circular=False)          # (the handle-wide flag is ignored while routes are set)
    try:
        h.set_packing(packing)
        h.set_car_routes(route)
        qp = h.assemble(wp, x0, cc)
        sol = h.solve(wp, x0, cc)
        h.upload(wp, x0, cc)
        h.solve_resident(B)
        res = h.download(B)
    finally:
        h.close()
    assert np.array_equal(res.status, sol.status) and np.array_equal(res.iters, sol.iters) and np.array_equal(res.z, sol.z)
    assert (sol.status == 1).mean() > 0.9
    for p in range(R.P):
        idx = np.flatnonzero(route == p)
        s = _solo_handle(R, p, N, idx.size)
        try:
            qp1 = s.assemble(wp[idx], x0[idx], cc[idx])
            sol1 = s.solve(wp[idx], x0[idx], cc[idx])
        finally:
            s.close()
        assert np.array_equal(qp[:, idx, :], qp1), R.names[p]
        assert np.array_equal(sol.status[idx], sol1.status) and np.array_equal(sol.iters[idx], sol1.iters), R.names[p]
        du, dz = np.abs(sol.u0[idx] - sol1.u0).max(), np.abs(sol.z[idx] - sol1.z).max()
        print("route %s: %d cars, max |du0| = %.3g, max |dz| = %.3g" % (R.names[p], idx.size, du, dz))
        # (the project's bound for a solve in another place of another wave is 1e-9; measured here: bit-equal at all three
        #  shapes - the fields are bit-equal and none of these instances met a wave-mate through a reduction that rounds)
        assert np.array_equal(sol.u0[idx], sol1.u0) and np.array_equal(sol.z[idx], sol1.z), R.names[p]


@pytest.mark.gpu
@pytest.mark.parametrize("copies", [3, 6])
def test_copies_of_one_path_equal_the_single_path_handle(copies, track):
    """Oracle B: copies of L concatenated, cars dealt round-robin, against the whole fleet on a single-path handle - the same
    launch, the same place of every car in its wave: bit-equal.  3 copies = 600 rows: K1 stages the concatenated table in LDS;
    6 copies = 1 200 rows, above K1_LDS_WP = 1 024: K1 gathers from memory."""
    N, B = 30, 1536
    R = Routes(track, ["L"] * copies)
    sc = scenarios.make(2, track, B=B)
    route = (np.arange(B) % copies).astype(np.int32)
    h = _fleet_handle(R, N, B)
    s = _solo_handle(R, 0, N, B)
    try:
        h.set_car_routes(route)
        qp, sol = h.assemble(sc.wp_id, sc.x0, sc.cc_prev), h.solve(sc.wp_id, sc.x0, sc.cc_prev)
        qp1, sol1 = s.assemble(sc.wp_id, sc.x0, sc.cc_prev), s.solve(sc.wp_id, sc.x0, sc.cc_prev)
    finally:
        h.close()
        s.close()
    assert np.array_equal(qp, qp1)
    for k in ("status", "iters", "u0", "z"):
        assert np.array_equal(getattr(sol, k), getattr(sol1, k)), k


@pytest.mark.gpu
def test_build_corridor_with_routes_against_solo_builds():
    """mpmpc_build_corridor on the concatenated geometry of L+A+Bo (Sim_Track grid with obstacles, 30 columns) against three
    solo builds: array_equal, NaN rows and their count included; the handle then assembles from the rows of the car's route."""
    N = 30
    g1, grid, sm = _g1_world()
    names = ["L", "A", "Bo"]
    own = _geometry(g1, names)
    cat, first = mpmpc.concat_routes(own)
    circ = np.array([SPANS[k][2] for k in names], np.int32)
    v = np.full(int(first[-1]), 0.8)

    def build(tab, circular, routes):
        h = mpmpc.Handle(T.stock_config(N, max_batch=4, circular=circular), mpmpc.default_settings())
        try:
            h.set_path(tab["kappa"], v[:tab["kappa"].size], tab["ds_next"])
            if routes:
                h.set_routes(first, circ)
            h.set_map(grid, (-1.0, -2.0), 0.005)
            h.set_path_geometry(tab["x"], tab["y"], tab["psi"], tab["border_ub"], tab["border_lb"])
            out = h.build_corridor(N, 2 * sm, sm)
            # a built table is void once the routes change (its horizons were walked under the old ones): the solve asks for one
            if routes:
                wp, x0, cc = np.zeros(4, np.int32), np.zeros((4, 3)), np.zeros((4, 2 * N))
                h.set_car_routes([0, 1, 2, 0])
                h.assemble(wp, x0, cc)
                h.set_map(grid, (-1.0, -2.0), 0.005)          # (a new map generation in between does not keep the table alive)
                h.set_routes([], [])
                assert _rc(h, "mpmpc_upload", 4, _i(wp), _d(x0), _d(cc), None, None) == E_STATE
                assert "corridor table" in h.lib.mpmpc_last_error().decode()
            return out
        finally:
            h.close()
    ub, lb, bad = build(cat, False, True)
    bad_solo = 0
    for p, o in enumerate(own):
        u1, l1, b1 = build(o, bool(circ[p]), False)
        f = int(first[p])
        assert np.array_equal(ub[f:f + u1.shape[0]], u1, equal_nan=True) and np.array_equal(lb[f:f + u1.shape[0]], l1, equal_nan=True), names[p]
        bad_solo += b1
    assert bad == bad_solo


# ---- the closed loop.  Integers (wp_id, status, alive, counter, audit steps) equal; s, pose, u, x0, plans, predicted paths,
# corridor rows and clearances to 1e-8, the device-against-host rollout bound of DESIGN (K3) - a fleet's solves may sit in other
# waves than the solo handle's.  Entries a step did not produce are NaN in both.
INT_KEYS = ("wp_id", "status", "alive", "counter", "contact_steps", "first_contact", "min_step", "last_contact", "disc_first", "disc_last",
            "wall_first", "wall_last", "disc_known", "wall_known")


def _same(a, b, where):
    for k in a:
        if isinstance(a[k], dict):
            _same(a[k], b[k], "%s %s" % (where, k))
        elif a[k] is None:
            assert b[k] is None, (where, k)
        elif k in INT_KEYS:
            assert np.array_equal(a[k], b[k]), (where, k, np.flatnonzero(np.asarray(a[k]).ravel() != np.asarray(b[k]).ravel())[:8])
        else:
            x, y = np.asarray(a[k], float), np.asarray(b[k], float)
            assert np.array_equal(np.isnan(x), np.isnan(y)), (where, k)
            d = np.nanmax(np.abs(x - y)) if x.size and not np.isnan(x).all() else 0.0
            assert d <= 1e-8, (where, k, d)


def _cars_of(out, idx):
    """the cars idx of a rollout's result: state arrays are [B, ...], trace arrays [records, B, ...]"""
    return {k: (None if v is None else _cars_of(v, idx) if isinstance(v, dict) and k != "trace" else
                {f: t[:, idx] for f, t in v.items()} if k == "trace" else v[idx]) for k, v in out.items()}


def _same_rollout(fleet, solo, idx, where):
    _same(_cars_of(fleet, idx), solo, where)


def _route_tables(track, names, grid_name="free"):
    """geometry, path tables and re-based cum_lengths of the fixture routes, each route's own and concatenated"""
    g1, grid, sm = _g1_world(grid_name)
    own = _geometry(g1, names)
    cum = np.cumsum(track.segment_lengths)
    for k, o in zip(names, own):
        lo, hi, _ = SPANS[k]
        o["v_ref"] = track.v_ref[lo:hi].copy()
        o["cum_lengths"] = cum[lo:hi] - cum[lo]
    cat, first = mpmpc.concat_routes(own)
    return own, cat, first, np.array([SPANS[k][2] for k in names], np.int32), grid, sm


def _cells(xy):
    """map cells of world points on the Sim_Track grid (origin (-1, -2), 5 mm)"""
    xy = np.atleast_2d(np.asarray(xy, float))
    return np.stack([np.floor((xy[:, 0] + 1.0) / 0.005), np.floor((xy[:, 1] + 2.0) / 0.005)], 1).astype(np.int32)


def _run(tab, circular, routes, N, grid, sm, s, poses, steps, discs=None, walls=None, movers=None, traffic=None, perception=None,
         car_routes=None):
    """one recorded, audited rollout on a handle with the corridor built on the device -> state + audit (+ perception) + trace"""
    B = s.size
    h = mpmpc.Handle(T.stock_config(N, max_batch=B, circular=circular), mpmpc.default_settings())
    try:
        h.set_path(tab["kappa"], tab["v_ref"], tab["ds_next"])
        if routes is not None:
            h.set_routes(*routes)
        h.set_map(grid, (-1.0, -2.0), 0.005)
        h.set_path_geometry(tab["x"], tab["y"], tab["psi"], tab["border_ub"], tab["border_lb"])
        assert h.build_corridor(N, 2 * sm, sm, want_tables=False)[2] == 0
        if car_routes is not None:
            h.set_car_routes(car_routes)
        if walls is not None:
            h.rollout_set_walls(walls)
        if discs is not None:
            h.rollout_set_obstacles(discs)
        if movers is not None:
            h.rollout_set_movers(movers)
        if traffic is not None:
            h.rollout_set_traffic(*traffic)
        h.rollout_set_audit(1, 0.12, 0.06, 0.1)
        if perception is not None:
            h.rollout_set_perception(*perception)
        h.rollout_record(steps, plan=True, prediction=True, rows=True, B=B)
        h.rollout_init(0.05, tab["cum_lengths"], s, poses)
        h.rollout_step(steps)
        out = h.rollout_state()
        out["audit"] = h.rollout_audit()
        if perception is not None:
            out["perception"] = h.rollout_perception()
        out["trace"] = h.rollout_trace()
        return out
    finally:
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("B,steps", [(96, 12), (1536, 4)])
def test_rollout_against_solo_rollouts(B, steps, track):
    """Oracle A in closed loop: cars on L+A+Bo (route = i % 3), everything recorded and audited, per-car discs on a third of the
    cars, some cars N + 3 waypoints before the end of an open route (alive = -2 fires after a few steps, per route), one car on
    L with s just short of the lap's length (alive = 0) - state, audit accumulators and the whole trace (predicted path and
    corridor rows included) against three solo rollouts.  1 536 cars: a packed closed-loop launch."""
    N = 30
    names = ["L", "A", "Bo"]
    own, cat, first, circ, grid, sm = _route_tables(track, names)
    rng = np.random.default_rng(60)
    route = (np.arange(B) % 3).astype(np.int32)
    n = np.diff(first)
    wp = np.array([rng.integers(0, n[p] - N - 3 if not circ[p] else n[p] - 1) for p in route], np.int32)
    for j, i in enumerate(np.flatnonzero(route != 0)[:8]):
        wp[i] = n[route[i]] - N - 3 + (j % 3)          # open routes: the end comes within the run, sooner or later
    s = np.array([own[p]["cum_lengths"][w] for p, w in zip(route, wp)])
    poses = np.array([[own[p]["x"][w], own[p]["y"][w], own[p]["psi"][w]] for p, w in zip(route, wp)])
    lap = int(np.flatnonzero(route == 0)[1])
    s[lap] = own[0]["cum_lengths"][-1] - 1e-4          # the lap ends with the first step
    poses[lap] = (own[0]["x"][-1], own[0]["y"][-1], own[0]["psi"][-1])
    discs = []
    for i in range(B):
        o, m = own[route[i]], int(n[route[i]])
        w = (wp[i] + 9) % m if circ[route[i]] else min(wp[i] + 9, m - 1)
        discs.append(np.concatenate([_cells(o["border_ub"][w]), [[3]]], 1) if i % 3 == 1 else np.zeros((0, 3), np.int32))
    fleet = _run(cat, False, (first, circ), N, grid, sm, s, poses, steps, discs=discs, car_routes=route)
    ended = np.argmax(fleet["trace"]["alive"] == -2, 0)[fleet["alive"] == -2]
    print("B = %d: alive %s, the open routes' ends came at steps %s" % (B, dict(zip(*np.unique(fleet["alive"], return_counts=True))), sorted(set(ended))))
    assert (fleet["alive"] == -2).any() and fleet["alive"][lap] == 0 and (fleet["alive"] == 1).sum() > B // 2
    assert fleet["trace"]["alive"].shape == (steps, B) and (steps < 12 or len(set(ended)) > 1)
    for p in range(3):
        idx = np.flatnonzero(route == p)
        solo = _run(own[p], bool(circ[p]), None, N, grid, sm, s[idx], poses[idx], steps, discs=[discs[i] for i in idx])
        _same_rollout(fleet, solo, idx, "%s, %d cars" % (names[p], B))


@pytest.mark.gpu
def test_rollout_of_copies_equals_the_single_path_rollout(track):
    """Oracle B in closed loop: 3 copies of L, 64 cars dealt round-robin, 10 steps, against the same fleet on a single-path
    handle - with traffic (ONE group spanning all copies: cars of different routes meet), per-car walls, one straight-line and
    one along-the-path mover per car (the latter follows its owner's route), the audit and perception, everything recorded."""
    N, B, steps = 30, 64, 10
    own, cat, first, circ, grid, sm = _route_tables(track, ["L", "L", "L"])
    L = own[0]
    route = (np.arange(B) % 3).astype(np.int32)
    wp = (np.arange(B) * 3 + 2) % 200          # cars a few waypoints apart: they see each other
    s = L["cum_lengths"][wp]
    poses = np.stack([L["x"][wp], L["y"][wp], L["psi"][wp]], 1)
    walls, movers = [], []
    for i in range(B):
        w = (wp[i] + 14) % 200
        a, c = _cells(L["border_ub"][w])[0], _cells([L["x"][w], L["y"][w]])[0]
        walls.append(np.array([[a[0], a[1], a[0] + (c[0] - a[0]) // 3, a[1] + (c[1] - a[1]) // 3]], np.int32) if i % 2 else np.zeros((0, 4), np.int32))
        w2 = (wp[i] + 20) % 200
        movers.append(np.array([[0, 2, L["border_lb"][w2][0], L["border_lb"][w2][1], 0.001, -0.001],
                                [1, 2, s[i] + 0.9, -0.08, 0.004, 0.0]]))
    traffic = (np.zeros(B, np.int32), np.full(B, 5, np.int32), 2, 120)
    perception = (np.linspace(-1.2, 1.2, 25), 1.0, 2)
    kw = dict(walls=walls, movers=movers, traffic=traffic, perception=perception)
    fleet = _run(cat, False, (first, circ), N, grid, sm, s, poses, steps, car_routes=route, **kw)
    single = _run(L, True, None, N, grid, sm, s, poses, steps, **kw)
    print("alive %s, cars that know a disc: %d" % (dict(zip(*np.unique(fleet["alive"], return_counts=True))),
                                                  int((fleet["perception"]["disc_known"] != 0).sum())))
    assert (fleet["alive"] == 1).sum() > B // 4
    _same(fleet, single, "3 copies of L")


@pytest.mark.gpu
def test_batch_mpc_with_routes_end_to_end():
    """Through Python: two routes built by ReferencePath.on_device on the Sim grid from different corner points (the lap,
    circular; its first corners, open), their speed profiles (K4), BatchMPC.set_routes with the corridor built on the device
    for both at once, one get_control_batch(routes=...) and rollout(routes=...) for 5 recorded steps - against two solo BatchMPC
    controllers, one per route."""
    import warnings
    from map import Map
    from MPC import BatchMPC
    from reference_path import ReferencePath
    from scipy import sparse
    from spatial_bicycle_models import BicycleModel
    g1 = np.load(os.path.join(T.GOLDEN, "g1_path_sim_track.npz"))
    g2 = np.load(os.path.join(T.GOLDEN, "g2_speed_profile.npz"))
    hh, ww = g1["grid_shape"]
    grid = np.unpackbits(g1["grid_free"])[:hh * ww].reshape(hh, ww).astype(np.int8)
    m = Map.from_grid(grid, origin=[-1, -2], resolution=0.005)
    cons = dict(zip(('a_min', 'a_max', 'v_min', 'v_max', 'ay_max'), g2["constraints"]))
    wx, wy = list(g1["wp_x"]), list(g1["wp_y"])
    paths = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for xs, ys, circ in ((wx, wy, True), (wx[:5], wy[:5], False)):
            rp = ReferencePath.on_device(m, xs, ys, 0.05, 5, 0.23, circ)
            rp.compute_speed_profile(cons)
            paths.append(rp)
    assert paths[0].n_waypoints == 200 and 40 < paths[1].n_waypoints < 200
    N, B = 30, 48
    Q, R, QN = sparse.diags([1.0, 0.0, 0.0]), sparse.diags([0.5, 0.0]), sparse.diags([1.0, 0.0, 0.0])
    ic = {'umin': np.array([0.0, -np.tan(0.66) / 0.12]), 'umax': np.array([1.0, np.tan(0.66) / 0.12])}
    sc = {'xmin': np.array([-np.inf] * 3), 'xmax': np.array([np.inf] * 3)}
    cars_ = [BicycleModel(reference_path=rp, length=0.12, width=0.06, Ts=0.05) for rp in paths]
    rng = np.random.default_rng(8)
    route = (np.arange(B) % 2).astype(np.int32)
    s = np.array([rng.uniform(0.0, 0.9 * paths[p].length if p == 0 else paths[p].length - (N + 3) * 0.06) for p in route])
    poses = np.zeros((B, 3))
    for i, p in enumerate(route):
        w = paths[p].waypoints[int(np.searchsorted(np.cumsum(paths[p].segment_lengths), s[i]))]
        poses[i] = (w.x - 0.01 * np.sin(w.psi), w.y + 0.01 * np.cos(w.psi), w.psi + 0.05)
    cc = np.zeros((B, 2 * N))
    fleet = BatchMPC(cars_[0], N, Q, R, QN, sc, ic, 4.0, max_batch=B, corridor="device")
    try:
        assert fleet.set_routes(paths) == 0
        wp, x0 = fleet.spatial_states(s, poses, routes=route)
        u, plan, status, sol = fleet.get_control_batch(wp, x0, cc, routes=route)
        ro = fleet.rollout(s, poses, 5, routes=route, record=dict(plan=True, prediction=True, rows=True))
        with pytest.raises(ValueError):
            fleet.rollout(s, poses, 1)          # routes are set: the rollout needs the cars' routes
        fleet.set_routes(None)          # back to the lap: global ids of route 0
        idx = np.flatnonzero(route == 0)
        back = fleet.get_control_batch(wp[idx], x0[idx], cc[idx])
    finally:
        fleet.close()
    assert (status == 1).all()
    for p in range(2):
        idx = np.flatnonzero(route == p)
        solo = BatchMPC(cars_[p], N, Q, R, QN, sc, ic, 4.0, max_batch=idx.size, corridor="device")
        try:
            wp1, x01 = solo.spatial_states(s[idx], poses[idx])
            u1, plan1, status1, sol1 = solo.get_control_batch(wp1, x01, cc[idx])
            ro1 = solo.rollout(s[idx], poses[idx], 5, record=dict(plan=True, prediction=True, rows=True))
        finally:
            solo.close()
        assert np.array_equal(wp1, wp[idx]) and np.array_equal(x01, x0[idx])
        assert np.array_equal(status1, status[idx]) and np.array_equal(sol1.iters, sol.iters[idx])
        assert np.abs(u1 - u[idx]).max() <= 1e-9 and np.abs(sol1.z - sol.z[idx]).max() <= 1e-9
        _same_rollout(ro, ro1, idx, "route %d" % p)
        if p == 0:
            assert np.array_equal(back[2], status1) and np.abs(back[0] - u1).max() <= 1e-9
