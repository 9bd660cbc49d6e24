"""Real_Track (src/simulation.py:57-88 of the reference): the second scenario the reference ships, and the only one with
an OPEN path.  302 waypoints over 59.5 m on a non-square 767 x 867 grid at 0.06 m/px, a 0.30 x 0.20 m car, corridors up
to 1.50 m wide.  Goldens G1r-G6r (tests/golden/make_golden.py real, make_g5.py) were produced by the reference itself.

At the end of an open path the reference's get_waypoint prints "Reached end of path!" and calls exit(1) as soon as a
horizon would read waypoint wp_id + N >= n_wp (src/reference_path.py:359-369, from src/MPC.py:93-94).  The product mirrors
that in three places, pinned here: MPC.get_control raises SystemExit(1), the batch solve refuses the call
(MPMPC_E_ARG, "Reached end of path!"), and the K3 rollout ends such a car with alive = -2.

The CPU tests run the host classes, the oracle and the CPU emulation of the kernels; the -m gpu tests run libmpmpc.so."""
import ctypes as C
import os

import numpy as np
import pytest
from scipy import sparse

import mpc_np as M
import mpmpc
import mpmpc_testlib as T
import osqp_np as O
import scenarios

G = M.GOLDEN
N_WP = 302
_d = T._d


def _load(name):
    return np.load(os.path.join(G, name))


def _grid(g1, key):
    h, w = g1["grid_shape"]
    return np.ascontiguousarray(np.unpackbits(g1[key])[:h * w].reshape(h, w).astype(np.int8))


@pytest.fixture(scope="module")
def g1():
    return _load("g1_path_real_track.npz")


@pytest.fixture(scope="module")
def g3():
    return _load("g3_corridor_real.npz")


@pytest.fixture(scope="module")
def rtrack():
    return scenarios.real_track()


@pytest.fixture(scope="module")
def ortrack(g1):
    g2 = _load("g2_speed_profile_real.npz")
    return M.Track(g1["x"], g1["y"], g1["psi"], g1["kappa"], g1["ds_next"], g1["segment_lengths"], g2["v_ref"],
                   float(g1["length"][0]), False)


def _g4(N):
    return _load("g4_assembly_real_N%d.npz" % N), _load("g5_solutions_real_N%d.npz" % N)


def _dense_A(g4, c, N):
    n, m = 5 * N + 3, 8 * N + 6
    lo, hi = g4["A_case_ptr"][c], g4["A_case_ptr"][c + 1]
    return sparse.csc_matrix((g4["A_data"][lo:hi], g4["A_indices"][lo:hi], g4["A_indptr"][c]), shape=(m, n)).toarray()


def _weights(g4):
    return M.Weights.time_optimal() if str(g4["weights"][0]) == "time_optimal" else M.Weights.stock()


def _real_world(obstacles=False):
    """Real_Track with our host classes from the golden tables (as tests/mpmpc_testlib.py:build_world does for Sim_Track)."""
    from map import Map
    from reference_path import ReferencePath
    from spatial_bicycle_models import BicycleModel
    g1 = _load("g1_path_real_track.npz")
    g2 = _load("g2_speed_profile_real.npz")
    m = Map.from_grid(_grid(g1, "grid_obstacles" if obstacles else "grid_free"), origin=list(g1["origin"]),
                      resolution=float(g1["resolution"][0]))
    rp = ReferencePath.from_tables(m, g1["x"], g1["y"], g1["psi"], g1["kappa"], circular=False, v_ref=g2["v_ref"],
                                   border_ub=g1["border_ub"], border_lb=g1["border_lb"],
                                   ub_static=g1["ub_static"], lb_static=g1["lb_static"])
    car = BicycleModel(reference_path=rp, length=float(g1["car"][0]), width=float(g1["car"][1]), Ts=float(g1["car"][2]))
    return m, rp, car


def _make_mpc(car, N, rtrack, backend=None, corridor="host", settings=None):
    from MPC import MPC
    Q, R, QN = sparse.diags([1.0, 0.0, 0.0]), sparse.diags([0.5, 0.0]), sparse.diags([1.0, 0.0, 0.0])
    ic = {'umin': np.array([0.0, -np.tan(0.66) / car.length]), 'umax': np.array([1.0, np.tan(0.66) / car.length])}
    sc = {'xmin': np.array([-np.inf] * 3), 'xmax': np.array([np.inf] * 3)}
    if backend == "emu":
        backend = T.EmuBackend(T.stock_config(N, track=rtrack), settings or mpmpc.default_settings())
    return MPC(car, N, Q, R, QN, sc, ic, 4.0, settings=settings, backend=backend, corridor=corridor)


# ======================================================================================================== fixtures
def test_fixtures_are_the_open_real_track(g1, g3, rtrack):
    assert tuple(g1["grid_shape"]) == (767, 867) and g1["x"].size == N_WP and not bool(g1["circular"][0])
    ds = g1["ds_next"][:-1]
    assert 0.14 < ds.min() and ds.max() < 0.21 and g1["ds_next"][-1] == 0.0 and 59.5 < g1["length"][0] < 59.6
    assert rtrack.car_length == 0.30 and rtrack.car_width == 0.20 and not rtrack.circular
    assert np.array_equal(rtrack.umax, [1.0, np.tan(0.66) / 0.30]) and np.array_equal(rtrack.umin, -rtrack.umax * [0, 1])
    # the corridor prefix the reference can build: full up to row n_wp - 51, then one column less per row
    for key in ("free", "obstacles"):
        v = g3["valid_cols_" + key]
        assert np.array_equal(v, np.minimum(50, N_WP - 1 - np.arange(N_WP)))
        cols = np.arange(50)[None, :]
        assert np.all(np.isfinite(g3["ub_" + key][cols < v[:, None]])) and np.all(np.isnan(g3["ub_" + key][cols >= v[:, None]]))
    g6 = _load("g6_closed_loop_real_N30.npz")
    assert bool(g6["exited_end_of_path"][0]) and int(g6["exit_wp_id"][0]) + 30 >= N_WP > int(g6["wp_id"][-1]) + 30
    for N in (10, 30, 50):
        g4, _ = _g4(N)
        last = N_WP - N - 1
        assert 0 in g4["wp_id"] and g4["wp_id"].max() == last and set(range(last - 4, last + 1)) <= set(g4["wp_id"])
        assert g4["obst"].sum() * 2 == g4["obst"].size


# ======================================================================================================== host classes
def test_host_grids_match_reference_on_the_non_square_map(g1):
    from map import Map, Obstacle, fill_small_holes
    thr = _grid(g1, "grid_thresholded").astype(bool)
    assert np.array_equal(fill_small_holes(thr, 5).astype(np.int8), _grid(g1, "grid_free"))
    m = Map.from_grid(_grid(g1, "grid_free"), origin=list(g1["origin"]), resolution=float(g1["resolution"][0]))
    assert (m.height, m.width) == (767, 867)
    m.add_obstacles([Obstacle(cx=c[0], cy=c[1], radius=c[2]) for c in g1["obstacles"]])
    assert np.array_equal(m.data, _grid(g1, "grid_obstacles"))


def test_host_path_construction_matches_reference(g1):
    from map import Map
    from reference_path import ReferencePath
    m = Map.from_grid(_grid(g1, "grid_free"), origin=list(g1["origin"]), resolution=float(g1["resolution"][0]))
    rp = ReferencePath(m, list(g1["wp_x"]), list(g1["wp_y"]), 0.20, smoothing_distance=5, max_width=1.50, circular=False)
    wps = rp.waypoints
    assert rp.n_waypoints == N_WP
    for key, got in (("x", [w.x for w in wps]), ("y", [w.y for w in wps]), ("segment_lengths", rp.segment_lengths),
                     ("ub_static", [w.ub for w in wps]), ("lb_static", [w.lb for w in wps]),
                     ("border_ub", [w.static_border_cells[0] for w in wps]),
                     ("border_lb", [w.static_border_cells[1] for w in wps])):
        assert np.array_equal(np.array(got, float), g1[key]), key
    # psi through arctan2, kappa from psi: a few ulp between numpy versions
    assert np.max(np.abs(np.array([w.psi for w in wps]) - g1["psi"])) <= 1e-14
    assert np.max(np.abs(np.array([float(w.kappa) for w in wps]) - g1["kappa"])) <= 1e-14
    assert bool(g1["kappa0_is_int"][0]) and isinstance(wps[0].kappa, int)
    assert rp.length == g1["length"][0]
    kappa, v_ref, ds = rp.tables()
    assert np.array_equal(ds, g1["ds_next"])
    with pytest.raises(SystemExit):
        rp.get_waypoint(N_WP)


def test_host_speed_profile_matches_reference(g1):
    m, rp, car = _real_world()
    g2 = _load("g2_speed_profile_real.npz")
    cons = dict(zip(('a_min', 'a_max', 'v_min', 'v_max', 'ay_max'), g2["constraints"]))
    P, q, A, l, u = rp.speed_profile_qp(cons)
    Aref = sparse.coo_matrix((g2["A_val"], (g2["A_row"], g2["A_col"])), shape=tuple(g2["A_shape"])).toarray()
    assert A.shape == (2 * 301 - 1, 301)
    assert np.allclose(A, Aref, rtol=0, atol=1e-12) and np.allclose(q, g2["q"], atol=1e-14)
    assert np.allclose(l, g2["l"]) and np.allclose(u, g2["u"], atol=1e-14)
    rp.compute_speed_profile(cons, solver=T.emu_speed_profile)
    v = np.array([w.v_ref for w in rp.waypoints])
    assert np.max(np.abs(v - g2["v_ref"])) <= 1e-9 and v[-1] == v[-2]


@pytest.mark.parametrize("key", ["free", "obstacles"])
def test_host_corridor_matches_reference_up_to_the_end_of_the_path(key, g3):
    m, rp, car = _real_world(key == "obstacles")
    sm = float(g3["safety_margin"][0])
    assert sm == car.safety_margin
    v = g3["valid_cols_" + key]
    for w in range(0, N_WP - 1, 3):
        ub, lb, _ = rp.update_path_constraints(w + 1, int(v[w]), 2 * sm, sm)
        assert np.array_equal(ub, g3["ub_" + key][w, :v[w]]) and np.array_equal(lb, g3["lb_" + key][w, :v[w]]), w
        if v[w] < 50:          # one column more reads waypoint n_wp: the reference exits there, and so does the host
            with pytest.raises(SystemExit):
                rp.update_path_constraints(w + 1, int(v[w]) + 1, 2 * sm, sm)


# ======================================================================================================== oracle
@pytest.mark.parametrize("N", [10, 30, 50])
def test_oracle_assembly_matches_reference_capture(N, ortrack):
    g4, _ = _g4(N)
    w, lim = _weights(g4), M.Limits.stock(0.30)
    for c in range(g4["s"].size):
        wp = int(g4["wp_id"][c])
        assert M.current_waypoint(ortrack.segment_lengths, g4["s"][c]) == wp
        x0 = np.array(M.t2s(*g4["pose"][c], ortrack.x[wp], ortrack.y[wp], ortrack.psi[wp]))
        assert np.array_equal(x0, g4["x0"][c])
        P, q, A, l, u = M.assemble(ortrack, wp, g4["x0"][c], g4["cc_prev"][c], g4["lb"][c], g4["ub"][c], N, w, lim)
        Aref = _dense_A(g4, c, N)
        assert np.array_equal(A, Aref) and sparse.csc_matrix(A).nnz == np.diff(g4["A_case_ptr"])[c]
        assert np.array_equal(np.diag(P), g4["P_diag"][c]) and np.count_nonzero(P) == np.count_nonzero(np.diag(P))
        assert np.array_equal(q, g4["q"][c]) and np.array_equal(np.signbit(q), np.signbit(g4["q"][c]))
        assert np.array_equal(l, g4["l"][c])
        # u: bit exact but for the speed-cap entries (libm tan across numpy versions: a few ulp)
        fin = np.isfinite(u)
        assert np.array_equal(u[~fin], g4["u"][c][~fin])
        assert np.all(np.abs(u[fin] - g4["u"][c][fin]) <= 4 * np.spacing(np.abs(u[fin])))
        cap = np.flatnonzero(u != g4["u"][c])
        assert all((i >= 6 * (N + 1)) and ((i - 6 * (N + 1)) % 2 == 0) for i in cap)


@pytest.mark.parametrize("N", [10, 30, 50])
def test_g5r_solutions_are_certified(N):
    g4, g5 = _g4(N)
    assert set(np.unique(g5["status"])) <= {1, -3} and np.sum(g5["status"] == 1) >= 60
    for c in range(g4["s"].size):
        A = _dense_A(g4, c, N)
        if g5["status"][c] == 1:
            k = O.kkt_certificate(np.diag(g4["P_diag"][c]), g4["q"][c], A, g4["l"][c], g4["u"][c], g5["x"][c], g5["y"][c])
            assert k["ok_tol"](1e-8), (N, c, k["prim"], k["stat"], k["comp"])
            assert abs(k["obj"] - g5["obj"][c]) <= 1e-12 * max(1.0, abs(k["obj"]))
            if np.isfinite(g5["obj_highs"][c]):
                assert abs(k["obj"] - g5["obj_highs"][c]) <= 2e-5 * max(1.0, abs(k["obj"]))
        else:
            f = O.farkas_certificate(A, g4["l"][c], g4["u"][c], g5["y"][c], 1e-6)
            assert f["ok"], (N, c)


def test_g5r_has_an_infeasible_capture():
    assert sum(int(np.sum(_g4(N)[1]["status"] == -3)) for N in (10, 30, 50)) >= 1


# ======================================================================================================== emulation
_EMU_GROUPS = {10: (64, 32, 16), 30: (64, 32), 50: (64,)}


@pytest.mark.parametrize("N", [10, 30, 50])
def test_emulated_kernels_on_the_reference_captures(N, emu, rtrack):
    g4, g5 = _g4(N)
    cfg = T.stock_config(N, str(g4["weights"][0]), track=rtrack)
    assert cfg.circular == 0 and cfg.wheelbase == 0.30
    inputs = (g4["wp_id"].astype(np.int32), g4["x0"], g4["cc_prev"], g4["lb"], g4["ub"])
    qp = emu.assemble(cfg, rtrack, inputs)
    for c in range(g4["s"].size):                                   # K1: bit exact (speed cap: libm tan, a few ulp)
        Pd, q, A, l, u = T.qp_to_dense(qp[:, c, :], N)
        assert np.array_equal(q, g4["q"][c]) and np.array_equal(l, g4["l"][c]) and np.array_equal(Pd, g4["P_diag"][c])
        assert np.array_equal(A, _dense_A(g4, c, N))
        fin = np.isfinite(g4["u"][c])
        assert np.array_equal(u[~fin], g4["u"][c][~fin])
        assert np.max(np.abs(u[fin] - g4["u"][c][fin])) <= 4 * np.finfo(float).eps
    ok = g5["status"] == 1
    for Gs in _EMU_GROUPS[N]:
        sol = emu.solve(cfg, mpmpc.default_settings(), qp, G=Gs)
        assert np.array_equal(sol.status, g5["status"]), Gs
        assert np.max(np.abs(sol.z[ok] - g5["x"][ok])) <= 1e-6, Gs
        assert np.max(np.abs(sol.z[ok][:, -2 * N:-2 * N + 2] - g5["x"][ok][:, -2 * N:-2 * N + 2])) <= 1e-8, Gs


def test_emulation_handle_refuses_the_end_of_the_path(rtrack):
    N = 30
    h = T.EmuBackend(T.stock_config(N, track=rtrack), mpmpc.default_settings())
    h.set_path(rtrack.kappa, rtrack.v_ref, rtrack.ds_next)
    last = N_WP - N - 1
    lb, ub = rtrack.lb_free[[last], :N], rtrack.ub_free[[last], :N]
    assert h.solve(np.array([last], np.int32), np.zeros((1, 3)), np.zeros((1, 2 * N)), lb, ub).status[0] == 1
    for wp in ([last + 1], [last, last + 1], [N_WP - 1]):
        B = len(wp)
        with pytest.raises(mpmpc.MpmpcError, match="Reached end of path!"):
            h.solve(np.array(wp, np.int32), np.zeros((B, 3)), np.zeros((B, 2 * N)), np.repeat(lb, B, 0), np.repeat(ub, B, 0))


@pytest.mark.parametrize("key", ["free", "obstacles"])
def test_corridor_code_matches_reference_on_the_open_path(key, emu, g1, g3):
    """K0's per-thread code on the 767 x 867 grid (a row / column swap cannot hide on it): bit exact on every column the
    reference could build; no row without a free segment."""
    grid = _grid(g1, "grid_" + key)
    sm = float(g3["safety_margin"][0])
    nc = 50
    ub, lb, nseg = np.zeros((N_WP, nc)), np.zeros((N_WP, nc)), np.zeros(N_WP, np.int32)
    arrs = [np.ascontiguousarray(g1[k], float) for k in ("x", "y", "psi", "ds_next")]
    bu, bl = np.ascontiguousarray(g1["border_ub"], float), np.ascontiguousarray(g1["border_lb"], float)
    bad = emu.lib.emu_corridor(C.c_int(grid.shape[0]), C.c_int(grid.shape[1]), grid.ctypes.data_as(C.POINTER(C.c_int8)),
                               C.c_double(g1["origin"][0]), C.c_double(g1["origin"][1]), C.c_double(g1["resolution"][0]),
                               C.c_int(N_WP), *[_d(a) for a in arrs], C.c_int(0), _d(bu), _d(bl), C.c_int(nc),
                               C.c_double(2 * sm), C.c_double(sm), _d(ub), _d(lb), nseg.ctypes.data_as(C.POINTER(C.c_int32)))
    assert bad == int(g3["value_error_" + key].sum()) == 0
    v = g3["valid_cols_" + key]
    for w in range(N_WP):
        assert np.array_equal(ub[w, :v[w]], g3["ub_" + key][w, :v[w]]) and np.array_equal(lb[w, :v[w]], g3["lb_" + key][w, :v[w]]), w
    assert nseg.min() >= 1 and nseg.max() == (2 if key == "obstacles" else 1)


# ======================================================================================================== rollout end (host code)
def _localise(emu, g1, s, pose, N, circular):
    cum = np.ascontiguousarray(np.cumsum(g1["segment_lengths"]))
    gx, gy, gpsi = (np.ascontiguousarray(g1[k]) for k in ("x", "y", "psi"))
    x0, alive = np.zeros(3), C.c_int(7)
    wp = emu.lib.emu_localise(C.c_int(N_WP), C.c_int(N), C.c_int(int(circular)), _d(cum), _d(gx), _d(gy), _d(gpsi),
                              C.c_double(float(s)), _d(np.ascontiguousarray(pose, float)), _d(x0), C.byref(alive))
    return wp, x0, alive.value


def test_localise_reproduces_the_reference_trace_and_ends_the_open_path(emu, g1):
    g = _load("g6_closed_loop_real_N30.npz")
    N = 30
    for t in range(g["s"].size):                                    # every step of the reference's run: running
        wp, x0, alive = _localise(emu, g1, g["s"][t], g["pose"][t], N, False)
        assert wp == g["wp_id"][t] and np.allclose(x0, g["x0"][t], rtol=0, atol=1e-14) and alive == 1, t
    # the state at which the reference's get_control exited: the car ends with -2, after writing wp_id and x0
    wp, x0, alive = _localise(emu, g1, g["exit_s"][0], g["exit_pose"], N, False)
    assert alive == -2 and wp == g["exit_wp_id"][0] and np.allclose(x0, g["exit_x0"], rtol=0, atol=1e-14)
    # one waypoint earlier the horizon still fits; a circular path never ends; past the length: 0
    cum = np.cumsum(g1["segment_lengths"])
    w = int(g["exit_wp_id"][0]) - 1
    pose = np.array([g1["x"][w], g1["y"][w], g1["psi"][w]])
    assert _localise(emu, g1, cum[w], pose, N, False)[::2] == (w, 1)
    assert _localise(emu, g1, g["exit_s"][0], g["exit_pose"], N, True)[2] == 1
    assert _localise(emu, g1, cum[-1] - 1e-9, pose, N, True)[2] == 1
    assert _localise(emu, g1, cum[-1] + 1e-9, pose, N, False)[::2] == (-1, 0)
    assert _localise(emu, g1, cum[N_WP - 10], pose, 10, False)[::2] == (N_WP - 10, -2)
    assert _localise(emu, g1, cum[N_WP - 11], pose, 10, False)[::2] == (N_WP - 11, 1)


# ======================================================================================================== host MPC, corridor 'host'
def test_get_control_replays_the_reference_run_and_exits_at_its_end(rtrack, g3, capsys):
    """MPC.get_control (corridor 'host', the emulated kernels behind it) on the reference's own run (G6r), teacher forced,
    and SystemExit(1) with "Reached end of path!" at the step where the reference exited."""
    from spatial_bicycle_models import TemporalState
    g = _load("g6_closed_loop_real_N30.npz")
    N = 30
    m, rp, car = _real_world()
    mpc = _make_mpc(car, N, rtrack, "emu", settings=mpmpc.default_settings(phase1_accept=0))
    T_ = g["s"].size
    cc_prev = np.vstack([g["cc_prev0"][None, :], g["cc_next"][:-1]])
    for t in list(range(0, T_, 12)) + list(range(T_ - 4, T_)):
        car.s = float(g["s"][t])
        car.temporal_state = TemporalState(*g["pose"][t])
        mpc.current_control = cc_prev[t].copy()
        mpc.infeasibility_counter = int(g["counter"][t - 1]) if t > 0 else 0
        u = mpc.get_control()
        assert car.wp_id == g["wp_id"][t] and np.allclose(np.array(car.spatial_state[:]), g["x0"][t], atol=1e-13)
        # the corridor this step handed over (MPC._init_problem) is G3r's row wp_id
        ub_t, lb_t, _ = rp.update_path_constraints(car.wp_id + 1, N, 2 * car.safety_margin, car.safety_margin)
        assert np.array_equal(lb_t, g3["lb_free"][car.wp_id, :N]) and np.array_equal(ub_t, g3["ub_free"][car.wp_id, :N])
        assert (mpc.last_status > 0) == (g["status"][t] > 0) and mpc.infeasibility_counter == g["counter"][t]
        assert np.max(np.abs(u - g["u"][t])) <= 1e-6, t
        d = np.abs(mpc.current_control - g["cc_next"][t])
        d[-1] = 0.0                                       # kappa_{N-1} is cost free
        assert d.max() <= 1e-6, t
    capsys.readouterr()
    car.s = float(g["exit_s"][0])
    car.temporal_state = TemporalState(*g["exit_pose"])
    mpc.current_control = g["exit_cc_prev"].copy()
    mpc.infeasibility_counter = int(g["exit_counter"][0])
    status_before = mpc.last_status
    with pytest.raises(SystemExit) as e:
        mpc.get_control()
    assert e.value.code == 1 and "Reached end of path!" in capsys.readouterr().out
    assert car.wp_id == g["exit_wp_id"][0] and np.allclose(np.array(car.spatial_state[:]), g["exit_x0"], atol=1e-13)
    assert mpc.last_status == status_before                 # the optimizer was not called


# ======================================================================================================== GPU
def _k0_handle(rtrack, g1, N, key="free", max_batch=1, settings=None, weights="stock"):
    """a handle on Real_Track whose corridor table K0 builds on the device from the golden grid"""
    h = mpmpc.Handle(T.stock_config(N, weights, max_batch=max_batch, track=rtrack), settings or mpmpc.default_settings())
    h.set_path(rtrack.kappa, rtrack.v_ref, rtrack.ds_next)
    h.set_map(_grid(g1, "grid_" + key), tuple(g1["origin"]), float(g1["resolution"][0]))
    h.set_path_geometry(g1["x"], g1["y"], g1["psi"], g1["border_ub"], g1["border_lb"])
    sm = float(_load("g3_corridor_real.npz")["safety_margin"][0])
    ub, lb, bad = h.build_corridor(50, 2 * sm, sm)
    return h, ub, lb, bad


@pytest.mark.gpu
@pytest.mark.parametrize("N", [10, 30, 50])
def test_device_on_the_reference_captures(N, rtrack):
    """K1 bit exact against G4r, K2 at every lane packing the horizon allows: G5r's statuses, optima to 1e-6, first
    control to 1e-8."""
    g4, g5 = _g4(N)
    B = g4["s"].size
    h = mpmpc.Handle(T.stock_config(N, str(g4["weights"][0]), max_batch=B, track=rtrack))
    h.set_path(rtrack.kappa, rtrack.v_ref, rtrack.ds_next)
    inputs = (g4["wp_id"].astype(np.int32), g4["x0"], g4["cc_prev"], g4["lb"], g4["ub"])
    qp = h.assemble(*inputs)
    for c in range(B):
        Pd, q, A, l, u = T.qp_to_dense(qp[:, c, :], N)
        assert np.array_equal(q, g4["q"][c]) and np.array_equal(l, g4["l"][c]) and np.array_equal(Pd, g4["P_diag"][c])
        assert np.array_equal(A, _dense_A(g4, c, N))
        fin = np.isfinite(g4["u"][c])
        assert np.array_equal(u[~fin], g4["u"][c][~fin])
        assert np.max(np.abs(u[fin] - g4["u"][c][fin])) <= 8 * np.finfo(float).eps
    ok = g5["status"] == 1
    for packing in ((0, 64, 32, 16) if N < 32 else (0, 64)):
        h.set_packing(packing)
        sol = h.solve(*inputs, want_y=True)
        assert np.array_equal(sol.status, g5["status"]), packing
        assert np.max(np.abs(sol.z[ok] - g5["x"][ok])) <= 1e-6, packing
        assert np.max(np.abs(sol.z[ok][:, -2 * N:-2 * N + 2] - g5["x"][ok][:, -2 * N:-2 * N + 2])) <= 1e-8, packing
        assert np.max(np.abs(sol.u0[ok, 1] - np.arctan(g5["x"][ok][:, -2 * N + 1] * 0.30))) <= 1e-8, packing
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cfgid,B,N", [(4, 8192, 30), (3, 4096, 50)])
def test_device_full_batches_on_real_track_against_c_oracle(cfgid, B, N, rtrack):
    """Full batches on Real_Track (config 4 with obstacles; config 3's time-optimal weights at N = 50) against the C port
    of the oracle at strict verdicts: every status, every control; KKT certificates and Farkas rays in plain numpy on the
    device's own (z, y); nobody leaves the interior-point path for OSQP's ADMM."""
    import oracle_c as OC
    sc = scenarios.make(cfgid, rtrack, B=B, N=N)
    assert sc.wp_id.max() <= N_WP - N - 1 and np.all(np.isfinite(sc.lb)) and np.all(np.isfinite(sc.ub))
    h = mpmpc.Handle(T.stock_config(N, sc.weights, max_batch=B, track=rtrack), mpmpc.default_settings(phase1_accept=0))
    h.set_path(rtrack.kappa, rtrack.v_ref, rtrack.ds_next)
    qp = h.assemble(sc.wp_id, sc.x0, sc.cc_prev, sc.lb, sc.ub)
    sol = h.solve(sc.wp_id, sc.x0, sc.cc_prev, sc.lb, sc.ub, want_y=True)
    h.close()
    ocfg = OC.mpc_cfg(N, scenarios.WEIGHTS[sc.weights], rtrack.umin, rtrack.umax, scenarios.XMIN, scenarios.XMAX, 4.0,
                      rtrack.car_length, circular=False)
    ref = OC.mpc_batch(ocfg, OC.settings(), rtrack.kappa, rtrack.v_ref, rtrack.ds_next, sc.wp_id, sc.x0, sc.cc_prev,
                       sc.lb, sc.ub, want_y=True)
    assert np.array_equal(sol.status, ref["status"])
    assert set(np.unique(sol.status)) <= {1, mpmpc.PRIMAL_INFEASIBLE} and np.mean(sol.status == 1) > 0.5
    assert np.array_equal(sol.iters[:, 0], ref["iters"][:, 0]) and sol.iters[:, 0].max() <= 1     # no ADMM fallback
    worst, alt = T.controls_vs_reference(qp, N, sol, ref, 1e-6)
    assert worst <= 1e-6 and len(alt) <= 2, (worst, alt)
    both = sol.status == 1
    prim, stat, comp = T.kkt_batch(qp[:, both, :], N, sol.z[both], sol.y[both])
    assert max(prim.max(), stat.max(), comp.max()) <= 1e-8
    inf = ~both
    if inf.any():
        ok, support, aty = T.farkas_batch(qp[:, inf, :], N, sol.y[inf])
        assert ok.all(), (support.max(), aty.max())


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["free", "obstacles"])
def test_device_corridor_on_the_non_square_map(key, rtrack, g1, g3):
    h, ub, lb, bad = _k0_handle(rtrack, g1, 30, key)
    h.close()
    assert bad == int(g3["value_error_" + key].sum())               # (the end-of-path rows are not bad rows)
    v = g3["valid_cols_" + key]
    for w in range(N_WP):
        assert np.array_equal(ub[w, :v[w]], g3["ub_" + key][w, :v[w]]) and np.array_equal(lb[w, :v[w]], g3["lb_" + key][w, :v[w]]), w
    assert np.all(np.isfinite(ub)) and np.all(np.isfinite(lb))


@pytest.mark.gpu
def test_device_speed_profile_on_real_track(g1):
    g2 = _load("g2_speed_profile_real.npz")
    n = N_WP - 1
    v, status, iters = mpmpc.speed_profile(g1["ds_next"][:n], g1["kappa"][:n].astype(float), g2["constraints"])
    assert status[0] == 1
    assert np.max(np.abs(v[0] - g2["x"])) <= 1e-9 and np.max(np.abs(v[0] - g2["v_ref"][:-1])) <= 1e-9


@pytest.mark.gpu
def test_device_rollout_replays_the_reference_run_and_ends_it(rtrack, g1):
    """K3, teacher forced on G6r as tests/test_rollout.py does on G6: every recorded step is a car, one rollout step, each
    car lands where the reference's step landed.  One more car sits at the state where the reference's get_control
    exited: it ends with alive = -2 at the reference's wp_id and x0."""
    g = _load("g6_closed_loop_real_N30.npz")
    N = 30
    T_ = g["s"].size
    s = np.concatenate([g["s"], g["exit_s"]])
    pose = np.vstack([g["pose"], g["exit_pose"][None, :]])
    cc = np.vstack([g["cc_prev0"][None, :], g["cc_next"][:-1], g["exit_cc_prev"][None, :]])
    counter = np.concatenate([[0], g["counter"][:-1], g["exit_counter"]]).astype(np.int32)
    h, _, _, bad = _k0_handle(rtrack, g1, N, "free", max_batch=T_ + 1, settings=mpmpc.default_settings(phase1_accept=0))
    assert bad == 0
    cum = np.cumsum(g1["segment_lengths"])
    h.rollout_warm_start(False)
    h.rollout_init(0.05, cum, s, pose, cc0=cc)
    h.rollout_set_counters(counter)
    h.rollout_step(1)
    st = h.rollout_state()
    h.close()
    assert np.array_equal(st["wp_id"][:T_], g["wp_id"])
    assert np.max(np.abs(st["x0"][:T_] - g["x0"])) <= 1e-13
    assert np.array_equal(st["status"][:T_] > 0, g["status"] > 0)
    assert np.array_equal(st["counter"][:T_], g["counter"])
    assert np.max(np.abs(st["u"][:T_] - g["u"])) <= 1e-6
    d = np.abs(st["cc"][:T_] - g["cc_next"])
    d[:, -1] = 0.0                                                  # kappa_{N-1} is cost free
    assert d.max() <= 1e-6
    assert np.all(st["alive"][:T_] == 1)
    assert np.max(np.abs(st["s"][:T_ - 1] - g["s"][1:])) <= 1e-7
    assert np.max(np.abs(st["pose"][:T_ - 1] - g["pose"][1:])) <= 1e-7
    # the exit car: ended, not driven
    assert st["alive"][T_] == -2 and st["wp_id"][T_] == g["exit_wp_id"][0]
    assert np.max(np.abs(st["x0"][T_] - g["exit_x0"])) <= 1e-13
    assert st["s"][T_] == g["exit_s"][0] and np.array_equal(st["pose"][T_], g["exit_pose"])


@pytest.mark.gpu
def test_device_rollout_fleet_runs_to_the_end_of_the_open_path(rtrack, g1, track):
    """64 cars spread along Real_Track, rolled until none runs: every one ends at the end of the path (alive = -2, its
    horizon past the last waypoint), none drives on to s >= length.  On the circular Sim_Track no car ever gets -2."""
    N, B = 30, 64
    cum = np.cumsum(g1["segment_lengths"])
    starts = np.linspace(0, N_WP - N - 2, B).astype(int)
    poses = np.stack([g1["x"][starts], g1["y"][starts], g1["psi"][starts]], axis=1)
    h, _, _, _ = _k0_handle(rtrack, g1, N, "free", max_batch=B)
    h.rollout_init(0.05, cum, cum[starts], poses)
    h.rollout_step(1200)                                            # 59.5 m at <= 1 m/s, Ts = 0.05: <= 1190 steps
    st = h.rollout_state()
    h.close()
    assert np.all(st["alive"] == -2), np.unique(st["alive"], return_counts=True)
    assert np.all(st["wp_id"] == N_WP - N)                          # the first waypoint whose horizon passes the end
    assert np.all(st["s"] < cum[-1])
    # circular: the lap ends with alive = 0, never with -2
    g1s = _load("g1_path_sim_track.npz")
    g3s = _load("g3_corridor.npz")
    cum_s = np.cumsum(g1s["segment_lengths"])
    starts = np.linspace(0, 199, B).astype(int)
    h = mpmpc.Handle(T.stock_config(N, max_batch=B))
    h.set_path(track.kappa, track.v_ref, track.ds_next)
    h.set_corridor(g3s["ub_free"], g3s["lb_free"])
    h.set_path_geometry(g1s["x"], g1s["y"], g1s["psi"], g1s["border_ub"], g1s["border_lb"])
    h.rollout_init(0.05, cum_s, cum_s[starts], np.stack([g1s["x"][starts], g1s["y"][starts], g1s["psi"][starts]], axis=1))
    seen = set()
    for _ in range(5):
        h.rollout_step(50)
        seen |= set(np.unique(h.rollout_state()["alive"]).tolist())
    h.close()
    assert -2 not in seen and seen <= {0, 1} and 0 in seen


@pytest.mark.gpu
def test_device_solve_boundary_at_the_end_of_the_path(rtrack):
    """The batch call keeps its contract: a start whose horizon passes the last waypoint refuses the WHOLE call
    (MPMPC_E_ARG, the reference's message); the last legal start solves."""
    N = 30
    last = N_WP - N - 1
    h = mpmpc.Handle(T.stock_config(N, max_batch=4, track=rtrack))
    h.set_path(rtrack.kappa, rtrack.v_ref, rtrack.ds_next)
    lb, ub = rtrack.lb_free[[last], :N], rtrack.ub_free[[last], :N]
    sol = h.solve(np.array([last], np.int32), np.zeros((1, 3)), np.zeros((1, 2 * N)), lb, ub)
    assert sol.status[0] == 1
    for wp in ([last + 1], [last, last, last, last + 1], [N_WP - 1]):
        B = len(wp)
        with pytest.raises(mpmpc.MpmpcError, match="Reached end of path!"):
            h.solve(np.array(wp, np.int32), np.zeros((B, 3)), np.zeros((B, 2 * N)), np.repeat(lb, B, 0), np.repeat(ub, B, 0))
    h.close()


@pytest.mark.gpu
def test_get_control_with_device_corridor_exits_like_the_reference(rtrack, capsys):
    """MPC.get_control with corridor='device' (K0 table, libmpmpc.so) on G6r: same controls as the reference's run, and at
    its end SystemExit(1) with "Reached end of path!" - not a library error - at the step where the reference exited."""
    from spatial_bicycle_models import TemporalState
    g = _load("g6_closed_loop_real_N30.npz")
    N = 30
    m, rp, car = _real_world()
    mpc = _make_mpc(car, N, rtrack, corridor="device", settings=mpmpc.default_settings(phase1_accept=0))
    assert isinstance(mpc.optimizer, mpmpc.Handle)
    T_ = g["s"].size
    cc_prev = np.vstack([g["cc_prev0"][None, :], g["cc_next"][:-1]])
    for t in list(range(0, T_, 5)) + [T_ - 1]:
        car.s = float(g["s"][t])
        car.temporal_state = TemporalState(*g["pose"][t])
        mpc.current_control = cc_prev[t].copy()
        mpc.infeasibility_counter = int(g["counter"][t - 1]) if t > 0 else 0
        u = mpc.get_control()
        assert car.wp_id == g["wp_id"][t] and mpc.infeasibility_counter == g["counter"][t]
        assert (mpc.last_status > 0) == (g["status"][t] > 0)
        assert np.max(np.abs(u - g["u"][t])) <= 1e-6, t
    capsys.readouterr()
    car.s = float(g["exit_s"][0])
    car.temporal_state = TemporalState(*g["exit_pose"])
    mpc.current_control = g["exit_cc_prev"].copy()
    with pytest.raises(SystemExit) as e:
        mpc.get_control()
    assert e.value.code == 1 and "Reached end of path!" in capsys.readouterr().out
    assert car.wp_id == g["exit_wp_id"][0]
