"""Per-car obstacle worlds in the device rollout (K0c, mpmpc_rollout_set_obstacles): every car drives the base map with
its own circular obstacles added, and its corridor row is rebuilt from that world at every step.

Against golden G3o / G6o (tests/golden/make_g3o.py: the reference's Map.add_obstacles + update_path_constraints, and its
closed loop, in seeded obstacle worlds) and against the shared-table rollout run once per world."""
import ctypes as C

import numpy as np
import pytest

import mpc_np as M
import mpmpc
import mpmpc_testlib as T
import scenarios
import twins
from map import Map, Obstacle
from reference_path import ReferencePath

_d, _i, _g1, _sm = T._d, T._i, T.g1_world, T.safety_margin


@pytest.fixture(scope="module")
def twin():
    """The CPU twin of K0c (tests/emul_car)."""
    return twins.car()


def _twin_rows(twin, track, grid, disc_lists, wp_ids, N, sm):
    g1, _, origin, res = _g1(track)
    arrs = [np.ascontiguousarray(g1[k], float) for k in ("x", "y", "psi", "ds_next", "border_ub", "border_lb")]
    off, flat = T.csr(disc_lists, 3, pad=False)
    B = len(disc_lists)
    wp = np.ascontiguousarray(wp_ids, np.int32)
    ub, lb, flag = np.zeros((B, N)), np.zeros((B, N)), np.zeros(B, np.int32)
    rc = twin.car_emu_rows(grid.shape[0], grid.shape[1], grid.ctypes.data_as(C.POINTER(C.c_int8)), origin[0], origin[1],
                           res, arrs[0].size, *[_d(a) for a in arrs[:4]], 1 if track == "sim" else 0, _d(arrs[4]),
                           _d(arrs[5]), N, 2 * sm, sm, B, _i(wp), _i(off), _i(flat), _d(ub), _d(lb), _i(flag))
    assert rc == 0
    return ub, lb, flag


def _g3o(track):
    return np.load(M.GOLDEN + "/g3o_%s_obstacles.npz" % track)


# ------------------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("track", ["sim", "real"])
def test_obstacle_discs_rasterise_like_add_obstacles(track, twin):
    g1, grid, origin, res = _g1(track)
    rng = np.random.default_rng(7 if track == "sim" else 8)
    H, W = grid.shape
    span = (origin[0], origin[0] + W * res, origin[1], origin[1] + H * res)
    rmax = 0.09 if track == "sim" else 0.4
    obs = []
    while len(obs) < 50:
        r = rng.uniform(0.01, rmax)
        cx, cy = rng.uniform(span[0] + r + 2 * res, span[1] - r - 2 * res), rng.uniform(span[2] + r + 2 * res, span[3] - r - 2 * res)
        obs.append(Obstacle(cx, cy, r))
    m = Map.from_grid(grid, origin, res)
    discs = m.obstacle_discs(obs)
    assert discs.dtype == np.int32 and discs.shape == (50, 3)
    m.add_obstacles(obs)
    mine = grid.copy()
    yy, xx = np.mgrid[0:H, 0:W]
    for cx, cy, r in discs.tolist():
        dx, dy = xx - cx, yy - cy
        mine[(dx >= -r) & (dx < r) & (dy >= -r) & (dy < r) & (dx * dx + dy * dy <= r * r)] = 0
    assert np.array_equal(mine, m.data)
    # the validation the library runs (cor_check_obstacles): inside is fine, a square leaving the grid is refused
    off = np.array([0, 50], np.int32)
    assert twin.car_emu_check(1, 8, _i(off), _i(np.ascontiguousarray(discs)), 1, W, H) == 0
    for bad in ([5, 3, 6], [W - 2, 40, 3], [40, H - 1, 2], [40, 2, 3], [40, 40, -1]):
        d = np.array([bad], np.int32)
        assert twin.car_emu_check(1, 8, _i(np.array([0, 1], np.int32)), _i(d), 1, W, H) == -1, bad
    d = np.array([[3, 3, 3], [W - 3, H - 3, 3]], np.int32)             # touching the edges from inside
    assert twin.car_emu_check(1, 8, _i(np.array([0, 2], np.int32)), _i(d), 1, W, H) == 0


@pytest.mark.parametrize("track", ["sim", "real"])
def test_twin_reproduces_g3o_rows_bit_exact(track, twin):
    g = _g3o(track)
    _, grid, origin, res = _g1(track)
    sm, N = float(g["safety_margin"][0]), int(g["n_cols"][0])
    n_blocked = 0
    for k in range(int(g["n_sets"][0])):
        ub_ref, lb_ref, blocked = g["ub_%d" % k], g["lb_%d" % k], g["blocked_%d" % k]
        n = ub_ref.shape[0]
        ub, lb, flag = _twin_rows(twin, track, grid, [g["discs_%d" % k]] * n, np.arange(n), N, sm)
        assert np.array_equal(ub, ub_ref, equal_nan=True) and np.array_equal(lb, lb_ref, equal_nan=True)
        assert np.array_equal(flag == 1, blocked) and np.all(flag != 2)
        n_blocked += blocked.sum()
    if track == "sim":
        assert n_blocked >= 1           # the blocked-row path is exercised


def test_twin_matches_host_classes_on_random_worlds(twin):
    """the host mirror of the reference (Map.add_obstacles + ReferencePath.update_path_constraints) on a Map copy"""
    g1, grid, origin, res = _g1("sim")
    sm, N = float(_g3o("sim")["safety_margin"][0]), 30
    rng = np.random.default_rng(11)
    n = g1["x"].size
    for world in range(3):
        obs = [Obstacle(c[0] + rng.uniform(-0.05, 0.05), c[1] + rng.uniform(-0.05, 0.05), rng.uniform(0.04, 0.09))
               for c in [(0.0, 0.0), (-0.8, -0.5), (-0.7, -1.5), (-0.3, -1.0), (0.27, -1.0), (0.78, -1.47), (0.73, -0.9),
                         (1.2, 0.0), (0.67, -0.05)]]
        m = Map.from_grid(grid, origin, res)
        discs = m.obstacle_discs(obs)
        m.add_obstacles(obs)
        rp = ReferencePath.from_tables(m, g1["x"], g1["y"], g1["psi"], g1["kappa"], circular=True,
                                       border_ub=g1["border_ub"], border_lb=g1["border_lb"])
        starts = np.arange(0, n, 3)
        ub, lb, flag = _twin_rows(twin, "sim", grid, [discs] * starts.size, starts, N, sm)
        for j, w in enumerate(starts):
            try:
                u, l, _ = rp.update_path_constraints(int(w) + 1, N, 2 * sm, sm)
            except ValueError:
                assert flag[j] == 1
                continue
            assert flag[j] == 0 and np.array_equal(ub[j], u) and np.array_equal(lb[j], l)


@pytest.mark.parametrize("track", ["sim", "real"])
def test_the_four_k0c_entry_points_agree_with_every_feature_off(track, twin):
    """car_emu_rows, wall_emu_rows, look_emu_rows and tlk_emu_rows are one restatement of K0c (tests/emul_car/car_rows.hpp) behind
    four argument lists: without walls, routes, lookahead and traffic tables they return the same ub, lb and flag, bit for bit.
    One car per start waypoint, 0 .. 6 discs each on the border lines of the waypoints 1 .. 29 ahead of it (seeded: count, then
    per disc waypoint, fraction of the way from the upper to the lower border point, radius)."""
    N = 30
    g1, grid, origin, res = _g1(track)
    sm, n = _sm(track), g1["x"].size
    starts = np.arange(n if track == "sim" else n - N - 1)
    rng = np.random.default_rng(5)
    lists = []
    for w in starts:
        d = []
        for _ in range(rng.integers(0, 7)):
            i, f, r = (w + rng.integers(1, 30)) % n, rng.uniform(-0.1, 1.1), rng.integers(1, (39 if track == "sim" else 11) + 1)
            p = g1["border_ub"][i] + f * (g1["border_lb"][i] - g1["border_ub"][i])
            d.append([int(np.floor((p[0] - origin[0]) / res)), int(np.floor((p[1] - origin[1]) / res)), int(r)])
        lists.append(np.asarray(d, np.int32).reshape(-1, 3))
    B = starts.size
    off, flat = T.csr(lists, 3)
    arrs = [np.ascontiguousarray(g1[k], float) for k in ("x", "y", "psi", "ds_next", "border_ub", "border_lb")]
    wp = np.ascontiguousarray(starts, np.int32)
    head = (grid.shape[0], grid.shape[1], T._b(grid), origin[0], origin[1], res, n, *[_d(a) for a in arrs[:4]],
            1 if track == "sim" else 0, _d(arrs[4]), _d(arrs[5]), N, 2 * sm, sm, B, _i(wp))
    no_walls = T.csr([[]] * B, 4)

    def rows(fn, off, flat, *rest):
        ub, lb, flag = np.full((B, N), -7.0), np.full((B, N), -7.0), np.full(B, -7, np.int32)
        assert fn(*head, _i(off), _i(flat), *rest, _d(ub), _d(lb), _i(flag)) == 0
        return ub, lb, flag

    car = rows(twin.car_emu_rows, off, flat)
    others = dict(walls=rows(twins.walls().wall_emu_rows, off, flat, _i(no_walls[0]), _i(no_walls[1])),
                  look=rows(twins.lookahead().look_emu_rows, off, flat, None, None, None, None, None),
                  look_empty_walls=rows(twins.lookahead().look_emu_rows, off, flat, _i(no_walls[0]), _i(no_walls[1]), None, None, None),
                  tlk=rows(twins.traffic_lookahead().tlk_emu_rows, off, flat, None, None, None, None, None, 0, None))
    for name, got in others.items():
        assert np.array_equal(got[0], car[0], equal_nan=True) and np.array_equal(got[1], car[1], equal_nan=True), name
        assert np.array_equal(got[2], car[2]), name
    # not an empty world: the discs change rows, and block some
    free = rows(twin.car_emu_rows, *T.csr([[]] * B, 3))
    changed = [not (np.array_equal(car[0][b], free[0][b], equal_nan=True) and np.array_equal(car[1][b], free[1][b], equal_nan=True)
                    and car[2][b] == free[2][b]) for b in range(B)]
    print("%s: %d of %d rows changed by the discs, %d cars blocked" % (track, sum(changed), B, int((car[2] == 1).sum())))
    assert sum(changed) >= 100 and (car[2] == 1).sum() >= 1


def test_set_obstacles_validation_without_device(twin, built_library):
    lib = mpmpc.load_library(built_library)
    off, d = np.array([0, 1], np.int32), np.array([[50, 50, 3]], np.int32)
    assert lib.mpmpc_rollout_set_obstacles(None, 1, _i(off), _i(d)) == mpmpc_E_ARG
    assert lib.mpmpc_rollout_corridor(None, 1, None, None) == mpmpc_E_ARG
    W = H = 500
    ok = dict(B=1, max_batch=8, built=1)

    def check(off, discs, B=1, max_batch=8, built=1):
        return twin.car_emu_check(B, max_batch, _i(np.asarray(off, np.int32)),
                                  _i(np.ascontiguousarray(np.asarray(discs, np.int32).reshape(-1, 3))), built, W, H)
    assert check([0, 1], [[50, 50, 3]], **ok) == 0
    assert check([0, 0, 0], np.zeros((0, 3)), B=2) == 0                   # cars without obstacles
    assert check([1, 1], [[50, 50, 3]]) == -1                             # offsets[0] != 0
    assert check([0, 2, 1], [[50, 50, 3], [60, 60, 3]], B=2) == -1         # decreasing
    assert check([0, 1], [[50, 50, 3]], B=0) == -1 and check([0, 1, 1], [[50, 50, 3]], B=2, max_batch=1) == -1
    assert check([0, 64], [[50, 50, 3]] * 64) == 0
    assert check([0, 65], [[50, 50, 3]] * 65) == -1                       # more than COR_MAX_DISCS per car
    assert check([0, 1], [[50, 50, 3]], built=0) == -3                     # no build of the current map: E_STATE


# ------------------------------------------------------------------------------------------------------------ GPU
mpmpc_E_ARG, mpmpc_E_STATE = -1, -3


def _handle(track, N, B, warm=False, settings=None):
    tr = scenarios.sim_track() if track == "sim" else scenarios.real_track()
    g1, grid, origin, res = _g1(track)
    h = mpmpc.Handle(T.stock_config(N, max_batch=B, track=None if track == "sim" else tr),
                     settings or mpmpc.default_settings())
    h.set_path(tr.kappa, tr.v_ref, tr.ds_next)
    h.set_map(grid, origin, res)
    h.set_path_geometry(g1["x"], g1["y"], g1["psi"], g1["border_ub"], g1["border_lb"])
    h.rollout_warm_start(warm)
    return h, tr, g1, grid, origin, res


def _world_grid(grid, discs):
    g = grid.copy()
    H, W = g.shape
    yy, xx = np.mgrid[0:H, 0:W]
    for cx, cy, r in np.asarray(discs).reshape(-1, 3).tolist():
        dx, dy = xx - cx, yy - cy
        g[(dx >= -r) & (dx < r) & (dy >= -r) & (dy < r) & (dx * dx + dy * dy <= r * r)] = 0
    return g


@pytest.mark.gpu
@pytest.mark.parametrize("track", ["sim", "real"])
def test_device_rows_equal_g3o_bit_exact(track):
    g = _g3o(track)
    sm, N = _sm(track), int(g["n_cols"][0])
    sets = int(g["n_sets"][0])
    n = g["ub_0"].shape[0]
    B = sets * n
    h, tr, g1, grid, origin, res = _handle(track, N, B)
    h.build_corridor(N, 2 * sm, sm, want_tables=False)
    cum = np.cumsum(g1["segment_lengths"])
    starts = np.tile(np.arange(n), sets)
    poses = np.stack([g1["x"][starts], g1["y"][starts], g1["psi"][starts]], 1)
    s0 = cum[starts]
    s0[starts == g1["x"].size - 1] = np.nextafter(cum[-1], 0.0)      # (s = length: the lap is over)
    h.rollout_set_obstacles([g["discs_%d" % k] for k in range(sets) for _ in range(n)])
    h.rollout_init(0.05, cum, s0, poses)
    h.rollout_step(1)
    ub, lb = h.rollout_corridor()
    st = h.rollout_state()
    h.close()
    assert np.array_equal(st["wp_id"], starts)
    ub_ref = np.concatenate([g["ub_%d" % k] for k in range(sets)])
    lb_ref = np.concatenate([g["lb_%d" % k] for k in range(sets)])
    blocked = np.concatenate([g["blocked_%d" % k] for k in range(sets)])
    assert np.array_equal(ub, ub_ref, equal_nan=True) and np.array_equal(lb, lb_ref, equal_nan=True)
    assert np.all(st["alive"][blocked] == -3)
    assert np.array_equal(st["pose"][blocked], poses[blocked]) and np.array_equal(st["s"][blocked], s0[blocked])
    assert not np.any(st["alive"][~blocked] == -3)
    if track == "sim":
        assert blocked.sum() >= 1


@pytest.mark.gpu
def test_device_rollout_replays_the_reference_trace_in_obstacle_worlds():
    """G6o teacher-forced: every recorded step of the 3 worlds is one car carrying its own world's discs, ONE launch."""
    g = np.load(M.GOLDEN + "/g6o_closed_loop_N30.npz")
    N, Tn = 30, g["s"].size
    sm = _sm("sim")
    h, tr, g1, grid, origin, res = _handle("sim", N, Tn, settings=mpmpc.default_settings(phase1_accept=0))
    h.build_corridor(N, 2 * sm, sm, want_tables=False)
    cum = np.cumsum(g1["segment_lengths"])
    world = g["world"]
    counter_prev = np.zeros(Tn, np.int32)
    for t in range(1, Tn):
        counter_prev[t] = g["counter"][t - 1] if world[t] == world[t - 1] else 0
    h.rollout_set_obstacles([g["discs_%d" % w] for w in world])
    h.rollout_init(0.05, cum, g["s"], g["pose"], cc0=g["cc_prev"])
    h.rollout_set_counters(counter_prev)
    h.rollout_step(1)
    ub, lb = h.rollout_corridor()
    st = h.rollout_state()
    h.close()
    assert np.array_equal(ub, g["ub"]) and np.array_equal(lb, g["lb"])
    assert np.array_equal(st["wp_id"], g["wp_id"])
    assert np.max(np.abs(st["x0"] - g["x0"])) <= 1e-13
    ok = g["status"] > 0
    assert np.array_equal(st["status"] > 0, ok)
    assert np.array_equal(st["counter"], g["counter"])
    assert np.max(np.abs(st["u"] - g["u"])) <= 1e-6
    same = world[:-1] == world[1:]
    d = np.abs(st["cc"][:-1][same] - g["cc_prev"][1:][same])               # (a step's new plan is the next one's cc_prev)
    d[:, -1] = 0.0                                                          # kappa_{N-1} is cost free
    assert d.max() <= 1e-6
    assert np.all(st["alive"] == 1)
    assert np.max(np.abs(st["s"][:-1][same] - g["s"][1:][same])) <= 1e-7
    assert np.max(np.abs(st["pose"][:-1][same] - g["pose"][1:][same])) <= 1e-7


def _random_worlds(track, n, seed, grid, origin, res):
    rng = np.random.default_rng(seed)
    base = [(0.0, 0.0, 0.05), (-0.8, -0.5, 0.08), (-0.7, -1.5, 0.05), (-0.3, -1.0, 0.08), (0.27, -1.0, 0.05),
            (0.78, -1.47, 0.05), (0.73, -0.9, 0.07), (1.2, 0.0, 0.08), (0.67, -0.05, 0.06)]
    jit, rr = (0.05, (0.04, 0.07)) if track == "sim" else (0.2, None)
    if track == "real":
        base = [(-6.3, -11.1, 0.20), (-2.2, -6.8, 0.25), (2.0, -0.2, 0.25), (6.0, 5.0, 0.3), (7.42, 4.97, 0.3)]
    m = Map.from_grid(grid, origin, res)
    out = []
    for _ in range(n):
        obs = [Obstacle(c[0] + rng.uniform(-jit, jit), c[1] + rng.uniform(-jit, jit),
                        rng.uniform(*rr) if rr else c[2] * rng.uniform(0.8, 1.2)) for c in base]
        out.append(m.obstacle_discs(obs))
    return out


def _fleet_vs_per_world(track, N, B, n_worlds, steps, warm, seed):
    sm = _sm(track)
    h, tr, g1, grid, origin, res = _handle(track, N, B, warm=warm)
    cum = np.cumsum(g1["segment_lengths"])
    n_wp = g1["x"].size
    rng = np.random.default_rng(seed)
    hi = n_wp if track == "sim" else n_wp - N - steps // 2 - 5
    starts = rng.integers(0, hi, B)
    poses = np.stack([g1["x"][starts], g1["y"][starts], g1["psi"][starts]], 1)
    poses[:, 2] += rng.uniform(-0.05, 0.05, B)
    worlds = []
    for d in _random_worlds(track, 4 * n_worlds, seed, grid, origin, res):      # worlds without a blocked start row
        h.set_map(_world_grid(grid, d), origin, res)
        if h.build_corridor(N, 2 * sm, sm, want_tables=False)[2] == 0:
            worlds.append(d)
        if len(worlds) == n_worlds:
            break
    assert len(worlds) == n_worlds
    wid = np.arange(B) % n_worlds
    keys = ("s", "pose", "cc", "wp_id", "status", "counter", "alive")
    ref = {k: None for k in keys}
    for w in range(n_worlds):
        h.set_map(_world_grid(grid, worlds[w]), origin, res)
        h.build_corridor(N, 2 * sm, sm, want_tables=False)
        h.rollout_set_obstacles(None)
        h.rollout_init(0.05, cum, cum[starts], poses)
        h.rollout_step(steps)
        st = h.rollout_state()
        for k in keys:
            if ref[k] is None:
                ref[k] = np.zeros_like(st[k])
            ref[k][wid == w] = st[k][wid == w]
    h.set_map(grid, origin, res)
    h.build_corridor(N, 2 * sm, sm, want_tables=False)
    h.rollout_set_obstacles([worlds[w] for w in wid])
    h.rollout_init(0.05, cum, cum[starts], poses)
    h.rollout_step(steps)
    got = h.rollout_state()
    h.close()
    for k in keys:
        assert np.array_equal(got[k], ref[k]), k
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("warm", [False, True])
def test_fleet_of_worlds_equals_per_world_rollouts(warm):
    got = _fleet_vs_per_world("sim", 30, 1024, 16, 60, warm, seed=21)
    assert (got["alive"] == 1).sum() > 512 and not np.any(got["alive"] < -2)      # (the others finished their lap)


@pytest.mark.gpu
def test_fleet_of_worlds_equals_per_world_rollouts_real_track_long_horizon():
    got = _fleet_vs_per_world("real", 70, 64, 4, 30, False, seed=22)
    assert (got["alive"] == 1).sum() > 32 and not np.any(got["alive"] < -2)


@pytest.mark.gpu
def test_obstacles_changed_between_steps():
    """half the cars get new obstacles after 20 steps: the next 20 equal a fresh rollout started from step 20's state"""
    N, B, sm = 30, 256, _sm("sim")
    h, tr, g1, grid, origin, res = _handle("sim", N, B)
    h.build_corridor(N, 2 * sm, sm, want_tables=False)
    cum = np.cumsum(g1["segment_lengths"])
    rng = np.random.default_rng(31)
    starts = rng.integers(0, g1["x"].size, B)
    poses = np.stack([g1["x"][starts], g1["y"][starts], g1["psi"][starts]], 1)
    w0 = _random_worlds("sim", B, 32, grid, origin, res)
    w1 = _random_worlds("sim", B, 33, grid, origin, res)
    mixed = [w1[b] if b % 2 else w0[b] for b in range(B)]
    h.rollout_set_obstacles(w0)
    h.rollout_init(0.05, cum, cum[starts], poses)
    h.rollout_step(20)
    mid = h.rollout_state()
    h.rollout_set_obstacles(mixed)
    h.rollout_step(20)
    a = h.rollout_state()
    ua, la = h.rollout_corridor()
    # fresh rollout from the state after step 20 (the same handle: the base build is unchanged)
    h.rollout_set_obstacles(mixed)
    h.rollout_init(0.05, cum, mid["s"], mid["pose"], cc0=mid["cc"])
    h.rollout_set_counters(mid["counter"])
    h.rollout_step(20)
    b = h.rollout_state()
    ub_, lb_ = h.rollout_corridor()
    # the unchanged cars against a run that never changed anything
    h.rollout_set_obstacles(w0)
    h.rollout_init(0.05, cum, cum[starts], poses)
    h.rollout_step(40)
    c = h.rollout_state()
    h.close()
    live = mid["alive"] == 1
    for k in ("s", "pose", "cc", "wp_id", "status", "counter", "alive"):
        assert np.array_equal(a[k][live], b[k][live]), k
        assert np.array_equal(a[k][0::2], c[k][0::2]), k
    assert np.array_equal(ua[live], ub_[live], equal_nan=True) and np.array_equal(la[live], lb_[live], equal_nan=True)
    assert not np.array_equal(a["s"][1::2], c["s"][1::2])          # the change mattered


@pytest.mark.gpu
def test_zero_obstacles_per_car_is_the_shared_table():
    N, B, sm = 30, 512, _sm("sim")
    h, tr, g1, grid, origin, res = _handle("sim", N, B)
    ub_tab, lb_tab, bad = h.build_corridor(N, 2 * sm, sm)
    cum = np.cumsum(g1["segment_lengths"])
    starts = np.random.default_rng(41).integers(0, g1["x"].size, B)
    poses = np.stack([g1["x"][starts], g1["y"][starts], g1["psi"][starts]], 1)
    out = []
    for per_car in (False, True):
        h.rollout_set_obstacles([np.zeros((0, 3), np.int32)] * B if per_car else None)
        h.rollout_init(0.05, cum, cum[starts], poses)
        h.rollout_step(1)
        if per_car:
            ub, lb = h.rollout_corridor()
            wp = h.rollout_state()["wp_id"]
            assert np.array_equal(ub, ub_tab[wp]) and np.array_equal(lb, lb_tab[wp])
        h.rollout_step(39)
        out.append(h.rollout_state())
    # state errors of the C entry points
    with pytest.raises(mpmpc.MpmpcError, match="build_corridor"):
        h.set_map(grid, origin, res)        # the base changed: the obstacles need a new build
        h.rollout_set_obstacles([np.zeros((0, 3), np.int32)] * B)
    with pytest.raises(mpmpc.MpmpcError):
        h.rollout_step(1)                   # the obstacles were set against the old base
    h.build_corridor(N, 2 * sm, sm, want_tables=False)
    with pytest.raises(mpmpc.MpmpcError, match="leaves the map"):
        h.rollout_set_obstacles([np.array([[2, 2, 3]], np.int32)] + [np.zeros((0, 3), np.int32)] * (B - 1))
    h.close()
    for k in ("s", "pose", "cc", "wp_id", "status", "counter", "alive"):
        assert np.array_equal(out[0][k], out[1][k]), k
