"""Per-car boundary walls in device worlds (K0w, the WALLS variants of K0c / K0l / K0f, K-world; mpmpc_rollout_set_walls,
mpmpc_lidar_scan_world, mpmpc_footprint_audit_world, mpmpc_world_grid).  The law: csrc/wall_core.hpp.

Everything here is an integer or the product of unchanged arithmetic on integers, so every comparison is array_equal: the
wall table against the host line_aa (and skimage's own sequences, golden G7), worlds against Map.add_obstacles +
Map.add_boundary, corridor rows against ReferencePath.update_path_constraints on a Map with the walls stamped in, lidar and
footprint against the same code on the baked grid.  CPU: the twin tests/emul_walls (the same headers).  GPU: the device.

The test world W of a track, from the committed G1 tables: a gate at every (n_wp // 7)-th waypoint from 15 on - a wall from
one static border point 55 % of the way to the other, sides alternating - and a barrier fully across 7 waypoints after the
third gate.  The host classes alone give, for Sim_Track / Real_Track: 200 / 271 start waypoints, 198 / 204 rows that differ
from the wall-free ones, 1 / 1 blocked by the barrier, 29 / 29 with a closed (0, 0) column; the tests assert >= 100, >= 1
and >= 10, so that no comparison passes on empty worlds."""
import numpy as np
import pytest

import mpc_np as M
import mpmpc
import mpmpc_testlib as T
import scenarios
import twins
from map import Map, Obstacle, line_aa
from reference_path import ReferencePath

E_ARG, E_STATE = -1, -3
N = 30
TS = 0.05
KEYS = ("s", "pose", "cc", "wp_id", "status", "counter", "alive")
CARS = dict(sim=(0.12, 0.06, 0.05), real=(0.3, 0.2, 0.3))      # length, width, reach of the footprint


_d, _i, _b, _g1, _sm, _csr = T._d, T._i, T._b, T.g1_world, T.safety_margin, T.csr


# ------------------------------------------------------------------------------------------------ fixtures and worlds
@pytest.fixture(scope="module")
def twin():
    """The CPU twin of the wall kernels (tests/emul_walls)."""
    return twins.walls()


@pytest.fixture(scope="module")
def old_twins():
    """the twins of K0l and K0f as they stand (tests/emul_lidar, tests/emul_footprint): no walls"""
    return twins.lidar(), twins.footprint()


def _gates(track):
    """-> (gates, barrier, gate waypoints, barrier waypoint): boundaries ((x0, y0), (x1, y1)) in world coordinates"""
    g1 = _g1(track)[0]
    n = g1["x"].size
    idx = list(range(15, n, n // 7))
    gates = []
    for k, i in enumerate(idx):
        a, b = (g1["border_ub"][i], g1["border_lb"][i]) if k % 2 == 0 else (g1["border_lb"][i], g1["border_ub"][i])
        gates.append((tuple(a), tuple(a + 0.55 * (b - a))))
    j = idx[2] + 7
    return gates, (tuple(g1["border_ub"][j]), tuple(g1["border_lb"][j])), idx, j


def _world_W(track):
    gates, barrier, _, _ = _gates(track)
    return gates + [barrier]


def _starts(track):
    n = _g1(track)[0]["x"].size
    return np.arange(n if track == "sim" else n - N - 1)


def _host_map(track, boundaries=(), obstacles=()):
    _, grid, origin, res = _g1(track)
    m = Map.from_grid(grid, origin, res)
    m.add_obstacles(list(obstacles))
    m.add_boundary(list(boundaries))
    return m


def _host_rows(track, boundaries, starts, obstacles=()):
    """ReferencePath.update_path_constraints(w + 1, N, 2 sm, sm) on a Map with the boundaries (and obstacles) stamped in
    -> ub, lb [n, N] (NaN rows where the reference raises), blocked [n]"""
    g1 = _g1(track)[0]
    sm = _sm(track)
    rp = ReferencePath.from_tables(_host_map(track, boundaries, obstacles), g1["x"], g1["y"], g1["psi"], g1["kappa"],
                                   circular=track == "sim", border_ub=g1["border_ub"], border_lb=g1["border_lb"])
    ub, lb = np.full((len(starts), N), np.nan), np.full((len(starts), N), np.nan)
    blocked = np.zeros(len(starts), bool)
    for j, w in enumerate(starts):
        try:
            ub[j], lb[j], _ = rp.update_path_constraints(int(w) + 1, N, 2 * sm, sm)
        except ValueError:
            blocked[j] = True
    return ub, lb, blocked


_ROWS_W = {}


def _rows_W(track):
    """the host rows of world W for every start waypoint, computed once and shared (read only)"""
    if track not in _ROWS_W:
        _ROWS_W[track] = _host_rows(track, _world_W(track), _starts(track))
        for a in _ROWS_W[track]:
            a.setflags(write=False)
    return _ROWS_W[track]


def _twin_rows(twin, track, starts, wall_lists, disc_lists=None):
    g1, grid, origin, res = _g1(track)
    sm = _sm(track)
    arrs = [np.ascontiguousarray(g1[k], float) for k in ("x", "y", "psi", "ds_next", "border_ub", "border_lb")]
    B = len(starts)
    woff, wflat = _csr(wall_lists, 4)
    off, flat = _csr(disc_lists, 3) if disc_lists is not None else (None, None)
    wp = np.ascontiguousarray(starts, np.int32)
    ub, lb, flag = np.zeros((B, N)), np.zeros((B, N)), np.zeros(B, np.int32)
    rc = twin.wall_emu_rows(grid.shape[0], grid.shape[1], _b(grid), origin[0], origin[1], res, arrs[0].size, *[_d(a) for a in arrs[:4]],
                            1 if track == "sim" else 0, _d(arrs[4]), _d(arrs[5]), N, 2 * sm, sm, B, _i(wp), _i(off), _i(flat),
                            _i(woff), _i(wflat), _d(ub), _d(lb), _i(flag))
    assert rc == 0
    return ub, lb, flag


def _twin_cells(twin, wall, want_cells=True):
    """-> (set of (x, y) the table gives, props) of one wall (x0, y0, x1, y1)"""
    w = np.ascontiguousarray(wall, np.int32)
    cap = 4 * (int(max(abs(w[2] - w[0]), abs(w[3] - w[1]))) + 2)
    xs, ys, props = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(3, np.int32)
    n = twin.wall_emu_cells(_i(w), _i(xs) if want_cells else None, _i(ys) if want_cells else None, cap, _i(props))
    assert 0 <= n <= cap, (wall, n)
    return set(zip(xs[:n].tolist(), ys[:n].tolist())), props


def _check_line(twin, wall):
    cells, props = _twin_cells(twin, wall)
    rr, cc, _ = line_aa(int(wall[0]), int(wall[1]), int(wall[2]), int(wall[3]))
    assert cells == set(zip(rr.tolist(), cc.tolist())), wall
    # every major index holds a cell and none lies outside; contiguous in the minor direction, at most 3; at most one cell
    # outside the end points' minor range
    assert props[0] == 0 and 1 <= props[1] <= 3 and props[2] <= 1, (wall, props)
    return len(cells)


def _seeded_walls(track, n, seed, max_len=None):
    """n walls (x0, y0, x1, y1) with end points in [1, W - 2] x [1, H - 2]"""
    H, W = _g1(track)[1].shape
    rng = np.random.default_rng(seed)
    a = np.stack([rng.integers(1, W - 1, n), rng.integers(1, H - 1, n)], 1)
    if max_len is None:
        b = np.stack([rng.integers(1, W - 1, n), rng.integers(1, H - 1, n)], 1)
    else:
        b = a + rng.integers(-max_len, max_len + 1, (n, 2))
        b[:, 0] = np.clip(b[:, 0], 1, W - 2)
        b[:, 1] = np.clip(b[:, 1], 1, H - 2)
    return np.ascontiguousarray(np.concatenate([a, b], 1), np.int32)


def _seeded_discs(track, n, seed):
    H, W = _g1(track)[1].shape
    rng = np.random.default_rng(seed)
    r = rng.integers(0, 12, n)
    return np.ascontiguousarray(np.stack([rng.integers(12, W - 12, n), rng.integers(12, H - 12, n), r], 1), np.int32)


def _bake(grid, discs=(), walls=()):
    """the grid with discs (cells) and walls (cells) stamped in, by numpy and the host line_aa"""
    g = grid.copy()
    H, W = g.shape
    for cx, cy, r in np.asarray(discs, np.int64).reshape(-1, 3).tolist():
        yy, xx = np.ogrid[-r:r, -r:r]
        g[cy - r:cy + r, cx - r:cx + r][xx ** 2 + yy ** 2 <= r ** 2] = 0
    for x0, y0, x1, y1 in np.asarray(walls, np.int64).reshape(-1, 4).tolist():
        xs, ys, _ = line_aa(x0, y0, x1, y1)
        g[ys, xs] = 0
    return g


# ------------------------------------------------------------------------------------------------------------ CPU
def test_wall_table_is_line_aa_for_every_short_line(twin):
    n = 0
    for dx in range(-70, 71):
        for dy in range(-70, 71):
            _check_line(twin, (100, 100, 100 + dx, 100 + dy))
            n += 1
    assert n == 19881
    assert _twin_cells(twin, (7, 9, 7, 9))[0] == {(7, 9)}      # a wall of one cell


def test_wall_table_is_skimage_on_g7_and_seeded_walls(twin):
    g = np.load(M.GOLDEN + "/g7_line_aa.npz")
    assert g["ends"].shape == (300, 4)
    for i, e in enumerate(g["ends"]):
        lo, hi = g["ptr"][i], g["ptr"][i + 1]
        cells, props = _twin_cells(twin, e)
        assert cells == set(zip(g["rr"][lo:hi].tolist(), g["cc"][lo:hi].tolist())), i      # skimage's own output
        assert props[0] == 0 and 1 <= props[1] <= 3 and props[2] <= 1, (i, props)
    total = sum(_check_line(twin, w) for w in _seeded_walls("real", 200, 501))
    assert total > 200 * 100                                                        # (long lines: hundreds of cells each)
    # long lines, extents up to 65 000: the table holds them and the three properties hold (no cell list: too long a box)
    rng = np.random.default_rng(502)
    for _ in range(60):
        a = rng.integers(1, 65001, 2)
        b = np.clip(a + rng.integers(-65000, 65001, 2) // rng.integers(1, 40), 1, 65000)
        props = _twin_cells(twin, (a[0], a[1], b[0], b[1]), want_cells=False)[1]
        assert props[0] == 0 and 1 <= props[1] <= 3 and props[2] <= 1, (a, b, props)


@pytest.mark.parametrize("track", ["sim", "real"])
def test_boundary_walls_and_twin_world_equal_the_host_map(track, twin):
    g1, grid, origin, res = _g1(track)
    H, W = grid.shape
    rng = np.random.default_rng(510 if track == "sim" else 511)
    span = (origin[0] + 3 * res, origin[0] + (W - 3) * res, origin[1] + 3 * res, origin[1] + (H - 3) * res)
    bounds = [((rng.uniform(*span[:2]), rng.uniform(*span[2:])), (rng.uniform(*span[:2]), rng.uniform(*span[2:]))) for _ in range(16)]
    rmax = 0.09 if track == "sim" else 0.4
    obs = []
    for _ in range(40):
        r = rng.uniform(0.01, rmax)
        obs.append(Obstacle(rng.uniform(span[0] + r, span[1] - r), rng.uniform(span[2] + r, span[3] - r), r))
    m = Map.from_grid(grid, origin, res)
    walls, discs = m.boundary_walls(bounds), m.obstacle_discs(obs)
    assert walls.dtype == np.int32 and walls.shape == (16, 4)
    assert np.array_equal(walls[3], m.w2m(*bounds[3][0]) + m.w2m(*bounds[3][1]))
    m.add_obstacles(obs)
    m.add_boundary(bounds)
    assert len(m.boundaries) == 16 and (m.data == 0).sum() > (grid == 0).sum() + 1000
    out = np.full_like(grid, 7)
    assert twin.wall_emu_world_grid(H, W, _b(grid), 40, _i(np.ascontiguousarray(discs)), 16, _i(np.ascontiguousarray(walls)), _b(out)) == 0
    assert np.array_equal(out, m.data)
    assert np.array_equal(_bake(grid, discs, walls), m.data)                          # (the tests' own baker)
    # the world of W
    wW = m.boundary_walls(_world_W(track))
    assert twin.wall_emu_world_grid(H, W, _b(grid), 0, None, len(wW), _i(np.ascontiguousarray(wW)), _b(out)) == 0
    assert np.array_equal(out, _host_map(track, _world_W(track)).data)


@pytest.mark.parametrize("track", ["sim", "real"])
def test_twin_rows_with_walls_equal_the_host_classes(track, twin):
    starts = _starts(track)
    assert starts.size == dict(sim=200, real=271)[track]
    ub_ref, lb_ref, blocked = _rows_W(track)
    m = _host_map(track)
    walls = m.boundary_walls(_world_W(track))
    ub, lb, flag = _twin_rows(twin, track, starts, [walls] * starts.size)
    assert np.array_equal(ub, ub_ref, equal_nan=True) and np.array_equal(lb, lb_ref, equal_nan=True)
    assert np.array_equal(flag == 1, blocked) and np.all(flag != 2)
    # the world proves something: most rows differ from the wall-free ones, the barrier blocks one, gates close columns
    ub0, lb0, flag0 = _twin_rows(twin, track, starts, [np.zeros((0, 4), np.int32)] * starts.size)
    assert np.all(flag0 == 0)
    differ = ~(np.all(ub == ub0, 1) & np.all(lb == lb0, 1))
    closed = np.any((ub == 0) & (lb == 0), 1)
    print("%s: %d start waypoints, %d rows differ, %d blocked, %d with a closed column" %
          (track, starts.size, differ.sum(), blocked.sum(), closed.sum()))
    assert differ.sum() >= 100 and blocked.sum() >= 1 and closed.sum() >= 10
    if track == "sim":                                                                # discs mixed in
        obs = [Obstacle(c[0], c[1], c[2]) for c in _g1("sim")[0]["obstacles"]]
        discs = m.obstacle_discs(obs)
        some = starts[::3]
        ub_ref, lb_ref, blocked = _host_rows("sim", _world_W("sim"), some, obs)
        ub, lb, flag = _twin_rows(twin, "sim", some, [walls] * some.size, [discs] * some.size)
        assert np.array_equal(ub, ub_ref, equal_nan=True) and np.array_equal(lb, lb_ref, equal_nan=True)
        assert np.array_equal(flag == 1, blocked) and np.all(flag != 2)
        assert not np.array_equal(ub, _rows_W("sim")[0][::3], equal_nan=True)        # the discs mattered


def _sensing_fleet(track, B, seed):
    """B poses near the walls of world W (two in three) or on the centre line, any heading; per-car discs and walls: car b
    carries W's walls b % 9 .. (a rotating subset, none for some) and b % 5 seeded discs"""
    g1, grid, origin, res = _g1(track)
    rng = np.random.default_rng(seed)
    m = Map.from_grid(grid, origin, res)
    wW = m.boundary_walls(_world_W(track))
    wp = rng.integers(0, g1["x"].size, B)
    poses = np.stack([g1["x"][wp], g1["y"][wp], g1["psi"][wp] + rng.uniform(-3, 3, B)], 1)
    for b in range(B):
        if b % 3:
            w = wW[rng.integers(0, len(wW))]
            t = rng.uniform(0, 1)
            poses[b, 0] = origin[0] + (w[0] + t * (w[2] - w[0]) + 0.5 + rng.uniform(-8, 8)) * res
            poses[b, 1] = origin[1] + (w[1] + t * (w[3] - w[1]) + 0.5 + rng.uniform(-8, 8)) * res
    walls = [wW[np.arange(b % 9, len(wW))] if b % 9 < len(wW) else np.zeros((0, 4), np.int32) for b in range(B)]
    walls[1] = np.concatenate([wW, wW])                                               # 16 walls: the cap
    discs = [_seeded_discs(track, b % 5, seed + b) for b in range(B)]
    return grid, origin, res, poses, discs, walls


@pytest.mark.parametrize("track", ["sim", "real"])
def test_twin_lidar_and_footprint_with_walls_equal_the_baked_grid(track, twin, old_twins):
    lid, fpl = old_twins
    B, nb = 48, 61
    grid, origin, res, poses, discs, walls = _sensing_fleet(track, B, 520)
    H, W = grid.shape
    angles = np.linspace(-np.pi / 2, np.pi / 2, nb)
    rng_m = 60 * res
    car = CARS[track]
    off, flat = _csr(discs, 3)
    woff, wflat = _csr(walls, 4)
    r_w, con_w, clr_w = np.zeros((B, nb)), np.zeros(B, np.int32), np.zeros(B)
    assert twin.wall_emu_scan(H, W, _b(grid), origin[0], origin[1], res, B, _d(poses), _i(off), _i(flat), _i(woff), _i(wflat), nb,
                              _d(angles), rng_m, _d(r_w)) == 0
    assert twin.wall_emu_audit(H, W, _b(grid), origin[0], origin[1], res, B, _d(poses), _i(off), _i(flat), _i(woff), _i(wflat), car[0],
                               car[1], car[2], _i(con_w), _d(clr_w)) == 0
    seen_l = seen_f = 0
    for b in range(B):                                                                # one baked grid per car
        baked = _bake(grid, discs[b], walls[b])
        r, con, clr = np.zeros((1, nb)), np.zeros(1, np.int32), np.zeros(1)
        p = np.ascontiguousarray(poses[b:b + 1])
        assert lid.lid_emu_scan(H, W, _b(baked), origin[0], origin[1], res, 1, _d(p), None, None, nb, _d(angles), rng_m, _d(r), None, None) == 0
        assert fpl.fp_emu_audit(H, W, _b(baked), origin[0], origin[1], res, 1, _d(p), None, None, car[0], car[1], car[2], _i(con), _d(clr)) == 0
        assert np.array_equal(r[0], r_w[b]) and con[0] == con_w[b] and clr[0] == clr_w[b], b
        only_discs = _bake(grid, discs[b])
        lid.lid_emu_scan(H, W, _b(only_discs), origin[0], origin[1], res, 1, _d(p), None, None, nb, _d(angles), rng_m, _d(r), None, None)
        fpl.fp_emu_audit(H, W, _b(only_discs), origin[0], origin[1], res, 1, _d(p), None, None, car[0], car[1], car[2], _i(con), _d(clr))
        seen_l += not np.array_equal(r[0], r_w[b])
        seen_f += clr[0] != clr_w[b]
    print("%s: walls change %d scans and %d clearances of %d, %d contacts" % (track, seen_l, seen_f, B, con_w.sum()))
    assert seen_l >= 10 and seen_f >= 5 and con_w.sum() >= 1


def test_set_walls_validation_without_device(twin, built_library):
    lib = mpmpc.load_library(built_library)
    off, w = np.array([0, 1], np.int32), np.array([[50, 50, 60, 70]], np.int32)
    assert lib.mpmpc_rollout_set_walls(None, 1, _i(off), _i(w)) == E_ARG              # no handle
    grid = np.ones((20, 30), np.int8)
    out = np.zeros_like(grid)
    for bad in ([0, 5, 10, 10], [5, 0, 10, 10], [5, 5, 29, 10], [5, 5, 10, 19], [-3, 5, 10, 10]):      # before any device call
        assert lib.mpmpc_world_grid(0, 20, 30, _b(grid), 0.0, 0.0, 0.1, 0, None, 1, _i(np.array([bad], np.int32)), _b(out)) == E_ARG, bad
    assert lib.mpmpc_world_grid(0, 20, 30, _b(grid), 0.0, 0.0, 0.1, 0, None, 17, _i(np.tile(np.array([[5, 5, 9, 9]], np.int32), (17, 1))),
                                _b(out)) == E_ARG
    pose, rr = np.zeros((1, 3)), np.zeros((1, 3))
    ang = np.array([-0.1, 0.0, 0.1])
    assert lib.mpmpc_lidar_scan_world(0, 20, 30, _b(grid), 0.0, 0.0, 0.1, 1, _d(pose), None, None, _i(np.array([0, 1], np.int32)),
                                      _i(np.array([[5, 5, 29, 10]], np.int32)), 3, _d(ang), 1.0, _d(rr)) == E_ARG
    con, clr = np.zeros(1, np.int32), np.zeros(1)
    assert lib.mpmpc_footprint_audit_world(0, 20, 30, _b(grid), 0.0, 0.0, 0.1, 1, _d(pose), None, None, _i(np.array([1, 1], np.int32)),
                                           _i(np.array([[5, 5, 9, 9]], np.int32)), 0.3, 0.2, 0.3, _i(con), _d(clr)) == E_ARG
    W, H = 500, 400

    def check(off, walls, B=1, max_batch=8, built=1, other_B=0):
        return twin.wall_emu_check(B, max_batch, _i(np.asarray(off, np.int32)),
                                   _i(np.ascontiguousarray(np.asarray(walls, np.int32).reshape(-1, 4))), built, W, H, other_B)
    assert check([0, 1], [[50, 50, 60, 70]]) == 0
    assert check([0, 1], [[50, 50, 50, 50]]) == 0                                      # a wall of one cell
    assert check([0, 0, 0], np.zeros((0, 4)), B=2) == 0                               # cars without walls
    assert check([0, 2], [[1, 1, W - 2, H - 2], [W - 2, 1, 1, H - 2]]) == 0           # the outermost end points allowed
    for bad in ([0, 50, 60, 70], [50, 0, 60, 70], [50, 50, W - 1, 70], [50, 50, 60, H - 1], [50, 50, -1, 70], [W, 50, 60, 70]):
        assert check([0, 1], [bad]) == -1, bad
    assert check([1, 1], [[50, 50, 60, 70]]) == -1                                     # offsets[0] != 0
    assert check([0, 2, 1], [[50, 50, 60, 70]] * 2, B=2) == -1                         # decreasing
    assert check([0, 16], [[50, 50, 60, 70]] * 16) == 0
    assert check([0, 17], [[50, 50, 60, 70]] * 17) == -1                               # more than COR_MAX_WALLS per car
    assert check([0, 1], [[50, 50, 60, 70]], B=0) == -1 and check([0, 1, 1], [[50, 50, 60, 70]], B=2, max_batch=1) == -1
    assert check([0, 1], [[50, 50, 60, 70]], built=0) == -3                            # no build of the current map: E_STATE
    assert check([0, 1], [[50, 50, 60, 70]], other_B=1) == 0
    assert check([0, 1], [[50, 50, 60, 70]], other_B=2) == -3                          # another B than the settings in force


# ------------------------------------------------------------------------------------------------------------ GPU
def _handle(track, B, warm=False):
    tr = scenarios.sim_track() if track == "sim" else scenarios.real_track()
    g1, grid, origin, res = _g1(track)
    h = mpmpc.Handle(T.stock_config(N, max_batch=B, track=None if track == "sim" else tr), mpmpc.default_settings())
    h.set_path(tr.kappa, tr.v_ref, tr.ds_next)
    h.set_map(grid, origin, res)
    h.set_path_geometry(g1["x"], g1["y"], g1["psi"], g1["border_ub"], g1["border_lb"])
    h.rollout_warm_start(warm)
    sm = _sm(track)
    h.build_corridor(N, 2 * sm, sm, want_tables=False)
    return h


def _at_waypoints(track, starts):
    """-> cum, s, poses of cars that stand at the waypoints `starts`"""
    g1 = _g1(track)[0]
    cum = np.cumsum(g1["segment_lengths"])
    poses = np.stack([g1["x"][starts], g1["y"][starts], g1["psi"][starts]], 1)
    s0 = cum[starts].copy()
    s0[starts == g1["x"].size - 1] = np.nextafter(cum[-1], 0.0)      # (s = length: the lap is over)
    return cum, s0, poses


@pytest.mark.gpu
@pytest.mark.parametrize("track", ["sim", "real"])
def test_device_world_grid_equals_the_host_map(track):
    g1, grid, origin, res = _g1(track)
    m = Map.from_grid(grid, origin, res)
    walls = np.concatenate([_seeded_walls(track, 8, 530), m.boundary_walls(_world_W(track))])
    discs = _seeded_discs(track, 64, 531)
    got = mpmpc.world_grid(grid, origin, res, discs, walls)
    assert got.dtype == np.int8 and np.array_equal(got, _bake(grid, discs, walls))
    assert np.array_equal(mpmpc.world_grid(grid, origin, res), grid)
    assert np.array_equal(mpmpc.world_grid(grid, origin, res, walls=m.boundary_walls(_world_W(track))), _host_map(track, _world_W(track)).data)
    with pytest.raises(mpmpc.MpmpcError, match="end point"):
        mpmpc.world_grid(grid, origin, res, walls=[[0, 5, 9, 9]])


@pytest.mark.gpu
@pytest.mark.parametrize("track", ["sim", "real"])
def test_device_rows_in_world_W_equal_the_host_rows(track):
    ub_ref, lb_ref, blocked = _rows_W(track)
    all_starts = _starts(track)
    starts = np.union1d(all_starts[::4], all_starts[blocked])                          # every 4th, and the blocked row
    walls = Map.from_grid(*_g1(track)[1:]).boundary_walls(_world_W(track))
    seen_blocked = 0
    for lo in range(0, starts.size, 64):
        st_wp = starts[lo:lo + 64]
        B = st_wp.size
        h = _handle(track, B)
        cum, s0, poses = _at_waypoints(track, st_wp)
        h.rollout_set_walls([walls] * B)
        h.rollout_init(TS, cum, s0, poses)
        h.rollout_step(1)
        ub, lb = h.rollout_corridor()
        st = h.rollout_state()
        h.close()
        assert np.array_equal(st["wp_id"], st_wp)
        assert np.array_equal(ub, ub_ref[st_wp], equal_nan=True) and np.array_equal(lb, lb_ref[st_wp], equal_nan=True)
        assert np.array_equal(st["alive"] == -3, blocked[st_wp])
        assert np.array_equal(st["pose"][blocked[st_wp]], poses[blocked[st_wp]])       # a blocked car is not driven
        seen_blocked += blocked[st_wp].sum()
    assert seen_blocked >= 1


def _four_worlds(track):
    """four wall worlds without a barrier (the shared-table rollout has no verdict -3): cells [k, 4] each"""
    gates = _gates(track)[0]
    g1 = _g1(track)[0]
    flipped = []
    for k, i in enumerate(_gates(track)[2]):
        a, b = (g1["border_lb"][i], g1["border_ub"][i]) if k % 2 == 0 else (g1["border_ub"][i], g1["border_lb"][i])
        flipped.append((tuple(a), tuple(a + 0.5 * (b - a))))
    m = Map.from_grid(*_g1(track)[1:])
    return [m.boundary_walls(w) for w in (gates, flipped, gates[::2] + flipped[1::2], gates[:3])]


def _fleet_starts(track, B, seed):
    """B cars a few waypoints in front of gates, headings slightly off"""
    idx = _gates(track)[2]
    rng = np.random.default_rng(seed)
    starts = np.array([idx[b % len(idx)] - 2 - (b // len(idx)) % 9 for b in range(B)])
    cum, s0, poses = _at_waypoints(track, starts)
    poses[:, 2] += rng.uniform(-0.05, 0.05, B)
    return cum, s0, poses


def _run(h, cum, s0, poses, steps, walls=None, discs=None, movers=None, traffic=None, rows=True):
    h.rollout_set_obstacles(None)
    h.rollout_set_movers(None)
    h.rollout_set_traffic(None)
    h.rollout_set_walls(None)
    if walls is not None:
        h.rollout_set_walls(walls)
    if discs is not None:
        h.rollout_set_obstacles(discs)
    if movers is not None:
        h.rollout_set_movers(movers)
    if traffic is not None:
        h.rollout_set_traffic(*traffic)
    h.rollout_init(TS, cum, s0, poses)
    h.rollout_step(steps)
    st = h.rollout_state()
    if rows:
        st["ub"], st["lb"] = h.rollout_corridor()
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["cold", "warm", "mixed"])
def test_fleet_of_wall_worlds_equals_rollouts_on_baked_grids(case):
    """4 wall worlds x 8 cars in ONE rollout against four rollouts whose map is the baked grid: the shared table (cold, warm),
    or - mixed - per-car discs, a mover and traffic on the baked grid"""
    track, B, steps = "sim", 32, 10
    g1, grid, origin, res = _g1(track)
    sm = _sm(track)
    worlds = _four_worlds(track)
    wid = np.arange(B) % 4
    cum, s0, poses = _fleet_starts(track, B, 540)
    h = _handle(track, B, warm=case == "warm")
    extra = {}
    if case == "mixed":
        gx, gy = g1["x"], g1["y"]
        extra = dict(discs=[np.array([[int((gx[(15 + 28 * (b % 7) + 9) % 200] - origin[0]) / res), int((gy[(15 + 28 * (b % 7) + 9) % 200] - origin[1]) / res), 6]], np.int32)
                            if b % 2 else np.zeros((0, 3), np.int32) for b in range(B)],
                     movers=[np.array([[1, 5, s0[b] + 0.6, 0.03, 0.01, 0.0]]) if b % 3 == 0 else np.zeros((0, 6)) for b in range(B)],
                     traffic=(wid, np.full(B, 4), 2, 80))
    ref = {}
    for w in range(4):
        h.set_map(_bake(grid, walls=worlds[w]), origin, res)
        ub_tab, lb_tab, bad = h.build_corridor(N, 2 * sm, sm)
        assert bad == 0
        st = _run(h, cum, s0, poses, steps, rows=bool(extra), **extra)
        if not extra:
            st["ub"], st["lb"] = ub_tab[st["wp_id"]], lb_tab[st["wp_id"]]
        for k in st:
            ref.setdefault(k, np.zeros_like(st[k]))[wid == w] = st[k][wid == w]
    h.set_map(grid, origin, res)
    h.build_corridor(N, 2 * sm, sm, want_tables=False)
    got = _run(h, cum, s0, poses, steps, walls=[worlds[w] for w in wid], **extra)
    bare = _run(h, cum, s0, poses, steps, rows=False)
    h.close()
    for k in KEYS + ("ub", "lb"):
        assert np.array_equal(got[k], ref[k], equal_nan=True), k
    assert (got["alive"] == 1).sum() >= B // 2
    assert np.sum(np.any(got["pose"] != bare["pose"], 1)) >= B // 2                    # the walls mattered


@pytest.mark.gpu
@pytest.mark.parametrize("track", ["sim", "real"])
def test_device_lidar_and_footprint_with_walls_equal_the_baked_grid(track):
    B, nb = 48, 61
    grid, origin, res, poses, discs, walls = _sensing_fleet(track, B, 520)
    angles = np.linspace(-np.pi / 2, np.pi / 2, nb)
    rng_m = 60 * res
    car = CARS[track]
    r_w = mpmpc.lidar_scan(grid, origin, res, poses, angles, rng_m, discs, walls=walls)
    con_w, clr_w = mpmpc.footprint_audit(grid, origin, res, poses, *car, discs, walls=walls)
    seen_l = seen_f = 0
    for b in range(B):                                                                # the old entry points, one baked grid per car
        baked = _bake(grid, discs[b], walls[b])
        assert np.array_equal(mpmpc.lidar_scan(baked, origin, res, poses[b:b + 1], angles, rng_m)[0], r_w[b]), b
        con, clr = mpmpc.footprint_audit(baked, origin, res, poses[b:b + 1], *car)
        assert con[0] == con_w[b] and clr[0] == clr_w[b], b
    r_d = mpmpc.lidar_scan(grid, origin, res, poses, angles, rng_m, discs)
    con_d, clr_d = mpmpc.footprint_audit(grid, origin, res, poses, *car, discs)
    seen_l, seen_f = np.sum(np.any(r_d != r_w, 1)), np.sum(clr_d != clr_w)
    print("%s: walls change %d scans and %d clearances of %d, %d contacts" % (track, seen_l, seen_f, B, con_w.sum()))
    assert seen_l >= 10 and seen_f >= 5 and con_w.sum() >= 1
    # empty wall lists are the old entry points
    none = [np.zeros((0, 4), np.int32)] * B
    assert np.array_equal(mpmpc.lidar_scan(grid, origin, res, poses, angles, rng_m, discs, walls=none), r_d)
    assert np.array_equal(mpmpc.footprint_audit(grid, origin, res, poses, *car, discs, walls=none)[1], clr_d)


@pytest.mark.gpu
def test_rollout_scan_and_audit_see_the_walls():
    """world W for every car, and for car 0 a wall of its own through its start pose: in mode 2 it ends there with -5"""
    track, B, nb = "sim", 32, 61
    g1, grid, origin, res = _g1(track)
    car = CARS[track]
    m = Map.from_grid(grid, origin, res)
    wW = m.boundary_walls(_world_W(track))
    cum, s0, poses = _fleet_starts(track, B, 550)
    c0 = m.w2m(poses[0, 0], poses[0, 1])
    walls = [wW] * B
    walls[0] = np.concatenate([wW[:3], np.array([[c0[0] - 4, c0[1] - 4, c0[0] + 4, c0[1] + 4]], np.int32)])
    angles = np.linspace(-np.pi / 2, np.pi / 2, nb)
    h = _handle(track, B)
    h.rollout_set_audit(2, *car)
    h.rollout_set_walls(walls)
    h.rollout_init(TS, cum, s0, poses)
    before = poses
    for k in range(4):
        h.rollout_step(1)
        st, aud = h.rollout_state(), h.rollout_audit()
        run = (st["alive"] == 1) | ((st["alive"] == -5) & (aud["first_contact"] == k))      # audited in step k
        con, clr = mpmpc.footprint_audit(grid, origin, res, before, *car, walls=walls)
        assert np.array_equal(aud["last_contact"][run], con[run]) and np.array_equal(aud["last_clearance"][run], clr[run]), k
        before = st["pose"]
    assert st["alive"][0] == -5 and aud["first_contact"][0] == 0 and aud["contact_steps"][0] == 1
    assert np.array_equal(st["pose"][0], poses[0])                                     # it was not driven
    scan = h.rollout_scan(angles, 60 * res)
    assert np.array_equal(scan, mpmpc.lidar_scan(grid, origin, res, st["pose"], angles, 60 * res, walls=walls))
    assert np.sum(np.any(scan != mpmpc.lidar_scan(grid, origin, res, st["pose"], angles, 60 * res), 1)) >= B // 4
    with pytest.raises(mpmpc.MpmpcError):
        h.rollout_obstacles()                                                          # walls only: there are no disc lists
    h.rollout_set_walls(walls)
    with pytest.raises(mpmpc.MpmpcError, match="set anew"):
        h.rollout_scan(angles, 60 * res)                                               # the worlds are those of a step
    h.close()


@pytest.mark.gpu
def test_gate_removed_between_steps_and_state_errors():
    track, B = "sim", 16
    g1, grid, origin, res = _g1(track)
    gates, barrier, idx, _ = _gates(track)
    m = Map.from_grid(grid, origin, res)
    starts = np.array([idx[1] - 3 - (b % 8) for b in range(B)])                        # in front of the second gate
    cum, s0, poses = _at_waypoints(track, starts)
    with_gate, without = gates, gates[:1] + gates[2:]
    h = _handle(track, B)
    h.rollout_set_walls([m.boundary_walls(with_gate)] * B)
    h.rollout_init(TS, cum, s0, poses)
    h.rollout_step(3)
    st = h.rollout_state()
    ub, lb = h.rollout_corridor()
    want = _host_rows(track, with_gate, st["wp_id"])
    assert np.array_equal(ub, want[0]) and np.array_equal(lb, want[1])
    h.rollout_set_walls([m.boundary_walls(without)] * B)
    for _ in range(2):                                                                 # from the next step on
        h.rollout_step(1)
        st2 = h.rollout_state()
        ub2, lb2 = h.rollout_corridor()
        free = _host_rows(track, without, st2["wp_id"])
        assert np.array_equal(ub2, free[0]) and np.array_equal(lb2, free[1])
        gated = _host_rows(track, with_gate, st2["wp_id"])
        assert np.sum(np.any(lb2 != gated[1], 1)) >= B // 2                            # the gate (from the lower border) had mattered
    assert np.all(st2["alive"] == 1) and np.all(st2["s"] > st["s"])                    # the state was kept
    # a refused call leaves the setting as it was
    with pytest.raises(mpmpc.MpmpcError, match="end point"):
        h.rollout_set_walls([np.array([[0, 5, 9, 9]], np.int32)] * B)
    with pytest.raises(mpmpc.MpmpcError, match="16 walls"):
        h.rollout_set_walls([np.tile(np.array([[5, 5, 9, 9]], np.int32), (17, 1))] * B)
    with pytest.raises(mpmpc.MpmpcError, match="same number of cars|another number of cars"):
        h.rollout_set_obstacles([np.zeros((0, 3), np.int32)] * (B - 1))
    h.rollout_step(1)
    st3 = h.rollout_state()
    ub3, lb3 = h.rollout_corridor()
    free = _host_rows(track, without, st3["wp_id"])
    assert np.array_equal(ub3, free[0]) and np.array_equal(lb3, free[1])
    # void after a change of the map
    h.set_map(grid, origin, res)
    with pytest.raises(mpmpc.MpmpcError, match="build_corridor"):
        h.rollout_set_walls([m.boundary_walls(without)] * B)
    with pytest.raises(mpmpc.MpmpcError):
        h.rollout_step(1)
    h.close()


@pytest.mark.gpu
def test_no_walls_and_empty_lists_are_the_rollout_without_the_call():
    track, B, steps = "sim", 32, 10
    cum, s0, poses = _fleet_starts(track, B, 560)
    h = _handle(track, B)
    h.rollout_init(TS, cum, s0, poses)                                                # no call at all
    h.rollout_step(steps)
    a = h.rollout_state()
    h.rollout_set_walls(None)
    h.rollout_init(TS, cum, s0, poses)
    h.rollout_step(steps)
    b = h.rollout_state()
    c = _run(h, cum, s0, poses, steps, walls=[np.zeros((0, 4), np.int32)] * B)
    # ... and beside discs: empty wall lists change nothing either
    discs = [_seeded_discs(track, 3, 561 + i) for i in range(B)]
    d = _run(h, cum, s0, poses, steps, discs=discs)
    e = _run(h, cum, s0, poses, steps, discs=discs, walls=[np.zeros((0, 4), np.int32)] * B)
    h.close()
    for k in KEYS:
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]), k
        assert np.array_equal(d[k], e[k]), k
    assert np.array_equal(d["ub"], e["ub"], equal_nan=True) and np.array_equal(d["lb"], e["lb"], equal_nan=True)


@pytest.mark.gpu
def test_six_steps_at_once_equal_six_single_steps_with_walls():
    track, B = "sim", 32
    worlds = _four_worlds(track)
    walls = [worlds[b % 4] for b in range(B)]
    cum, s0, poses = _fleet_starts(track, B, 570)
    h = _handle(track, B)
    a = _run(h, cum, s0, poses, 6, walls=walls)
    h.rollout_set_walls(walls)
    h.rollout_init(TS, cum, s0, poses)
    for _ in range(6):
        h.rollout_step(1)
    b = h.rollout_state()
    b["ub"], b["lb"] = h.rollout_corridor()
    h.close()
    for k in KEYS + ("ub", "lb"):
        assert np.array_equal(a[k], b[k], equal_nan=True), k


@pytest.mark.gpu
def test_batchmpc_rollout_takes_walls():
    """BatchMPC.rollout(..., walls=...): boundaries in world coordinates per car; a later rollout is wall-free again"""
    from scipy import sparse
    from MPC import BatchMPC
    m, rp, car = T.build_world(obstacles=False)
    Q, R, QN = sparse.diags([1.0, 0.0, 0.0]), sparse.diags([0.5, 0.0]), sparse.diags([1.0, 0.0, 0.0])
    ic = {'umin': np.array([0.0, -np.tan(0.66) / car.length]), 'umax': np.array([1.0, np.tan(0.66) / car.length])}
    sc = {'xmin': np.array([-np.inf] * 3), 'xmax': np.array([np.inf] * 3)}
    gates, _, idx, _ = _gates("sim")
    B = 4
    starts = np.array([idx[0] - 4, idx[1] - 4, idx[2] - 4, idx[3] - 4])
    bm = BatchMPC(car, N, Q, R, QN, sc, ic, 4.0, max_batch=B, corridor="device")
    cum = np.cumsum(rp.segment_lengths)
    poses = np.array([[rp.waypoints[w].x, rp.waypoints[w].y, rp.waypoints[w].psi] for w in starts])
    plain = bm.rollout(cum[starts], poses, 3)
    out = bm.rollout(cum[starts], poses, 3, walls=[gates, gates, gates, []])
    ub, lb = bm.handle.rollout_corridor()
    again = bm.rollout(cum[starts], poses, 3)
    bm.close()
    assert all(np.array_equal(again[k], plain[k]) for k in plain)
    assert np.all(out["alive"] == 1)
    sm = car.safety_margin
    free = [rp.update_path_constraints(int(w) + 1, N, 2 * sm, sm)[:2] for w in out["wp_id"]]
    m.add_boundary(gates)                                                              # (the host map, after the device runs)
    gated = [rp.update_path_constraints(int(w) + 1, N, 2 * sm, sm)[:2] for w in out["wp_id"]]
    for b in range(B):
        want = gated[b] if b < 3 else free[b]
        assert np.array_equal(ub[b], want[0]) and np.array_equal(lb[b], want[1]), b
        assert b == 3 or not (np.array_equal(gated[b][0], free[b][0]) and np.array_equal(gated[b][1], free[b][1])), b
