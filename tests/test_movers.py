"""Moving obstacles in the device rollout (K0m, mpmpc_rollout_set_movers): per-car movers whose discs are a closed-form
function of the rollout step index, advanced on the device between localise and K0c.

CPU: the host twin of K0m (tests/emul_movers, the same obstacle_motion_core.hpp) against a restatement of the motion law
written here from the header's stated operation order, against Map.obstacle_discs and against the product's numpy
evaluation; the argument checks.  GPU: one multi-step call against the step-by-step loop that re-uploads every car's discs
(what a moving obstacle cost before), frozen movers against static discs, step0 / resuming, mpmpc_rollout_obstacles, the
recorder's rows."""
import ctypes as C
import math
from bisect import bisect_right

import numpy as np
import pytest

import mpmpc
import mpmpc_testlib as T
import scenarios
import twins
from map import Map, Obstacle

lp = C.POINTER(C.c_int64)
E_ARG, E_STATE = -1, -3
TS = 0.05
KEYS = ("s", "pose", "cc", "wp_id", "status", "counter", "alive")


_d, _i, _g1, _sm = T._d, T._i, T.g1_world, T.safety_margin


@pytest.fixture(scope="module")
def twin():
    """The CPU twin of K0m (tests/emul_movers)."""
    return twins.movers()


@pytest.fixture(scope="module")
def car_twin():
    """The CPU twin of K0c (tests/emul_car), for the step-0 condition on the fleets."""
    return twins.car()


# ------------------------------------------------------------------------------ the motion law, restated from the header
class World:
    """what a mover's disc depends on besides its own row: the grid's frame and the path's tables"""

    def __init__(self, origin, res, width, height, cum, x, y, psi, circular):
        self.ox, self.oy, self.res, self.W, self.H = float(origin[0]), float(origin[1]), float(res), int(width), int(height)
        self.cum, self.x, self.y = ([float(v) for v in a] for a in (cum, x, y))
        self.sin = [math.sin(float(a)) for a in psi]        # libm: the values of K0's per-waypoint table
        self.cos = [math.cos(float(a)) for a in psi]
        self.psi = np.ascontiguousarray(psi, float)
        self.circular = bool(circular)


def _world(track):
    g1, grid, origin, res = _g1(track)
    return World(origin, res, grid.shape[1], grid.shape[0], np.cumsum(g1["segment_lengths"]), g1["x"], g1["y"], g1["psi"],
                 track == "sim")


def _disc(row, j, w):
    """(cx, cy, r) of the mover `row` = (kind, r, p0, p1, p2, p3) at j = k - step0, in obstacle_motion_core.hpp's order"""
    kind, r = int(row[0]), int(row[1])
    p0, p1, p2, p3 = (float(v) for v in row[2:6])
    j = float(j)
    absent = (0, 0, 0)
    if kind == 0:
        x = p0 + j * p2
        y = p1 + j * p3
    else:
        s = p0 + j * p2
        L = w.cum[-1]
        if not math.isfinite(s) or not L > 0.0:
            return absent
        if w.circular:
            s = s - L * math.floor(s / L)
            if not (0.0 <= s < L):
                s = 0.0
        elif not (0.0 <= s < L):
            return absent
        i = min(max(bisect_right(w.cum, s) - 1, 0), len(w.cum) - 2)
        den = w.cum[i + 1] - w.cum[i]
        f = (s - w.cum[i]) / den if den > 0.0 else 0.0
        x = (w.x[i] + f * (w.x[i + 1] - w.x[i])) - p1 * w.sin[i]
        y = (w.y[i] + f * (w.y[i + 1] - w.y[i])) + p1 * w.cos[i]
    vx, vy = (x - w.ox) / w.res, (y - w.oy) / w.res
    if not (math.isfinite(vx) and math.isfinite(vy)):
        return absent
    cx, cy = math.floor(vx), math.floor(vy)
    if abs(cx) > 2 ** 30 or abs(cy) > 2 ** 30:
        return absent
    if cx - r < 0 or cy - r < 0 or cx + r > w.W or cy + r > w.H:
        return absent
    return (cx, cy, r)


def _np_discs(rows, j, w):
    rows = np.asarray(rows, float).reshape(-1, 6)
    js = np.broadcast_to(np.asarray(j), (rows.shape[0],))
    return np.array([_disc(rows[q], js[q], w) for q in range(rows.shape[0])], np.int32).reshape(-1, 3)


def _twin_discs(twin, rows, k, step0, w):
    rows = np.asarray(rows, float).reshape(-1, 6)
    n = rows.shape[0]
    kind, rad = (np.ascontiguousarray(rows[:, c], np.int32) for c in (0, 1))
    prm = np.ascontiguousarray(rows[:, 2:], float)
    ks = np.ascontiguousarray(np.broadcast_to(np.asarray(k, np.int64), (n,)))
    out = np.full((n, 3), -7, np.int32)
    cum, x, y = (np.ascontiguousarray(a, float) for a in (w.cum, w.x, w.y))
    twin.mov_emu_discs(n, _i(kind), _i(rad), _d(prm), ks.ctypes.data_as(lp), int(step0), w.H, w.W, w.ox, w.oy, w.res, cum.size,
                       _d(cum), _d(x), _d(y), _d(w.psi), int(w.circular), _i(out))
    return out


def _with_empty_segment(w, at):
    """the same world with waypoint `at` doubled: cum[at] == cum[at + 1]"""
    dup = lambda a: list(a[:at + 1]) + [a[at]] + list(a[at + 1:])
    return World((w.ox, w.oy), w.res, w.W, w.H, dup(w.cum), dup(w.x), dup(w.y), dup(list(w.psi)), w.circular)


def _law_cases(track):
    """seeded (rows [n, 6], k [n], step0, world, tag [n]) groups that cover the law's branches on one track"""
    w = _world(track)
    rng = np.random.default_rng(101 if track == "sim" else 102)
    L, span_x, span_y = w.cum[-1], w.W * w.res, w.H * w.res
    rmax = 12 if track == "sim" else 5
    groups = []

    def group(rows, step0, world, tag):
        rows = np.asarray(rows, float).reshape(-1, 6)
        k = rng.integers(-50, 301, rows.shape[0]) + step0           # k - step0 in [-50, 300]
        groups.append((rows, k.astype(np.int64), step0, world, tag))

    # straight lines inside the map, and leaving it on each of the four sides
    inside = [(0, rng.integers(0, rmax), rng.uniform(w.ox + 0.3 * span_x, w.ox + 0.7 * span_x),
               rng.uniform(w.oy + 0.3 * span_y, w.oy + 0.7 * span_y), rng.uniform(-1, 1) * span_x / 2000,
               rng.uniform(-1, 1) * span_y / 2000) for _ in range(150)]
    group(inside, 0, w, "line")
    for side, (ux, uy) in (("left", (-1, 0)), ("right", (1, 0)), ("bottom", (0, -1)), ("top", (0, 1))):
        rows = [(0, rng.integers(1, rmax), w.ox + span_x / 2 + ux * 0.45 * span_x, w.oy + span_y / 2 + uy * 0.45 * span_y,
                 ux * rng.uniform(0.5, 2) * span_x / 1000 + rng.uniform(-1, 1) * span_x / 4000 * abs(uy),
                 uy * rng.uniform(0.5, 2) * span_y / 1000 + rng.uniform(-1, 1) * span_y / 4000 * abs(ux)) for _ in range(60)]
        group(rows, int(rng.integers(-30, 30)), w, "leaves_" + side)
    # along the path: e of both signs; laps (circular, several times round in either direction) / both ends (open)
    e_max = 0.12 if track == "sim" else 0.6
    slow = [(1, rng.integers(0, rmax), rng.uniform(0, L), rng.uniform(-e_max, e_max), rng.uniform(-1, 1) * L / 2000, 0.0)
            for _ in range(250)]
    group(slow, -20, w, "path")
    fast = [(1, rng.integers(0, rmax), rng.uniform(0, L), rng.uniform(-e_max, e_max), rng.choice([-1, 1]) * rng.uniform(0.01, 0.03) * L,
             0.0) for _ in range(250)]
    group(fast, 7, w, "laps" if track == "sim" else "ends")
    # an empty segment (a doubled waypoint), movers spread over it and some exactly on it
    at = 40
    we = _with_empty_segment(w, at)
    rows = [(1, rng.integers(0, rmax), we.cum[at] + rng.uniform(-0.02, 0.02) * L, rng.uniform(-e_max, e_max),
             rng.uniform(-1, 1) * L / 5000, 0.0) for _ in range(120)]
    rows += [(1, 3, we.cum[at], e, 0.0, 0.0) for e in (-e_max, 0.0, e_max)]
    group(rows, 0, we, "empty_segment")
    return groups


# ------------------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("track", ["sim", "real"])
def test_twin_equals_the_restated_law_bit_exact(track, twin):
    n = 0
    seen = {}
    for rows, k, step0, w, tag in _law_cases(track):
        got = _twin_discs(twin, rows, k, step0, w)
        want = _np_discs(rows, k - step0, w)
        assert np.array_equal(got, want), tag
        absent = np.all(want == 0, 1)
        seen[tag] = (int(absent.sum()), int((~absent).sum()))
        n += rows.shape[0]
        if tag in ("path", "laps", "ends", "empty_segment"):
            e = rows[:, 3]
            assert (e > 0).any() and (e < 0).any()
        if tag == "laps":
            s = rows[:, 2] + (k - step0) * rows[:, 4]
            assert (s > 3 * w.cum[-1]).any() and (s < -0.5 * w.cum[-1]).any()        # several times round, and backwards
        if tag == "ends":
            s = rows[:, 2] + (k - step0) * rows[:, 4]
            assert (s < 0).sum() >= 10 and (s >= w.cum[-1]).sum() >= 10
            assert np.all(absent[(s < 0) | (s >= w.cum[-1])])
    assert n >= 1000                                       # (two tracks: about 2 000 movers x steps)
    for side in ("left", "right", "bottom", "top"):
        assert seen["leaves_" + side][0] >= 5 and seen["leaves_" + side][1] >= 5, (side, seen)
    assert seen["line"][0] == 0 and seen["empty_segment"][1] >= 100
    if track == "sim":
        assert seen["path"][0] == 0 and seen["laps"][0] == 0          # a circular path has no end


@pytest.mark.parametrize("track", ["sim", "real"])
def test_line_mover_rasterises_like_add_obstacles(track, twin):
    """a kind-0 mover's disc at step k is Map.obstacle_discs of an Obstacle at (x0 + k dx, y0 + k dy)"""
    g1, grid, origin, res = _g1(track)
    w = _world(track)
    m = Map.from_grid(grid, origin, res)
    rng = np.random.default_rng(5 if track == "sim" else 6)
    sx, sy = w.W * res, w.H * res
    for _ in range(100):
        radius = rng.uniform(0.01, 0.09 if track == "sim" else 0.4)
        x0, y0 = rng.uniform(origin[0] + 0.3 * sx, origin[0] + 0.7 * sx), rng.uniform(origin[1] + 0.3 * sy, origin[1] + 0.7 * sy)
        dx, dy = rng.uniform(-1, 1) * sx / 2000, rng.uniform(-1, 1) * sy / 2000
        k = int(rng.integers(0, 300))
        r = int(np.ceil(radius / res))
        want = m.obstacle_discs([Obstacle(x0 + k * dx, y0 + k * dy, radius)])
        assert np.array_equal(_twin_discs(twin, [(0, r, x0, y0, dx, dy)], k, 0, w), want)


@pytest.mark.parametrize("track", ["sim", "real"])
def test_product_mover_discs_equal_the_twin(track, twin):
    import movers
    for rows, k, step0, w, tag in _law_cases(track):
        got = movers.mover_discs_rows(rows, k - step0, (w.ox, w.oy), w.res, w.W, w.H, cum=w.cum, x=w.x, y=w.y, psi=w.psi,
                                      circular=w.circular)
        assert got.dtype == np.int32 and np.array_equal(got, _twin_discs(twin, rows, k, step0, w)), tag
    # the Mover front end: speeds per second become displacements per step, the radius a cell count
    g1, grid, origin, res = _g1(track)
    m = Map.from_grid(grid, origin, res)
    w = _world(track)
    a, b = movers.Mover.line(origin[0] + 1.0, origin[1] + 1.2, 0.2, -0.1, 0.043), movers.Mover.along_path(1.5, -0.05, 0.4, 0.06)
    assert a.row(TS, res) == (0, int(np.ceil(0.043 / res)), origin[0] + 1.0, origin[1] + 1.2, 0.2 * TS, -0.1 * TS)
    assert b.row(TS, res) == (1, int(np.ceil(0.06 / res)), 1.5, -0.05, 0.4 * TS, 0.0)

    class Path:
        waypoints = [type("W", (), dict(x=x, y=y, psi=p)) for x, y, p in zip(w.x, w.y, w.psi)]
        segment_lengths = g1["segment_lengths"]
        circular = w.circular
    got = movers.mover_discs([a, b], 17, TS, m, Path, step0=-3)
    assert np.array_equal(got, _twin_discs(twin, [a.row(TS, res), b.row(TS, res)], 17, -3, w))


def test_set_movers_validation_without_device(twin, built_library):
    lib = mpmpc.load_library(built_library)
    assert lib.mpmpc_rollout_set_movers(None, 1, None, None, None, None, 0) == E_ARG
    assert lib.mpmpc_rollout_obstacles(None, 1, None, None) == E_ARG

    def check(off, rows, B=1, max_batch=8, built=1, static_B=0, static_off=None):
        rows = np.asarray(rows, float).reshape(-1, 6)
        kind, rad = (np.ascontiguousarray(rows[:, c], np.int32) for c in (0, 1))
        prm = np.ascontiguousarray(rows[:, 2:], float)
        so = None if static_off is None else np.asarray(static_off, np.int32)
        return twin.mov_emu_check(B, max_batch, _i(np.asarray(off, np.int32)), _i(kind), _i(rad), _d(prm), built, static_B, _i(so))
    line, path = (0, 3, 0.5, 0.5, 0.01, 0.0), (1, 3, 2.0, 0.05, 0.02, 0.0)
    assert check([0, 2], [line, path]) == 0
    assert check([0, 0, 0], np.zeros((0, 6)), B=2) == 0                          # cars without movers
    assert check([0, 1], [(2, 3, 0, 0, 0, 0)]) == E_ARG                          # unknown kind
    assert check([0, 1], [(-1, 3, 0, 0, 0, 0)]) == E_ARG
    assert check([0, 1], [(0, -1, 0.5, 0.5, 0.01, 0.0)]) == E_ARG                # negative radius
    for c in range(2, 6):                                                        # a parameter that is not finite
        for bad in (np.nan, np.inf, -np.inf):
            row = list(line)
            row[c] = bad
            assert check([0, 1], [row]) == E_ARG, (c, bad)
    assert check([0, 2, 1], [line, path], B=2) == E_ARG                          # offsets decrease
    assert check([1, 2], [line, path]) == E_ARG                                  # offsets[0] != 0
    assert check([0, 1], [line], B=0) == E_ARG and check([0, 1, 1], [line], B=2, max_batch=1) == E_ARG
    assert check([0, 1], [line], built=0) == E_STATE                             # no build of the current map
    # static discs + movers share the 64 entries of a car
    assert check([0, 64], [line] * 64) == 0 and check([0, 65], [line] * 65) == E_ARG
    assert check([0, 4], [line] * 4, static_B=1, static_off=[0, 60]) == 0
    assert check([0, 5], [line] * 5, static_B=1, static_off=[0, 60]) == E_ARG
    assert check([0, 1, 6], [line] * 6, B=2, static_B=2, static_off=[0, 60, 120]) == E_ARG     # the second car: 60 + 5
    assert check([0, 1, 5], [line] * 5, B=2, static_B=2, static_off=[0, 60, 120]) == 0
    assert check([0, 1], [line], B=1, static_B=2, static_off=[0, 1, 2]) == E_STATE               # settings for different B
    # ... and the same rule from the other setter's side
    comb = lambda sB, so, mB, mo: twin.mov_emu_check_combined(sB, _i(np.asarray(so, np.int32)), mB, _i(np.asarray(mo, np.int32)))
    assert comb(1, [0, 60], 1, [0, 4]) == 0 and comb(1, [0, 61], 1, [0, 4]) == E_ARG
    assert comb(2, [0, 1, 2], 1, [0, 4]) == E_STATE and comb(2, [0, 1, 2], 0, [0]) == 0
    # the layout K0c reads: per car the static discs, then a slot per mover
    off, dst = np.zeros(4, np.int32), np.zeros(4, np.int32)
    twin.mov_emu_combine(3, _i(np.array([0, 2, 2, 5], np.int32)), _i(np.array([0, 1, 3, 4], np.int32)), _i(off), _i(dst))
    assert off.tolist() == [0, 3, 5, 9] and dst.tolist() == [2, 3, 4, 8]
    twin.mov_emu_combine(3, None, _i(np.array([0, 1, 3, 4], np.int32)), _i(off), _i(dst))
    assert off.tolist() == [0, 1, 3, 4] and dst.tolist() == [0, 1, 2, 3]


def test_new_entry_points_are_exported(built_library):
    assert "mpmpc_rollout_set_movers" in mpmpc.EXPORTS and "mpmpc_rollout_obstacles" in mpmpc.EXPORTS
    lib = C.CDLL(built_library)
    assert hasattr(lib, "mpmpc_rollout_set_movers") and hasattr(lib, "mpmpc_rollout_obstacles")


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


def _twin_flags(car_twin, track, disc_lists, wp_ids, N):
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
    return flag


BASE = dict(sim=[(0.0, 0.0, 0.05), (-0.8, -0.5, 0.08), (-0.7, -1.5, 0.05), (-0.3, -1.0, 0.08), (0.27, -1.0, 0.05),
                 (0.78, -1.47, 0.05), (0.73, -0.9, 0.07), (1.2, 0.0, 0.08), (0.67, -0.05, 0.06)],
            real=[(-6.3, -11.1, 0.20), (-2.2, -6.8, 0.25), (2.0, -0.2, 0.25), (6.0, 5.0, 0.3), (7.42, 4.97, 0.3)])


class Fleet:
    """B cars on a track, each with 3 static discs (jittered obstacles of the reference's simulations), 2 movers along the
    path that start 5 .. 25 waypoints ahead of the car at a third to two thirds of v_ref with e inside the track, and 1
    straight-line mover that crosses the track ahead of the car during the run.  Cars whose step-0 row the K0c twin finds
    blocked are drawn again (same generator): a fleet that starts blocked compares nothing."""

    def __init__(self, track, N, B, steps, seed, car_twin, n_static=3):
        self.track, self.N, self.B, self.steps = track, N, B, steps
        g1, grid, origin, res = _g1(track)
        self.w = _world(track)
        tr = scenarios.sim_track() if track == "sim" else scenarios.real_track()
        self.cum = np.cumsum(g1["segment_lengths"])
        n_wp = g1["x"].size
        rng = np.random.default_rng(seed)
        hi = n_wp if track == "sim" else n_wp - N - steps // 2 - 5
        self.starts = rng.integers(0, hi, B)
        self.poses = np.stack([g1["x"][self.starts], g1["y"][self.starts], g1["psi"][self.starts]], 1)
        self.poses[:, 2] += rng.uniform(-0.05, 0.05, B)
        m = Map.from_grid(grid, origin, res)
        sim = track == "sim"
        jit, e_max, rr, d0 = (0.05, 0.08, (0.03, 0.05), 0.3) if sim else (0.2, 0.3, (0.15, 0.25), 1.5)

        def ahead(w0, a):
            return (w0 + a) % n_wp if sim else min(w0 + a, n_wp - 2)

        def draw(b):
            w0 = int(self.starts[b])
            pick = rng.choice(len(BASE[track]), n_static, replace=False)
            static = m.obstacle_discs([Obstacle(BASE[track][q][0] + rng.uniform(-jit, jit), BASE[track][q][1] + rng.uniform(-jit, jit),
                                                BASE[track][q][2] * rng.uniform(0.8, 1.2)) for q in pick])
            rows = []
            for _ in range(2):
                rows.append((1, int(np.ceil(rng.uniform(*rr) / res)), self.cum[ahead(w0, int(rng.integers(5, 26)))],
                             rng.uniform(-e_max, e_max), rng.uniform(1 / 3, 2 / 3) * tr.v_ref[w0] * TS, 0.0))
            wc = ahead(w0, int(rng.integers(10, 30)))
            nx, ny = -math.sin(g1["psi"][wc]), math.cos(g1["psi"][wc])
            side = rng.choice([-1.0, 1.0])
            rows.append((0, int(np.ceil(rng.uniform(*rr) / res)), g1["x"][wc] - side * d0 * nx, g1["y"][wc] - side * d0 * ny,
                         side * nx * 2 * d0 / steps, side * ny * 2 * d0 / steps))
            return static, np.array(rows, float)
        cars = [draw(b) for b in range(B)]
        for _ in range(20):
            flag = _twin_flags(car_twin, track, [np.concatenate([c[0], _np_discs(c[1], 0, self.w)]) for c in cars], self.starts, N)
            if not np.any(flag != 0):
                break
            for b in np.nonzero(flag != 0)[0]:
                cars[b] = draw(b)
        assert not np.any(flag != 0)          # no car's row is blocked (or overflows) at step 0
        self.static = [c[0] for c in cars]
        self.rows = [c[1] for c in cars]

    def discs_at(self, j, frozen=False):
        """per car: its static discs, then its movers' discs j steps after step0 (the restated law)"""
        return [np.concatenate([self.static[b], _np_discs(self.rows[b], 0 if frozen else j, self.w)]) for b in range(self.B)]

    def frozen_rows(self):
        out = []
        for r in self.rows:
            r = r.copy()
            r[:, 4] = 0.0
            r[r[:, 0] == 0, 5] = 0.0
            out.append(r)
        return out

    def init(self, h):
        h.rollout_init(TS, self.cum, self.cum[self.starts], self.poses)


def _enough_alive(st):
    assert np.isin(st["alive"], (0, 1)).sum() * 2 >= st["alive"].size, np.unique(st["alive"], return_counts=True)
    assert not np.any(st["alive"] == -4)


def _same(a, b, sel=slice(None)):
    for k in KEYS:
        assert np.array_equal(a[k][sel], b[k][sel]), k


SHAPES = dict(sim=(30, 256, 40, 61), real=(70, 64, 20, 62))      # N, B, steps, seed


@pytest.fixture(scope="module")
def runs(car_twin):
    """per track, computed once: A one call with movers; L the step-by-step loop on a second handle, with each step's rows,
    waypoints and discs; F the movers frozen, one call; S the frozen movers as static discs"""
    cache = {}

    def get(track):
        if track in cache:
            return cache[track]
        N, B, steps, seed = SHAPES[track]
        fl = Fleet(track, N, B, steps, seed, car_twin)
        h, tabs = _handle(track, N, B)
        out = dict(fleet=fl, tabs=tabs)
        h.rollout_set_obstacles(fl.static)
        h.rollout_set_movers(fl.rows)
        fl.init(h)
        h.rollout_step(steps)
        out["A"], out["A_rows"], out["A_discs"] = h.rollout_state(), h.rollout_corridor(), h.rollout_obstacles()
        h.rollout_set_movers(fl.frozen_rows())
        fl.init(h)
        h.rollout_step(steps)
        out["F"], out["F_rows"] = h.rollout_state(), h.rollout_corridor()
        h.rollout_set_movers(None)
        h.rollout_set_obstacles(fl.discs_at(0))
        fl.init(h)
        h.rollout_step(steps)
        out["S"], out["S_rows"] = h.rollout_state(), h.rollout_corridor()
        h.close()
        h2, _ = _handle(track, N, B)
        fl.init(h2)
        ubs, lbs, wps, alive = [], [], [], []
        for k in range(steps):
            h2.rollout_set_obstacles(fl.discs_at(k))
            h2.rollout_step(1)
            ub, lb = h2.rollout_corridor()
            st = h2.rollout_state()
            ubs.append(ub), lbs.append(lb), wps.append(st["wp_id"]), alive.append(st["alive"])
        out["L"], out["L_ub"], out["L_lb"], out["L_wp"], out["L_alive"] = st, np.array(ubs), np.array(lbs), np.array(wps), np.array(alive)
        h2.close()
        cache[track] = out
        return out
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("track", ["sim", "real"])
def test_one_call_equals_the_step_by_step_loop(track, runs):
    r = runs(track)
    _same(r["A"], r["L"])
    assert np.array_equal(r["A_rows"][0], r["L_ub"][-1], equal_nan=True) and np.array_equal(r["A_rows"][1], r["L_lb"][-1], equal_nan=True)
    _enough_alive(r["A"])


@pytest.mark.gpu
def test_the_movers_mattered(runs):
    r = runs("sim")
    assert (r["A"]["s"] != r["F"]["s"]).sum() * 4 >= r["A"]["s"].size
    # a car that stayed at its waypoint from one step to the next has the same base row at every column; its own row
    # changed all the same, because its movers went on
    ub, lb, wp, alive = r["L_ub"], r["L_lb"], r["L_wp"], r["L_alive"]
    ub_tab = r["tabs"][0]
    found = 0
    for k in range(ub.shape[0] - 1):
        stay = (wp[k] == wp[k + 1]) & (alive[k] == 1) & (alive[k + 1] == 1)
        base_same = np.all(ub_tab[wp[k]] == ub_tab[wp[k + 1]], 1)
        found += int((stay & base_same & np.any((ub[k] != ub[k + 1]) | (lb[k] != lb[k + 1]), 1)).sum())
    assert found >= 1


@pytest.mark.gpu
def test_frozen_movers_are_static_discs(runs):
    r = runs("sim")
    _same(r["F"], r["S"])
    assert np.array_equal(r["F_rows"][0], r["S_rows"][0], equal_nan=True) and np.array_equal(r["F_rows"][1], r["S_rows"][1], equal_nan=True)
    _enough_alive(r["F"])


@pytest.mark.gpu
def test_step0_resumes_a_run(runs):
    r = runs("sim")
    fl = r["fleet"]
    N, B, steps, _ = SHAPES["sim"]
    h, _ = _handle("sim", N, B)
    h.rollout_set_obstacles(fl.static)
    h.rollout_set_movers(fl.rows)
    fl.init(h)
    h.rollout_step(steps // 2)
    mid = h.rollout_state()
    h.rollout_init(TS, fl.cum, mid["s"], mid["pose"], cc0=mid["cc"])
    h.rollout_set_counters(np.minimum(mid["counter"], N - 2))
    h.rollout_set_movers(fl.rows, step0=-(steps // 2))
    h.rollout_step(steps - steps // 2)
    a = h.rollout_state()
    rows = h.rollout_corridor()
    h.close()
    live = mid["alive"] == 1
    assert live.sum() * 2 >= B
    _same(a, r["A"], live)
    assert np.array_equal(rows[0][live], r["A_rows"][0][live], equal_nan=True)
    assert np.array_equal(rows[1][live], r["A_rows"][1][live], equal_nan=True)
    _enough_alive(r["A"])


@pytest.mark.gpu
def test_rollout_obstacles_returns_the_discs_of_the_last_step(runs, car_twin):
    r = runs("sim")
    fl, steps = r["fleet"], SHAPES["sim"][2]
    want = fl.discs_at(steps - 1)
    assert len(r["A_discs"]) == fl.B
    for b in range(fl.B):
        assert r["A_discs"][b].dtype == np.int32 and np.array_equal(r["A_discs"][b], want[b]), b
    # a small fleet, one mover steered off the map: absent from the step on at which its square leaves the grid
    N, B = 30, 8
    small = Fleet("sim", N, B, 6, 63, car_twin)
    small.rows[2][2] = (0, 4, 1.3, -1.0, 0.06, 0.0)            # leaves the 2.5 m map at x = 1.5 within four steps
    h, _ = _handle("sim", N, B)
    with pytest.raises(mpmpc.MpmpcError):
        h.rollout_obstacles()                                  # no rollout yet
    h.rollout_set_obstacles(small.static)
    h.rollout_set_movers(small.rows)
    small.init(h)
    gone = []
    for k in range(6):
        h.rollout_step(1)
        got = h.rollout_obstacles()
        want = small.discs_at(k)
        for b in range(B):
            assert np.array_equal(got[b], want[b]), (k, b)
        gone.append(bool(np.all(got[2][-1] == 0)))
    assert gone[0] is False and gone[-1] is True
    h.rollout_set_movers(None)
    with pytest.raises(mpmpc.MpmpcError):
        h.rollout_obstacles()                                  # the lists were laid out anew since the last step
    h.close()


@pytest.mark.gpu
def test_no_movers_is_the_static_rollout_and_neither_is_the_shared_table(car_twin):
    N, B, steps = 30, 128, 20
    fl = Fleet("sim", N, B, steps, 64, car_twin)
    h, _ = _handle("sim", N, B)

    def run():
        fl.init(h)
        h.rollout_step(steps)
        return h.rollout_state()
    shared = run()                                             # nothing ever set: the shared table
    h.rollout_set_obstacles(fl.static)
    static = run()
    h.rollout_set_movers(fl.rows)
    moved = run()
    h.rollout_set_movers(None)
    _same(run(), static)
    assert not np.array_equal(moved["s"], static["s"])
    h.rollout_set_movers([np.zeros((0, 6))] * B)               # cars without movers
    _same(run(), static)
    h.rollout_set_movers(fl.rows)
    h.rollout_set_obstacles(None)
    h.rollout_set_movers(None)
    _same(run(), shared)
    with pytest.raises(mpmpc.MpmpcError):
        h.rollout_corridor()                                   # that step built no per-car rows
    h.rollout_set_movers([np.zeros((0, 6))] * B)               # per-car rows, no discs at all: the table's rows
    _same(run(), shared)
    # refusals through the C ABI; a refused call leaves the setting in force
    h.rollout_set_obstacles([np.tile(d[:1], (60, 1)) for d in fl.static])
    with pytest.raises(mpmpc.MpmpcError, match="64"):
        h.rollout_set_movers([np.tile(r[:1], (5, 1)) for r in fl.rows])
    with pytest.raises(mpmpc.MpmpcError, match="different numbers of cars"):
        h.rollout_set_movers(fl.rows[:B - 1])
    with pytest.raises(mpmpc.MpmpcError, match="kind"):
        h.rollout_set_movers([np.array([(2, 3, 0.0, 0.0, 0.0, 0.0)])] * B)
    h.rollout_set_movers(fl.rows)
    with pytest.raises(mpmpc.MpmpcError, match="64"):
        h.rollout_set_obstacles([np.tile(d[:1], (62, 1)) for d in fl.static])
    h.rollout_set_obstacles(fl.static)
    _same(run(), moved)
    h.close()


@pytest.mark.gpu
def test_recorded_rows_are_the_rows_of_the_step_by_step_loop(car_twin):
    N, B, steps = 30, 64, 10
    fl = Fleet("sim", N, B, steps, 65, car_twin)
    h, _ = _handle("sim", N, B)
    h.rollout_record(steps, rows=True, B=B)
    h.rollout_set_obstacles(fl.static)
    h.rollout_set_movers(fl.rows)
    fl.init(h)
    h.rollout_step(steps)
    tr = h.rollout_trace()
    h.rollout_record(0, B=B)
    h.rollout_set_movers(None)
    fl.init(h)
    n_solved = 0
    for k in range(steps):
        h.rollout_set_obstacles(fl.discs_at(k))
        h.rollout_step(1)
        ub, lb = h.rollout_corridor()
        solved = np.isin(tr["alive"][k], (1, -1)) & (tr["alive"][k - 1] == 1 if k else np.ones(B, bool))
        assert np.array_equal(tr["ub"][k][solved], ub[solved]) and np.array_equal(tr["lb"][k][solved], lb[solved]), k
        assert not np.any(np.isnan(tr["ub"][k][solved])) and np.all(np.isnan(tr["ub"][k][~solved]))
        n_solved += int(solved.sum())
    h.close()
    assert n_solved * 2 >= B * steps
