"""The scratch of the entry points without a handle (csrc/device_scratch.hpp, scratch_acquire) when it is reused, regrown and
shared: every such export is called three times in one process - small, large (strictly more bytes in every region of its
block), small again over outputs pre-filled with a sentinel.  The third call must return the first one's bits, the large call
the CPU twin's (tests/twins.py, tests/localiser_twin.py) bit for bit - but for the two exports whose twin the project itself
holds to a figure: the speed profile's twin is the emulation, held to the 1e-9 that tests/test_speed_profile.py holds two runs
of that solver to, and the projection's x0 goes through tests/test_reroute.py's same_projection (wp, dist, s equal; x0, made
of a sine and a cosine that are the device's own and not glibc's, to 1e-12).  Then two threads: in different entry points (different scratch
tables: they may overlap) and both in mpmpc_lidar_scan (one table: the scratch's lock keeps the calls apart).

small: B = 1, 3 beams, a 16 x 16 map, one disc, one wall, one route of 4 corners, n = 8 segments.
large: B = 65 (one past a wavefront of cars), 64 beams, a 64 x 64 map, 8 discs and 4 walls per car.
Poses, headings and beam angles are seeded and irregular: no beam lies within the tie distance of a cell corner
(tests/test_lidar.py, THE TIE RULE), so device and twin are compared bit for bit."""
import ctypes as C
import threading

import numpy as np
import pytest

import mpmpc
import mpmpc_testlib as T
import localiser_twin
import twins
from test_path_build import TABLES, _call as _path_call
from test_reroute import same_projection, twin_project

pytestmark = pytest.mark.gpu

_d, _i = T._d, T._i
bp, u8p, u64p, u32p = C.POINTER(C.c_int8), C.POINTER(C.c_uint8), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
FILL = -7                                                   # what outputs hold before a call: no export returns it
SENTINEL = {"f8": FILL, "i4": FILL, "i1": FILL, "u1": 200, "u4": 0xAAAAAAAA, "u8": 0xAAAAAAAA}
RES, ORIGIN = 0.1, (-0.3, 0.2)
CAR = (0.25, 0.12, 0.4)                                     # length, width, reach [m]
MATCH = dict(D=3, m=1, W=2, T=1, step_psi=0.02, min_hits=1)


class World:
    """The arguments of one size, made once and never written."""

    def __init__(self, small):
        self.B, self.nb, side, nd, nw, self.n = (1, 3, 16, 1, 1, 8) if small else (65, 64, 64, 8, 4, 64)
        B = self.B
        rng = np.random.default_rng(31 if small else 32)
        g = np.ones((side, side), np.int8)
        g[0, :] = g[-1, :] = g[:, 0] = g[:, -1] = 0
        for _ in range(side // 8):                              # a few occupied blocks
            i, j = rng.integers(2, side - 4, 2)
            g[j:j + 2, i:i + 2] = 0
        self.grid, self.side = g, side
        cell = rng.uniform(3.0, side - 3.0, (B, 2))
        self.poses = np.ascontiguousarray(np.concatenate([np.array(ORIGIN) + cell * RES, rng.uniform(-3.0, 3.0, (B, 1))], 1))
        self.angles = np.linspace(-1.3, 1.3, self.nb) + 0.0123
        self.range = 0.6 * side * RES
        self.discs, self.walls = [], []
        for _ in range(B):
            r = rng.integers(1, 3, nd)
            self.discs.append(np.stack([rng.integers(2, side - 2, nd), rng.integers(2, side - 2, nd), r], 1).astype(np.int32))
            a = rng.integers(1, side - 1, (nw, 2))
            self.walls.append(np.concatenate([a, np.clip(a + rng.integers(-6, 7, (nw, 2)), 1, side - 2)], 1).astype(np.int32))
        self.off, self.flat = T.csr(self.discs, 3, n=B)
        self.woff, self.wflat = T.csr(self.walls, 4, n=B)
        # routes: one square of 4 corners per car, inside the map
        half = 0.25 * side * RES
        mid = np.array(ORIGIN) + 0.5 * side * RES + rng.uniform(-0.1, 0.1, (B, 2)) * side * RES
        sq = np.array([[-1, -1], [1, -1], [1, 1], [-1, 1]], float)
        self.routes = [mid[b] + half * sq for b in range(B)]
        # speed profile: B paths of n segments
        self.li = rng.uniform(0.03, 0.06, (B, self.n))
        self.kappa = rng.normal(0.0, 2.0, (B, self.n)) * (rng.uniform(0, 1, (B, self.n)) < 0.5)
        self.lim = np.ascontiguousarray(np.tile(np.array([-0.3, 0.4, 0.0, 1.2, 3.0]), (B, 1)))
        # projection: P routes of a circle each, B poses near them
        P, k = (1, 4) if small else (3, 40)
        t = np.linspace(0, 2 * np.pi, k, endpoint=False)
        tabs = [dict(x=c + np.cos(t), y=0.5 * c + np.sin(t), psi=t + np.pi / 2, cum_lengths=t.copy()) for c in range(P)]
        self.tab = {key: np.ascontiguousarray(np.concatenate([q[key] for q in tabs])) for key in tabs[0]}
        self.first = np.arange(P + 1, dtype=np.int32) * k
        self.P = P
        self.proj_poses = np.ascontiguousarray(np.stack([rng.uniform(-1, P, B), rng.uniform(-1, 2, B), rng.uniform(-3, 3, B)], 1))
        # scan match: the base map's own scans as measurements, the priors a little off the poses
        self.priors = np.ascontiguousarray(self.poses + rng.uniform(-0.05, 0.05, (B, 3)) * np.array([1, 1, 0.2]))
        for a in vars(self).values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)

    def map_args(self):
        return [self.side, self.side, self.grid.ctypes.data_as(bp), ORIGIN[0], ORIGIN[1], RES]


@pytest.fixture(scope="module")
def worlds():
    return {"small": World(True), "large": World(False)}


@pytest.fixture(scope="module")
def measured(worlds):
    """the ranges mpmpc_scan_match is handed: the twin's scans of the base map, per size"""
    return {k: _lidar_twin(w) for k, w in worlds.items()}


def _lidar_twin(w):
    out = np.full((w.B, w.nb), float(FILL))
    skipped, enclosed = np.zeros(w.B, np.int32), np.zeros((w.B, 2), np.int32)
    assert twins.lidar().lid_emu_scan(*w.map_args(), w.B, _d(w.poses), _i(w.off), _i(w.flat), w.nb, _d(w.angles), w.range, _d(out),
                                      _i(skipped), _i(enclosed)) == 0
    return out


# ------------------------------------------------------------------------------- the exports: fn(w, on) -> dict of outputs
# on = None: the CPU twin; else the library (the call goes to device 0, the outputs are pre-filled with FILL)
def _ok(lib, rc):
    assert rc == 0, lib.mpmpc_last_error().decode()


def speed_profile(w, lib, rg=None):
    if lib is None:
        v, status, _ = T.emu_speed_profile_wave(w.li, w.kappa, w.lim)
        return dict(v=v, status=status)
    v, status, iters = np.full((w.B, w.n), float(FILL)), np.full(w.B, FILL, np.int32), np.full(w.B, FILL, np.int32)
    _ok(lib, lib.mpmpc_speed_profile(0, w.B, w.n, _d(w.li), _d(w.kappa), _d(w.lim), 1e-12, _d(v), _i(status), _i(iters)))
    return dict(v=v, status=status, iters=iters)


def _scan(w, lib, walls, poses=None):
    poses = w.poses if poses is None else poses
    out = np.full((w.B, w.nb), float(FILL))
    head, tail = [*w.map_args(), w.B, _d(poses), _i(w.off), _i(w.flat)], [w.nb, _d(w.angles), w.range, _d(out)]
    wl = [_i(w.woff), _i(w.wflat)]
    if lib is None:
        if not walls:
            return dict(ranges=_lidar_twin(w))
        assert twins.walls().wall_emu_scan(*head, *wl, *tail) == 0
    elif walls:
        _ok(lib, lib.mpmpc_lidar_scan_world(0, *head, *wl, *tail))
    else:
        _ok(lib, lib.mpmpc_lidar_scan(0, *head, *tail))
    return dict(ranges=out)


def lidar_scan(w, lib, rg=None):
    return _scan(w, lib, False)


def lidar_scan_world(w, lib, rg=None):
    return _scan(w, lib, True)


def _audit(w, lib, walls, poses=None):
    poses = w.poses if poses is None else poses
    con, clr = np.full(w.B, FILL, np.int32), np.full(w.B, float(FILL))
    head, tail = [*w.map_args(), w.B, _d(poses), _i(w.off), _i(w.flat)], [*CAR, _i(con), _d(clr)]
    wl = [_i(w.woff), _i(w.wflat)]
    if lib is None:
        assert (twins.walls().wall_emu_audit(*head, *wl, *tail) if walls else twins.footprint().fp_emu_audit(*head, *tail)) == 0
    elif walls:
        _ok(lib, lib.mpmpc_footprint_audit_world(0, *head, *wl, *tail))
    else:
        _ok(lib, lib.mpmpc_footprint_audit(0, *head, *tail))
    return dict(contact=con, clearance=clr)


def footprint_audit(w, lib, rg=None):
    return _audit(w, lib, False)


def footprint_audit_world(w, lib, rg=None):
    return _audit(w, lib, True)


def world_grid(w, lib, rg=None):
    out = np.full_like(w.grid, FILL)
    d, wl = w.discs[-1], w.walls[-1]                            # one car's world
    if lib is None:
        assert twins.walls().wall_emu_world_grid(w.side, w.side, w.grid.ctypes.data_as(bp), len(d), _i(d), len(wl), _i(wl),
                                                 out.ctypes.data_as(bp)) == 0
    else:
        _ok(lib, lib.mpmpc_world_grid(0, *w.map_args(), len(d), _i(d), len(wl), _i(wl), out.ctypes.data_as(bp)))
    return dict(grid=out)


def perception_scan(w, lib, rg=None):
    out, ds, ws = np.full((w.B, w.nb), float(FILL)), np.full(w.B, 0xAAAAAAAA, np.uint64), np.full(w.B, 0xAAAAAAAA, np.uint32)
    args = [*w.map_args(), w.B, _d(w.poses), _i(w.off), _i(w.flat), _i(w.woff), _i(w.wflat), w.nb, _d(w.angles), w.range, _d(out),
            ds.ctypes.data_as(u64p), ws.ctypes.data_as(u32p)]
    if lib is None:
        assert twins.perception().per_emu_scan(*args) == 0
    else:
        _ok(lib, lib.mpmpc_perception_scan(0, *args))
    return dict(ranges=out, disc_seen=ds, wall_seen=ws)


def _path(w, lib, timed):
    a = (w.grid, ORIGIN, RES, w.routes, 0.05, 2, 0.3, True)
    kw = dict(discs=w.discs, walls=w.walls, fill=float(FILL))
    if lib is None:
        rc, o = _path_call(twins.path().path_emu_build, *a, count=twins.path().path_emu_count, **kw)
        assert rc == 0
        return o
    ms = np.full(3, float(FILL), np.float32)
    fn = (lambda dev, *args: lib.mpmpc_path_build_timed(dev, *args, ms.ctypes.data_as(C.POINTER(C.c_float)))) if timed else lib.mpmpc_path_build
    rc, o = _path_call(fn, *a, count=lib.mpmpc_path_count, device=0, **kw)
    _ok(lib, rc)
    assert not timed or np.all(ms >= 0)
    return o


def path_build(w, lib, rg=None):
    return _path(w, lib, False)


def path_build_timed(w, lib, rg=None):
    return _path(w, lib, True)


def project(w, lib, rg=None):
    if lib is None:
        return twin_project(twins.project(), w.tab, w.proj_poses, first=w.first)
    B, K = w.B, w.P
    out = dict(wp=np.full((B, K), FILL, np.int32), dist=np.full((B, K), float(FILL)), x0=np.full((B, K, 3), float(FILL)),
               s=np.full((B, K), float(FILL)))
    _ok(lib, lib.mpmpc_project(0, w.tab["x"].size, _d(w.tab["x"]), _d(w.tab["y"]), _d(w.tab["psi"]), _d(w.tab["cum_lengths"]), w.P,
                               _i(w.first), B, _d(w.proj_poses), K, None, np.pi, _i(out["wp"]), _d(out["dist"]), _d(out["x0"]),
                               _d(out["s"])))
    return out


def plant_noise(w, lib, rg=None):
    steps, seed, car0, j0 = w.n, 0x9E3779B97F4A7C15, 5, 1000
    out = np.full((steps, w.B, 5), float(FILL))
    if lib is None:
        j = np.arange(j0, j0 + steps, dtype=np.int64)
        twins.plant().pl_emu_noise(seed, car0, w.B, steps, j.ctypes.data_as(C.POINTER(C.c_int64)), _d(out))
    else:
        _ok(lib, lib.mpmpc_plant_noise(0, seed, car0, w.B, j0, steps, _d(out)))
    return dict(noise=out)


def distance_field(w, lib, rg=None):
    out = np.full(w.grid.shape, 200, np.uint8)
    if lib is None:
        localiser_twin.localiser().lc_emu_field(w.side, w.side, w.grid.ctypes.data_as(bp), MATCH["D"], out.ctypes.data_as(u8p))
    else:
        _ok(lib, lib.mpmpc_distance_field(0, w.side, w.side, w.grid.ctypes.data_as(bp), MATCH["D"], out.ctypes.data_as(u8p)))
    return dict(field=out)


def scan_match(w, lib, rg=None):
    B, M = w.B, MATCH
    o = dict(fix=np.full((B, 3), float(FILL)), score=np.full(B, FILL, np.int32), cand=np.full(B, FILL, np.int32), hits=np.full(B, FILL, np.int32))
    sets = [M["D"], M["m"], M["W"], M["T"], M["step_psi"], M["min_hits"]]
    if lib is None:
        field, edge = distance_field(w, None)["field"], np.zeros(B)
        localiser_twin.localiser().lc_emu_match(*w.map_args()[:3], field.ctypes.data_as(u8p), ORIGIN[0], ORIGIN[1], RES, B, _d(w.priors), _d(rg),
                                                None, w.nb, _d(w.angles), w.range, *sets, _d(o["fix"]), _i(o["score"]), _i(o["cand"]),
                                                _i(o["hits"]), _d(edge))
    else:
        _ok(lib, lib.mpmpc_scan_match(0, *w.map_args(), B, _d(w.priors), _d(rg), w.nb, _d(w.angles), w.range, *sets, _d(o["fix"]),
                                      _i(o["score"]), _i(o["cand"]), _i(o["hits"])))
    return o


EXPORTS = [speed_profile, lidar_scan, lidar_scan_world, footprint_audit, footprint_audit_world, world_grid, perception_scan, path_build,
           path_build_timed, project, plant_noise, distance_field, scan_match]      # (the twelve, and mpmpc_path_build_timed's sibling)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).tobytes(), a.shape, a.dtype


def _same(a, b, where):
    assert a.keys() == b.keys()
    for k in a:
        assert _bits(a[k]) == _bits(b[k]), (where, k)


@pytest.mark.parametrize("export", EXPORTS, ids=lambda f: f.__name__)
def test_small_large_small(export, worlds, measured):
    lib = mpmpc.load_library()
    first = export(worlds["small"], lib, measured["small"])
    large = export(worlds["large"], lib, measured["large"])
    again = export(worlds["small"], lib, measured["small"])
    _same(again, first, "the small call after the large one")
    for o in (first, large):                                    # every call wrote all of its outputs
        for k, a in o.items():
            assert not np.any(a == SENTINEL[a.dtype.kind + str(a.dtype.itemsize)]), k
    twin = export(worlds["large"], None, measured["large"])
    if export is speed_profile:
        assert np.array_equal(large["status"], twin["status"]) and np.all(large["status"] == 1)
        assert np.max(np.abs(large["v"] - twin["v"])) <= 1e-9
        return
    if export is project:      # wp, dist and s bit for bit, x0 to 1e-12: the device's sine and cosine are not glibc's
        return same_projection(large, twin, "large")
    for k in twin:
        if k in TABLES + ("border", "length"):      # (NaN where a path has no row)
            assert np.array_equal(large[k], twin[k], equal_nan=True), k
        else:
            assert _bits(large[k]) == _bits(twin[k]), k


def _threads(jobs):
    """jobs: callables -> their results, each run on a thread of its own, all started together"""
    out, errs = [None] * len(jobs), []

    def run(i):
        try:
            out[i] = jobs[i]()
        except BaseException as e:      # noqa: BLE001 (handed to the test's thread)
            errs.append(e)

    ts = [threading.Thread(target=run, args=(i,), daemon=True) for i in range(len(jobs))]
    for t in ts:
        t.start()
    for t in ts:
        t.join(60)
        assert not t.is_alive(), "a one-shot call did not return"
    assert not errs, errs
    return out


def test_two_entry_points_on_two_threads(worlds):
    """mpmpc_lidar_scan and mpmpc_footprint_audit, 8 calls each and sizes alternating, at once: what the same calls return serially"""
    lib = mpmpc.load_library()
    sizes = ["small", "large"] * 4
    scans = lambda: [_scan(worlds[s], lib, False) for s in sizes]
    audits = lambda: [_audit(worlds[s], lib, False) for s in sizes]
    want = [scans(), audits()]
    got = _threads([scans, audits])
    for g, w in zip(got, want):
        for k, (a, b) in enumerate(zip(g, w)):
            _same(a, b, k)


def test_one_entry_point_on_two_threads(worlds):
    """both threads in mpmpc_lidar_scan, each with its own poses: every call returns its own scan"""
    lib = mpmpc.load_library()
    w = worlds["large"]
    other = np.ascontiguousarray(w.poses[::-1] + np.array([0.013, -0.007, 0.3]))
    jobs = [lambda p=p: [_scan(w, lib, False, poses=p) for _ in range(8)] for p in (w.poses, other)]
    want = [job()[0] for job in jobs]
    assert _bits(want[0]["ranges"]) != _bits(want[1]["ranges"])
    for g, wnt in zip(_threads(jobs), want):
        for k, a in enumerate(g):
            _same(a, wnt, k)
