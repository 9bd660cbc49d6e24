"""Lidar on the device (K0l, mpmpc_lidar_scan / mpmpc_rollout_scan): LidarModel.scan for fleets and rollout worlds.

CPU: a numpy restatement of the law, written here from the header csrc/lidar_core.hpp, against the reference's scans
(golden G9, tests/golden/make_g9.py), the host twin of K0l (tests/emul_lidar, the same header) against G9 and against the
restatement on seeded fleets, LidarModel's fields, the argument checks through the C ABI.  GPU: the device against G9 and
against the twin, mpmpc_rollout_scan in its three worlds, scans that do not disturb a run, drop-in use.

THE TIE RULE.  A cell's beam interval comes from atan2, and numpy, glibc and the device each have their own.  Two of
them can differ only where an angle ties with something to within a few ulp, so every comparison between two
implementations leaves out exactly that case, computed by the restatement: a BEAM is tie-sensitive when an occupied
in-range cell has mn or mx within TIE = 1e-9 rad of its angle; a whole SCAN when a cell has mn within TIE of -pi/2 or mx
within TIE of pi/2, or one of its nine raw angles lies within TIE of the a < -pi wrap point, or wrapped within TIE of
+-pi.  TIE is about 10^6 times any libm's atan2 error at these magnitudes; it is no tolerance on ranges: every beam
that is compared must be bit-equal.  Caps: G9 none left out (the generator guarantees it), seeded fleets at most 1 beam
in 10 000.  Device against device has no exclusions."""
import ctypes as C
import math

import numpy as np
import pytest

import mpc_np as M
import mpmpc
import mpmpc_testlib as T
import twins
from map import Map, Obstacle

bp = C.POINTER(C.c_int8)
E_ARG, E_STATE = -1, -3
TIE = 1e-9
TS = 0.05


_d, _i, _g1 = T._d, T._i, T.g1_world


# ------------------------------------------------------------------------------------------------ worlds and fixtures
def _angles(fov, reso):
    """the beam angles of LidarModel(FoV, ., resolution) (src/lidar_model.py:28-33)"""
    n = int(fov / reso + 1)
    return np.linspace(-math.pi / 360 * fov, math.pi / 360 * fov, n)


@pytest.fixture(scope="module")
def g9():
    """-> list of scans: dict(track, pose, fov, range, reso, discs, angles, ranges)"""
    g = np.load(M.GOLDEN + "/g9_lidar.npz")
    out = []
    for k in range(int(g["n_scans"][0])):
        tr = str(g["track"][k])
        fov, rng, reso = (float(v) for v in g["sensor"][k])
        out.append(dict(track=tr, pose=g["pose"][k].copy(), fov=fov, range=rng, reso=reso, discs=g["discs_" + tr],
                        angles=g["measurements_%d" % k][0].copy(), ranges=g["measurements_%d" % k][1].copy()))
    return out


@pytest.fixture(scope="module")
def twin():
    """The CPU twin of K0l (tests/emul_lidar)."""
    return twins.lidar()


def _twin_scan(twin, grid, origin, res, poses, angles, rng, discs=None):
    poses = np.ascontiguousarray(poses, float).reshape(-1, 3)
    B = poses.shape[0]
    ang = np.ascontiguousarray(angles, float)
    off, flat = T.csr(discs, 3, n=B)
    out, skipped, enclosed = np.full((B, ang.size), -7.0), np.zeros(B, np.int32), np.zeros((B, 2), np.int32)
    rc = twin.lid_emu_scan(grid.shape[0], grid.shape[1], grid.ctypes.data_as(bp), origin[0], origin[1], res, B, _d(poses), _i(off),
                           _i(flat), ang.size, _d(ang), float(rng), _d(out), _i(skipped), _i(enclosed))
    assert rc == 0
    # K0l's shortcut (lid_cell_enclosure): wherever it gives an enclosure, the cell's interval lies inside
    assert not enclosed[:, 1].any(), enclosed[:, 1]
    _twin_scan.enclosed += int(enclosed[:, 0].sum())
    return out, skipped


_twin_scan.enclosed = 0


# ------------------------------------------------------------------------------- the law, restated from the header
def _cells(grid, origin, res, pose, rng, discs=None):
    """Steps 1 - 3 of csrc/lidar_core.hpp without the beams: None for a NaN row, else dict(d2, mn, mx, skip, raw, a) over the
    occupied in-range cells of the car's world (numpy's floor, arctan2 and mod, as the reference uses them)"""
    H, W = grid.shape
    x, y, psi = (float(v) for v in pose)
    with np.errstate(invalid="ignore", over="ignore"):
        qx, qy = np.floor((x - origin[0]) / res), np.floor((y - origin[1]) / res)
    if not math.isfinite(psi) or not (abs(qx) <= 2.0 ** 30 and abs(qy) <= 2.0 ** 30):
        return None
    cx, cy = int(qx), int(qy)
    lim = rng / res
    R = int(lim)
    i0, i1, j0, j1 = max(cx - R, 0), min(cx + R, W - 1), max(cy - R, 0), min(cy + R, H - 1)
    empty = dict(d2=np.zeros(0, np.int64), mn=np.zeros(0), mx=np.zeros(0), skip=np.zeros(0, bool), raw=np.zeros((0, 9)),
                 a=np.zeros((0, 9)))
    if i0 > i1 or j0 > j1:
        return empty
    occ = grid[j0:j1 + 1, i0:i1 + 1] == 0
    for dcx, dcy, r in ([] if discs is None else np.asarray(discs).reshape(-1, 3).tolist()):
        # cor_in_disc: dx, dy in [-r, r - 1] and dx^2 + dy^2 <= r^2
        xs = np.arange(max(dcx - r, i0), min(dcx + r - 1, i1) + 1)
        ys = np.arange(max(dcy - r, j0), min(dcy + r - 1, j1) + 1)
        if xs.size and ys.size:
            occ[np.ix_(ys - j0, xs - i0)] |= (xs[None, :] - dcx) ** 2 + (ys[:, None] - dcy) ** 2 <= r * r
    jj, ii = np.nonzero(occ)
    ii, jj = ii + i0, jj + j0
    d2 = (cx - ii) ** 2 + (cy - jj) ** 2
    keep = np.sqrt(d2.astype(float)) < lim
    ii, jj, d2 = ii[keep], jj[keep], d2[keep]
    if ii.size == 0:
        return empty
    ks = np.array([-0.5, 0.0, 0.5])
    dx = np.broadcast_to((ii - cx)[:, None, None] + ks[None, :, None], (ii.size, 3, 3))
    dy = np.broadcast_to((jj - cy)[:, None, None] + ks[None, None, :], (ii.size, 3, 3))
    raw = (np.arctan2(dy, dx) - psi).reshape(ii.size, 9)
    a = np.where(raw < -math.pi, -np.mod(math.pi + raw, 2 * math.pi) + math.pi, np.mod(math.pi + raw, 2 * math.pi) - math.pi)
    mn, mx = a.min(1), a.max(1)
    return dict(d2=d2, mn=mn, mx=mx, skip=(mn < -math.pi / 2) & (mx > math.pi / 2), raw=raw, a=a)


def _beams(c, angles, rng, res):
    """step 3's beams and step 4 -> (ranges [n], tie-sensitive beams [n] bool - all of them for a tie-sensitive scan)"""
    n = angles.size
    if c is None:
        return np.full(n, np.nan), np.zeros(n, bool)
    out = np.full(n, float(rng))
    if c["d2"].size == 0:
        return out, np.zeros(n, bool)
    mn, mx = c["mn"][:, None], c["mx"][:, None]
    hit = (~c["skip"])[:, None] & (mn <= angles[None, :]) & (angles[None, :] <= mx)
    big = np.iinfo(np.int64).max
    best = np.where(hit, c["d2"][:, None], big).min(0)
    out[best < big] = np.sqrt(best[best < big].astype(float)) * res
    tie = np.any((np.abs(mn - angles[None, :]) <= TIE) | (np.abs(mx - angles[None, :]) <= TIE), 0)
    whole = (np.abs(c["mn"] + math.pi / 2).min() <= TIE or np.abs(c["mx"] - math.pi / 2).min() <= TIE or
             np.abs(c["raw"] + math.pi).min() <= TIE or np.abs(np.abs(c["a"]) - math.pi).min() <= TIE)
    return out, (np.ones(n, bool) if whole else tie)


def _law(grid, origin, res, poses, angles, rng, discs=None):
    """-> ranges [B, n], tie-sensitive [B, n], skipped cells [B]"""
    poses = np.asarray(poses, float).reshape(-1, 3)
    out, tie, skipped = [], [], []
    for b in range(poses.shape[0]):
        c = _cells(grid, origin, res, poses[b], rng, None if discs is None else discs[b])
        r, t = _beams(c, angles, rng, res)
        out.append(r)
        tie.append(t)
        skipped.append(0 if c is None else int(c["skip"].sum()))
    return np.array(out), np.array(tie), np.array(skipped)


def _equal_outside_ties(a, b, tie):
    """bit-equal where compared (NaN rows equal NaN rows); -> the number of beams left out"""
    keep = ~tie
    assert np.array_equal(a[keep], b[keep], equal_nan=True), int(np.sum((a != b) & ~(np.isnan(a) & np.isnan(b)) & keep))
    return int(tie.sum())


# ------------------------------------------------------------------------------------------------ the seeded fleets
B_FLEET = 67
SENSORS = ((100, 200), (180, 1), (256, 0.25))         # FoV, resolution: n_beams = 1, 181, 1 025
RANGE = dict(sim=0.3, real=3.0)
_FLEETS = {}


def _fleet(track):
    """B = 67 cars at random waypoints (jittered, any heading in [-4, 4]) with 0 .. 64 discs each - around the car, some at
    the window's very edge, some absent (0, 0, 0), some of radius 0 - and the edge poses: a NaN x, a NaN and an infinite
    psi (NaN rows), 2^31 cells away (NaN row), 2^20 cells away (off the grid: every beam at range), in the grid's first and
    last cell, and just off the grid with the window reaching in."""
    if track in _FLEETS:
        return _FLEETS[track]
    g1, grid, origin, res = _g1(track)
    H, W = grid.shape
    rng = np.random.default_rng(901 if track == "sim" else 902)
    B = B_FLEET
    wp = rng.integers(0, g1["x"].size, B)
    poses = np.stack([g1["x"][wp] + rng.uniform(-8, 8, B) * res, g1["y"][wp] + rng.uniform(-8, 8, B) * res, rng.uniform(-4, 4, B)], 1)
    R = int(RANGE[track] / res)
    special = dict(nan_x=3, nan_psi=4, inf_psi=5, far31=6, far20=7, first=8, last=9, outside=10)
    poses[special["nan_x"], 0] = np.nan
    poses[special["nan_psi"], 2] = np.nan
    poses[special["inf_psi"], 2] = np.inf
    poses[special["far31"], 0] = origin[0] + res * 2.0 ** 31
    poses[special["far20"], 1] = origin[1] - res * 2.0 ** 20
    poses[special["first"], :2] = (origin[0], origin[1])
    poses[special["last"], :2] = (origin[0] + res * (W - 0.5), origin[1] + res * (H - 0.5))
    poses[special["outside"], :2] = (origin[0] - res * (R // 2), origin[1] + res * (H // 2))
    discs = []
    for b in range(B):
        k = b % 65                                                            # 0 .. 64, then 0 and 1 again
        with np.errstate(invalid="ignore"):
            cx, cy = np.floor((poses[b, 0] - origin[0]) / res), np.floor((poses[b, 1] - origin[1]) / res)
        if not (np.isfinite(cx) and np.isfinite(cy) and abs(cx) < 2 ** 20 and abs(cy) < 2 ** 20):
            cx, cy = W // 2, H // 2
        d = np.zeros((k, 3), np.int64)
        d[:, 0] = cx + rng.integers(-R - 3, R + 4, k)
        d[:, 1] = cy + rng.integers(-R - 3, R + 4, k)
        d[:, 2] = rng.integers(0, 7, k)
        if k >= 4:
            d[0] = (cx + R, cy - R // 3, 2)                                   # straddles the window's edge column
            d[1] = (cx - R - 2, cy, 2)                                        # touches it from outside: its last column is cx - R - 1
            d[2] = (0, 0, 0)                                                  # absent
        d[:, 2] = np.minimum(d[:, 2], np.minimum.reduce([d[:, 0], d[:, 1], W - d[:, 0], H - d[:, 1]]))      # the square stays on the grid
        d[d[:, 2] < 0] = 0                                                    # (a centre off the grid: absent)
        discs.append(d.astype(np.int32))
    _FLEETS[track] = dict(grid=grid, origin=origin, res=res, poses=poses, discs=discs, special=special, range=RANGE[track],
                          cells=[_cells(grid, origin, res, poses[b], RANGE[track], discs[b]) for b in range(B)])
    return _FLEETS[track]


def _fleet_law(f, angles):
    r, t = zip(*[_beams(c, angles, f["range"], f["res"]) for c in f["cells"]])
    return np.array(r), np.array(t)


# ------------------------------------------------------------------------------------------------------------ CPU
def test_restated_law_equals_the_reference_scans(g9):
    assert len(g9) >= 12 and {s["track"] for s in g9} == {"sim", "real"}
    seen = dict(clipped=0, inside=0, skipped=0, no_hit=0, wide_psi=0, fractional=0)
    for k, s in enumerate(g9):
        g1, grid, origin, res = _g1(s["track"])
        got, tie, skipped = _law(grid, origin, res, s["pose"], s["angles"], s["range"], [s["discs"]])
        assert not tie.any(), k                                               # the cap on G9: nothing left out
        assert np.array_equal(got[0], s["ranges"]), k
        world = Map.from_grid(grid, origin, res)
        cx, cy = world.w2m(s["pose"][0], s["pose"][1])
        R = int(s["range"] / res)
        occ = _cells(grid, origin, res, (origin[0] + (cx + 0.5) * res, origin[1] + (cy + 0.5) * res, 0.3), res * 1.5, s["discs"])
        seen["clipped"] += cx - R < 0 or cy - R < 0 or cx + R >= world.width or cy + R >= world.height
        seen["inside"] += bool(0 <= cx < world.width and 0 <= cy < world.height and np.any(occ["d2"] == 0))
        seen["skipped"] += skipped[0] > 0
        seen["no_hit"] += bool(np.all(s["ranges"] == s["range"]))
        seen["wide_psi"] += abs(s["pose"][2]) > math.pi
        seen["fractional"] += s["reso"] != int(s["reso"])
    assert all(v > 0 for v in seen.values()), seen
    assert {s["fov"] for s in g9} >= {90, 180, 270, 360}


def test_twin_equals_the_reference_scans(g9, twin):
    for k, s in enumerate(g9):
        g1, grid, origin, res = _g1(s["track"])
        got, _ = _twin_scan(twin, grid, origin, res, s["pose"], s["angles"], s["range"], [s["discs"]])
        assert np.array_equal(got[0], s["ranges"]), k
        baked = Map.from_grid(grid, origin, res)                              # the same world as one grid, no discs
        for cx, cy, r in s["discs"].tolist():
            yy, xx = np.ogrid[-r:r, -r:r]
            baked.data[cy - r:cy + r, cx - r:cx + r][xx ** 2 + yy ** 2 <= r ** 2] = 0
        got, _ = _twin_scan(twin, np.ascontiguousarray(baked.data), origin, res, s["pose"], s["angles"], s["range"])
        assert np.array_equal(got[0], s["ranges"]), k


@pytest.mark.parametrize("track", ["sim", "real"])
def test_twin_equals_the_restated_law_on_seeded_fleets(track, twin):
    f = _fleet(track)
    sp = f["special"]
    left_out = total = 0
    for fov, reso in SENSORS:
        ang = _angles(fov, reso)
        want, tie = _fleet_law(f, ang)
        got, skipped = _twin_scan(twin, f["grid"], f["origin"], f["res"], f["poses"], ang, f["range"], f["discs"])
        left_out += _equal_outside_ties(got, want, tie)
        total += want.size
        for k in ("nan_x", "nan_psi", "inf_psi", "far31"):
            assert np.all(np.isnan(got[sp[k]])), k
        assert np.all(got[sp["far20"]] == f["range"])
        assert np.isfinite(np.delete(got, [sp[k] for k in ("nan_x", "nan_psi", "inf_psi", "far31")], 0)).all()
        assert skipped.sum() > 0 or ang.size == 1
    print("beams left out by the tie rule: %d of %d" % (left_out, total))
    assert left_out * 10000 <= total
    assert _twin_scan.enclosed > 10000                                        # (the enclosure check above saw cells)
    assert [_angles(*s).size for s in SENSORS] == [1, 181, 1025]
    # ... and the cases are what they claim to be
    assert sorted({len(d) for d in f["discs"]}) == list(range(65))
    ang = _angles(*SENSORS[1])
    with_d, _ = _fleet_law(f, ang)
    without, _, _ = _law(f["grid"], f["origin"], f["res"], f["poses"], ang, f["range"])
    assert np.sum(np.any(with_d != without, 1) & ~np.isnan(with_d[:, 0])) >= 20          # the discs are seen
    for k in ("first", "last"):
        assert np.any(with_d[sp[k]] < f["range"]), k                                     # clipped windows that still hit
    assert f["cells"][sp["outside"]] is not None and np.all(np.isfinite(with_d[sp["outside"]]))


def test_lidar_model_fields_equal_the_reference(g9):
    from lidar_model import LidarModel
    for s in g9:
        fov, reso = (int(v) if v == int(v) else v for v in (s["fov"], s["reso"]))
        lm = LidarModel(FoV=fov, range=s["range"], resolution=reso)
        assert lm.n_measurements == s["angles"].size and lm.measurements.shape == (2, s["angles"].size)
        assert np.array_equal(lm.measurements[0], s["angles"]) and np.all(lm.measurements[1] == s["range"])
        assert (lm.FoV, lm.range, lm.resolution) == (fov, s["range"], reso)
    assert hasattr(LidarModel, "scan") and hasattr(LidarModel, "scan_batch") and hasattr(LidarModel, "plot_scan")
    assert hasattr(mpmpc.Handle, "rollout_scan")
    from MPC import BatchMPC
    assert hasattr(BatchMPC, "rollout_scan")


def test_argument_checks_through_the_abi_without_device(built_library, twin):
    lib = mpmpc.load_library(built_library)
    grid = np.ones((40, 50), np.int8)
    pose = np.array([[0.1, 0.1, 0.3], [0.2, 0.1, 0.3]])
    ang = _angles(180, 1)
    out = np.zeros((2, 2048))

    def call(n=None, angles=ang, rng=0.1, off=None, discs=None, res=0.01, B=2):
        angles = np.ascontiguousarray(angles, float)
        n = angles.size if n is None else n
        off = None if off is None else np.ascontiguousarray(off, np.int32)
        discs = None if discs is None else np.ascontiguousarray(discs, np.int32)
        rc = lib.mpmpc_lidar_scan(0, 40, 50, grid.ctypes.data_as(bp), 0.0, 0.0, res, B, _d(pose), _i(off), _i(discs), n, _d(angles),
                                  rng, _d(out))
        rc2 = twin.lid_emu_check(40, 50, grid.ctypes.data_as(bp), res, B, _d(pose), _i(off), _i(discs), n, _d(angles), rng, _d(out))
        assert rc2 == (rc if rc == E_ARG else 0)                              # the twin runs the same checks
        return rc, lib.mpmpc_last_error()

    def refused(word, **kw):
        rc, why = call(**kw)
        assert rc == E_ARG and word in why, (kw, rc, why)

    refused(b"n_beams", n=0)
    refused(b"n_beams", angles=np.linspace(-1, 1, 2049))
    refused(b"finite", angles=[-1.0, np.nan, 1.0])
    refused(b"finite", angles=[-1.0, 0.0, np.inf])
    refused(b"ascending", angles=[-1.0, 0.5, 0.0])
    for r in (0.0, -1.0, np.inf, np.nan):
        refused(b"range", rng=r)
    refused(b"2048 cells", rng=20.49)                                         # R = 2049
    refused(b"decrease", off=[0, 2, 1], discs=[[5, 5, 1]] * 2)
    refused(b"64 discs", off=[0, 65, 65], discs=[[5, 5, 1]] * 65)
    refused(b"leaves the map", off=[0, 1, 1], discs=[[2, 5, 3]])
    refused(b"leaves the map", off=[0, 0, 1], discs=[[48, 5, 3]])
    refused(b"negative radius", off=[0, 0, 1], discs=[[10, 5, -1]])
    refused(b"B must", B=0)
    refused(b"resolution", res=0.0)
    assert lib.mpmpc_lidar_scan(0, 40, 50, None, 0.0, 0.0, 0.01, 2, _d(pose), None, None, ang.size, _d(ang), 0.1, _d(out)) == E_ARG
    assert lib.mpmpc_rollout_scan(None, 2, ang.size, _d(ang), 0.1, _d(out)) == E_ARG      # no handle
    # what passes the checks reaches the device call: without a device that is an error of another kind, never a result
    rc, why = call(rng=20.48, off=[0, 64, 64], discs=[[5, 5, 5]] * 64)        # R = 2048 and 64 discs: the caps themselves
    assert rc != E_ARG
    if mpmpc.device_count() == 0:
        assert rc == -2 and why != b""


# ------------------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
def test_device_equals_the_reference_scans(g9):
    for k, s in enumerate(g9):
        g1, grid, origin, res = _g1(s["track"])
        got = mpmpc.lidar_scan(grid, origin, res, [s["pose"]], s["angles"], s["range"], [s["discs"]])
        assert got.shape == (1, s["angles"].size) and np.array_equal(got[0], s["ranges"]), k


@pytest.mark.gpu
@pytest.mark.parametrize("track", ["sim", "real"])
def test_device_equals_the_twin_on_seeded_fleets(track, twin):
    f = _fleet(track)
    left_out = total = 0
    for fov, reso in SENSORS:
        ang = _angles(fov, reso)
        _, tie = _fleet_law(f, ang)
        want, _ = _twin_scan(twin, f["grid"], f["origin"], f["res"], f["poses"], ang, f["range"], f["discs"])
        got = mpmpc.lidar_scan(f["grid"], f["origin"], f["res"], f["poses"], ang, f["range"], f["discs"])
        left_out += _equal_outside_ties(got, want, tie)
        total += want.size
        again = mpmpc.lidar_scan(f["grid"], f["origin"], f["res"], f["poses"], ang, f["range"], f["discs"])
        assert np.array_equal(got, again, equal_nan=True)                     # device against device: no exclusions
    print("beams left out by the tie rule: %d of %d" % (left_out, total))
    assert left_out * 10000 <= total
    # B = 1, with and without discs
    ang = _angles(*SENSORS[1])
    _, tie = _fleet_law(f, ang)
    b = 20
    got = mpmpc.lidar_scan(f["grid"], f["origin"], f["res"], f["poses"][b:b + 1], ang, f["range"], f["discs"][b:b + 1])
    want, _ = _twin_scan(twin, f["grid"], f["origin"], f["res"], f["poses"][b:b + 1], ang, f["range"], f["discs"][b:b + 1])
    _equal_outside_ties(got, want, tie[b:b + 1])
    got = mpmpc.lidar_scan(f["grid"], f["origin"], f["res"], f["poses"][b:b + 1], ang, f["range"])
    want, _ = _twin_scan(twin, f["grid"], f["origin"], f["res"], f["poses"][b:b + 1], ang, f["range"])
    assert len(f["discs"][b]) == 20 and np.array_equal(got, want)


def _rollout_world(B=16, N=30):
    """a handle on Sim_Track with B cars, and per car 2 static discs, 2 movers along the path and traffic in one group"""
    import test_traffic as TT
    g1, grid, origin, res = _g1("sim")
    h, _ = TT._handle("sim", N, B)
    rng = np.random.default_rng(77)
    cum = np.cumsum(g1["segment_lengths"])
    starts = (np.arange(B) * 11 + 3) % g1["x"].size
    poses = np.stack([g1["x"][starts], g1["y"][starts], g1["psi"][starts] + rng.uniform(-0.05, 0.05, B)], 1)
    m = Map.from_grid(grid, origin, res)
    static = [m.obstacle_discs([Obstacle(x + rng.uniform(-0.05, 0.05), y + rng.uniform(-0.05, 0.05), r)
                                for x, y, r in (TT.BASE["sim"][q] for q in rng.choice(len(TT.BASE["sim"]), 2, replace=False))])
              for _ in range(B)]
    rows = [np.array([(1, 6, cum[(starts[b] + 8 + 9 * q) % cum.size], rng.uniform(-0.08, 0.08), 0.004, 0.0) for q in range(2)])
            for b in range(B)]
    return dict(h=h, grid=grid, origin=origin, res=res, cum=cum, starts=starts, poses=poses, static=static, rows=rows,
                group=np.zeros(B, np.int32), rad=np.full(B, 7, np.int32), B=B, N=N)


def _set_all(w):
    w["h"].rollout_set_obstacles(w["static"])
    w["h"].rollout_set_movers(w["rows"])
    w["h"].rollout_set_traffic(w["group"], w["rad"], 3, -1)


@pytest.fixture(scope="module")
def rollout_scans():
    """computed once: the scans of a rollout in its three worlds, by mpmpc_rollout_scan and by mpmpc_lidar_scan on the
    state the host can read"""
    w = _rollout_world()
    h = w["h"]
    ang, rng = _angles(270, 1.5), 0.3
    out = dict(w=w, ang=ang, rng=rng, errors={})

    def refused(key):
        try:
            h.rollout_scan(ang, rng)
            out["errors"][key] = None
        except mpmpc.MpmpcError as e:
            out["errors"][key] = str(e)
    refused("before rollout_init")
    _set_all(w)
    h.rollout_init(TS, w["cum"], w["cum"][w["starts"]], w["poses"])
    refused("settings no step has used")
    h.rollout_step(4)
    out["got"] = h.rollout_scan(ang, rng)
    st, discs = h.rollout_state(), h.rollout_obstacles()
    out["discs"] = discs
    out["want"] = mpmpc.lidar_scan(w["grid"], w["origin"], w["res"], st["pose"], ang, rng, discs)
    out["bare"] = mpmpc.lidar_scan(w["grid"], w["origin"], w["res"], st["pose"], ang, rng)
    out["alive"] = st["alive"]
    h.rollout_set_traffic(w["group"], w["rad"], 2, -1)
    refused("a setter with no step since")
    h.rollout_step(1)
    out["got2"] = h.rollout_scan(ang, rng)
    out["want2"] = mpmpc.lidar_scan(w["grid"], w["origin"], w["res"], h.rollout_state()["pose"], ang, rng, h.rollout_obstacles())
    try:
        h.rollout_scan(ang, 0.0)
        out["errors"]["range 0"] = None
    except mpmpc.MpmpcError as e:
        out["errors"]["range 0"] = str(e)
    h.upload(np.zeros(w["B"], np.int32), np.zeros((w["B"], 3)), np.zeros((w["B"], 2 * w["N"])))
    refused("after an upload")
    for off in (h.rollout_set_obstacles, h.rollout_set_movers, h.rollout_set_traffic):
        off(None)
    h.rollout_init(TS, w["cum"], w["cum"][w["starts"]], w["poses"])
    out["base0"] = h.rollout_scan(ang, rng)                                   # no per-car setting: no step is needed
    out["base0_want"] = mpmpc.lidar_scan(w["grid"], w["origin"], w["res"], w["poses"], ang, rng)
    h.rollout_step(3)
    out["base"] = h.rollout_scan(ang, rng)
    out["base_want"] = mpmpc.lidar_scan(w["grid"], w["origin"], w["res"], h.rollout_state()["pose"], ang, rng)
    h.close()
    return out


@pytest.mark.gpu
def test_rollout_scan_in_its_three_worlds(rollout_scans):
    r = rollout_scans
    B = r["w"]["B"]
    assert r["got"].shape == (B, r["ang"].size)
    assert np.array_equal(r["got"], r["want"]) and np.array_equal(r["got2"], r["want2"])
    # the worlds were worth scanning: statics, movers and traffic slots present, and seen by the scans
    kinds = np.array([[np.any(d[:2, 2] > 0), np.any(d[2:4, 2] > 0), np.any(d[4:, 2] > 0)] for d in r["discs"]])
    assert all(d.shape == (7, 3) for d in r["discs"]) and kinds.all(0).all()
    assert np.sum(np.any(r["got"] != r["bare"], 1)) >= 4
    assert np.array_equal(r["base0"], r["base0_want"]) and np.array_equal(r["base"], r["base_want"])
    assert np.any(r["base"] < r["rng"])


@pytest.mark.gpu
def test_rollout_scan_state_errors(rollout_scans):
    e = rollout_scans["errors"]
    for key in ("before rollout_init", "settings no step has used", "a setter with no step since", "after an upload"):
        assert e[key] is not None and "error %d" % E_STATE in e[key], (key, e[key])
    assert e["range 0"] is not None and "error %d" % E_ARG in e["range 0"]


@pytest.mark.gpu
def test_scans_do_not_disturb_a_run():
    import test_traffic as TT
    ang, rng = _angles(180, 1), 0.3
    finals = []
    for scanning in (False, True):
        w = _rollout_world()
        h = w["h"]
        _set_all(w)
        h.rollout_init(TS, w["cum"], w["cum"][w["starts"]], w["poses"])
        for _ in range(4):
            h.rollout_step(2)
            if scanning:
                h.rollout_scan(ang, rng)
        finals.append((h.rollout_state(), h.rollout_corridor(), h.rollout_obstacles()))
        h.close()
    (a, a_rows, a_discs), (b, b_rows, b_discs) = finals
    for k in TT.KEYS + ("x0", "u"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a_rows[0], b_rows[0], equal_nan=True) and np.array_equal(a_rows[1], b_rows[1], equal_nan=True)
    assert all(np.array_equal(p, q) for p, q in zip(a_discs, b_discs))
    assert np.any(a["alive"] == 1)


@pytest.mark.gpu
def test_drop_in_use(g9, rollout_scans):
    from lidar_model import LidarModel
    from MPC import BatchMPC
    from scipy import sparse
    s = g9[0]
    assert s["track"] == "sim"
    g1, grid, origin, res = _g1("sim")
    world = Map.from_grid(grid, origin, res)
    for cx, cy, r in s["discs"].tolist():
        yy, xx = np.ogrid[-r:r, -r:r]
        world.data[cy - r:cy + r, cx - r:cx + r][xx ** 2 + yy ** 2 <= r ** 2] = 0

    class Car:
        x, y, psi = (float(v) for v in s["pose"])
    lm = LidarModel(FoV=int(s["fov"]), range=s["range"], resolution=int(s["reso"]))
    lm.scan(Car, world)
    assert np.array_equal(lm.measurements[1], s["ranges"]) and np.array_equal(lm.measurements[0], s["angles"])
    both = lm.scan_batch([s["pose"], s["pose"]], Map.from_grid(grid, origin, res), discs=[s["discs"], np.zeros((0, 3))])
    assert np.array_equal(both[0], s["ranges"]) and not np.array_equal(both[1], s["ranges"])
    # BatchMPC: one car parked at G9's pose on the map with G9's obstacles - a rollout of zero steps leaves it there
    m, rp, car = T.build_world(obstacles=False)
    m.data[:] = world.data
    Q, R, QN = sparse.diags([1.0, 0.0, 0.0]), sparse.diags([0.5, 0.0]), sparse.diags([1.0, 0.0, 0.0])
    ic = {'umin': np.array([0.0, -np.tan(0.66) / car.length]), 'umax': np.array([1.0, np.tan(0.66) / car.length])}
    sc = {'xmin': np.array([-np.inf] * 3), 'xmax': np.array([np.inf] * 3)}
    r = rollout_scans
    w = r["w"]
    bm = BatchMPC(car, w["N"], Q, R, QN, sc, ic, 4.0, max_batch=w["B"], corridor="device")
    bm.rollout(np.zeros(1), [s["pose"]], 0)
    assert np.array_equal(bm.rollout_scan(lm)[0], s["ranges"])
    # ... and a rollout in the three worlds, through BatchMPC's own arguments: test 8's equality
    import movers
    import traffic
    m.data[:] = grid
    bm.update_corridor_from_map()
    rng = np.random.default_rng(78)
    B = w["B"]
    base = [(0.0, 0.0, 0.05), (-0.3, -1.0, 0.08), (0.73, -0.9, 0.07), (1.2, 0.0, 0.08)]
    obstacles = [[Obstacle(x + rng.uniform(-0.05, 0.05), y + rng.uniform(-0.05, 0.05), rad) for x, y, rad in base[b % 3:b % 3 + 2]]
                 for b in range(B)]
    mv = [[movers.Mover.along_path(w["cum"][(w["starts"][b] + 9) % w["cum"].size], rng.uniform(-0.08, 0.08), 0.08, 0.03)] for b in range(B)]
    tf = traffic.Traffic(np.zeros(B, int), 0.035, 3)
    st = bm.rollout(w["cum"][w["starts"]], w["poses"], 4, obstacles=obstacles, movers=mv, traffic=tf)
    lm2 = LidarModel(FoV=270, range=r["rng"], resolution=1.5)
    assert np.array_equal(lm2.measurements[0], r["ang"])
    discs = bm.handle.rollout_obstacles()
    got = bm.rollout_scan(lm2)
    assert all(d.shape == (6, 3) for d in discs) and got.shape == (B, lm2.n_measurements)
    assert np.array_equal(got, mpmpc.lidar_scan(grid, origin, res, st["pose"], lm2.measurements[0], lm2.range, discs))
    assert np.any(got != mpmpc.lidar_scan(grid, origin, res, st["pose"], lm2.measurements[0], lm2.range))
    bm.close()
