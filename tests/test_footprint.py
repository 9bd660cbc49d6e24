"""Footprint audit on the device (K0f, mpmpc_footprint_audit / mpmpc_rollout_set_audit / mpmpc_rollout_audit): contact and
clearance of every car's rectangle in the car's own world.

CPU: a numpy restatement of the law, written here from the header csrc/footprint_core.hpp, on hand cases; the host twin of
K0f (tests/emul_footprint, the same header) against the restatement on seeded fleets; Footprint's fields; the argument
checks through the C ABI.  GPU: the device against the twin, the audit inside a rollout teacher-forced from its own trace,
rollout_step(n) against n steps of one, an audit that does not disturb a run, mode 2.

THE TIE RULE.  The car's frame comes from cos(psi) and sin(psi), and numpy, glibc and the device each have their own.  Two
of them can differ by a few ulp, so the contact FLAG of two implementations can differ only where an occupied window cell
lies on the rectangle's boundary to within rounding.  The restatement marks a car as tie-sensitive when such a cell lies
within TIE = 1e-9 m of the boundary: outside with 0 < sqrt(g) < TIE, or inside with min(length/2 - |u|, width/2 - |v|) < TIE.
Comparisons between two implementations leave those cars out - at most 1 car in 1 000 per seeded fleet, which the CPU tests
check of the restatement alone - and every compared flag must be equal.  TIE is about 10^6 times the rounding at these
magnitudes; it is no tolerance on clearances.  Those agree to CLR_TOL = 16 eps (reach + length + width + 2 res): the only
differing inputs are c and s, the distance is 1-Lipschitz in (u, v), and |dx| + |dy| <= 2 (R + 1) res (measured on the
device against the twin: at most 5.6e-17 m where the bound is 8.5e-16 .. 4.9e-15; every comparison prints its figure).
Device against device has no exclusions and is bit-equal."""
import ctypes as C
import math

import numpy as np
import pytest

import mpmpc
import mpmpc_testlib as T
import twins
from map import Map, Obstacle

bp = C.POINTER(C.c_int8)
E_ARG, E_HIP, E_STATE = -1, -2, -3
TIE = 1e-9
EPS = 2.2e-16
TS = 0.05
ACC = ("contact_steps", "first_contact", "min_clearance", "min_step", "last_contact", "last_clearance")


def clr_tol(reach, length, width, res):
    return 16 * EPS * (reach + length + width + 2 * res)


_d, _i, _g1 = T._d, T._i, T.g1_world


# ------------------------------------------------------------------------------------------------ worlds and fixtures
@pytest.fixture(scope="module")
def twin():
    """The CPU twin of K0f (tests/emul_footprint)."""
    return twins.footprint()


def _twin_audit(twin, grid, origin, res, poses, car, discs=None):
    """car = (length, width, reach) -> contact [B] int32, clearance [B]"""
    poses = np.ascontiguousarray(poses, float).reshape(-1, 3)
    B = poses.shape[0]
    off, flat = T.csr(discs, 3, n=B)
    contact, clearance = np.full(B, -7, np.int32), np.full(B, -7.0)
    rc = twin.fp_emu_audit(grid.shape[0], grid.shape[1], grid.ctypes.data_as(bp), origin[0], origin[1], res, B, _d(poses), _i(off),
                           _i(flat), car[0], car[1], car[2], _i(contact), _d(clearance))
    assert rc == 0
    return contact, clearance


def _reach_cells(car, res):
    return int((car[2] + 0.5 * math.sqrt(car[0] ** 2 + car[1] ** 2)) / res) + 1


# ------------------------------------------------------------------------------- the law, restated from the header
def _law_one(grid, origin, res, pose, car, discs=None):
    """Steps 1 - 4 of csrc/footprint_core.hpp for one car -> (contact, clearance, tie-sensitive)"""
    H, W = grid.shape
    length, width, reach = car
    x, y, psi = (float(v) for v in pose)
    with np.errstate(invalid="ignore", over="ignore"):
        qx, qy = np.floor((x - origin[0]) / res), np.floor((y - origin[1]) / res)
    if not math.isfinite(psi) or not (abs(qx) <= 2.0 ** 30 and abs(qy) <= 2.0 ** 30):
        return 0, math.nan, False
    cx, cy = int(qx), int(qy)
    c, s = np.cos(psi), np.sin(psi)
    R = _reach_cells(car, res)
    i0, i1, j0, j1 = max(cx - R, 0), min(cx + R, W - 1), max(cy - R, 0), min(cy + R, H - 1)
    if i0 > i1 or j0 > j1:
        return 0, reach, False
    occ = grid[j0:j1 + 1, i0:i1 + 1] == 0
    for dcx, dcy, r in ([] if discs is None else np.asarray(discs).reshape(-1, 3).tolist()):
        # cor_in_disc: dx, dy in [-r, r - 1] and dx^2 + dy^2 <= r^2
        xs = np.arange(max(dcx - r, i0), min(dcx + r - 1, i1) + 1)
        ys = np.arange(max(dcy - r, j0), min(dcy + r - 1, j1) + 1)
        if xs.size and ys.size:
            occ[np.ix_(ys - j0, xs - i0)] |= (xs[None, :] - dcx) ** 2 + (ys[:, None] - dcy) ** 2 <= r * r
    jj, ii = np.nonzero(occ)
    if ii.size == 0:
        return 0, reach, False
    px, py = (ii + i0 + 0.5) * res + origin[0], (jj + j0 + 0.5) * res + origin[1]
    dx, dy = px - x, py - y
    u, v = c * dx + s * dy, c * dy - s * dx
    au, av = np.abs(u) - length / 2, np.abs(v) - width / 2
    du, dv = np.maximum(au, 0.0), np.maximum(av, 0.0)
    g = du * du + dv * dv
    d = np.sqrt(g)
    inside = g == 0
    tie = bool(np.any((d > 0) & (d < TIE)) or np.any(inside & (np.minimum(-au, -av) < TIE)))
    return int(inside.any()), min(reach, float(d.min())), tie


def _law(grid, origin, res, poses, car, discs=None):
    poses = np.asarray(poses, float).reshape(-1, 3)
    out = [_law_one(grid, origin, res, poses[b], car, None if discs is None else discs[b]) for b in range(poses.shape[0])]
    return (np.array([o[0] for o in out], np.int32), np.array([o[1] for o in out], float), np.array([o[2] for o in out], bool))


def _compare(got, want, tie, tol):
    """flags equal and clearances within tol on every car the tie rule keeps (a NaN equals a NaN); -> cars left out"""
    keep = ~tie
    assert np.array_equal(got[0][keep], want[0][keep]), np.nonzero((got[0] != want[0]) & keep)[0]
    a, b = got[1][keep], want[1][keep]
    assert np.array_equal(np.isnan(a), np.isnan(b))
    diff = np.abs(a - b)[~np.isnan(a)]
    print("largest clearance difference %.3g (bound %.3g)" % (diff.max() if diff.size else 0.0, tol))
    assert diff.size == 0 or diff.max() <= tol, (diff.max(), tol)
    return int(tie.sum())


# ------------------------------------------------------------------------------------------------ the seeded fleets
B_FLEET = 2048
CARS = dict(sim=(0.12, 0.06, 0.05), real=(0.3, 0.2, 0.3))      # length, width, reach: R = 24 and 9
SEEDS = dict(sim=1201, real=1202)
SPECIAL = dict(nan_x=33, nan_psi=34, inf_psi=35, far31=36, far20=37, outside=38, c00=40, c10=41, c01=42, c11=43, e_lo_x=44,
               e_hi_x=45, e_lo_y=46, e_hi_y=47)
_FLEETS = {}


def _fleet(track):
    """B = 2 048 cars.  Three in four sit within a few cells of a wall (a random occupied cell that has a free neighbour,
    jittered by up to half a car length, any heading), one in four on the path's centre line; car b carries b % 65 discs
    (one car in four anywhere in its window, the others around it, where they bound the clearance) - some at the window's very edge, some absent (0, 0, 0), some of radius 0.  The edge poses: a NaN x, a NaN and
    an infinite psi, 2^31 cells away (all four: (0, NaN)), 2^20 cells away (off the grid: reach), just off the grid with the
    window reaching in, and windows clipped by each corner and each edge of the grid."""
    if track in _FLEETS:
        return _FLEETS[track]
    g1, grid, origin, res = _g1(track)
    H, W = grid.shape
    car = CARS[track]
    R = _reach_cells(car, res)
    hd = 0.5 * math.hypot(car[0], car[1]) / res                              # half the car's diagonal in cells
    rng = np.random.default_rng(SEEDS[track])
    B = B_FLEET
    occ = grid == 0
    free = ~occ
    near = np.zeros_like(occ)
    near[1:, :] |= free[:-1, :]; near[:-1, :] |= free[1:, :]; near[:, 1:] |= free[:, :-1]; near[:, :-1] |= free[:, 1:]
    wj, wi = np.nonzero(occ & near)
    pick = rng.integers(0, wi.size, B)
    jit = 0.5 * car[0] / res + 3
    poses = np.stack([origin[0] + (wi[pick] + 0.5 + rng.uniform(-jit, jit, B)) * res,
                      origin[1] + (wj[pick] + 0.5 + rng.uniform(-jit, jit, B)) * res, rng.uniform(-4, 4, B)], 1)
    wp = rng.integers(0, g1["x"].size, B)
    mid = np.arange(B) % 4 == 3
    poses[mid] = np.stack([g1["x"][wp], g1["y"][wp], g1["psi"][wp] + rng.uniform(-0.2, 0.2, B)], 1)[mid]
    sp = SPECIAL
    poses[sp["nan_x"], 0] = np.nan
    poses[sp["nan_psi"], 2] = np.nan
    poses[sp["inf_psi"], 2] = np.inf
    poses[sp["far31"], 0] = origin[0] + res * 2.0 ** 31
    poses[sp["far20"], 1] = origin[1] - res * 2.0 ** 20
    poses[sp["outside"], :2] = (origin[0] - res * (R // 2), origin[1] + res * (H // 2))
    lo, hi_x, hi_y, mx, my = 0.5, W - 0.5, H - 0.5, W / 2 + 0.3, H / 2 + 0.3
    for key, (ci, cj) in dict(c00=(lo, lo), c10=(hi_x, lo), c01=(lo, hi_y), c11=(hi_x, hi_y), e_lo_x=(lo, my), e_hi_x=(hi_x, my),
                              e_lo_y=(mx, lo), e_hi_y=(mx, hi_y)).items():
        poses[sp[key], :2] = (origin[0] + ci * res, origin[1] + cj * res)
    discs = []
    for b in range(B):
        k = b % 65
        with np.errstate(invalid="ignore"):
            cx, cy = np.floor((poses[b, 0] - origin[0]) / res), np.floor((poses[b, 1] - origin[1]) / res)
        if not (np.isfinite(cx) and np.isfinite(cy) and abs(cx) < 2 ** 20 and abs(cy) < 2 ** 20):
            cx, cy = W // 2, H // 2
        d = np.zeros((k, 3), np.int64)
        d[:, 2] = rng.integers(0, 5, k)
        if b % 4 == 0:                                                        # anywhere in the window, under the car too
            d[:, 0] = cx + rng.integers(-R - 3, R + 4, k)
            d[:, 1] = cy + rng.integers(-R - 3, R + 4, k)
        else:                                                                 # around the car: they bound the clearance, they cannot touch
            rho, phi = rng.uniform(hd + 6, R + 4, k), rng.uniform(0, 2 * math.pi, k)
            d[:, 0] = cx + np.rint(rho * np.cos(phi))
            d[:, 1] = cy + np.rint(rho * np.sin(phi))
        if k >= 4:
            d[0] = (cx + R, cy - R // 3, 2)                                   # straddles the window's edge column
            d[1] = (cx - R - 2, cy, 2)                                        # touches it from outside: its last column is cx - R - 1
            d[2] = (0, 0, 0)                                                  # absent
            d[3, 2] = 0                                                       # radius 0: occupies nothing
        d[:, 2] = np.minimum(d[:, 2], np.minimum.reduce([d[:, 0], d[:, 1], W - d[:, 0], H - d[:, 1]]))      # the square stays on the grid
        d[d[:, 2] < 0] = 0                                                    # (a centre off the grid: absent)
        discs.append(d.astype(np.int32))
    f = dict(grid=grid, origin=origin, res=res, poses=poses, discs=discs, car=car, R=R, tol=clr_tol(car[2], car[0], car[1], res))
    f["law_discs"] = _law(grid, origin, res, poses, car, discs)
    f["law_bare"] = _law(grid, origin, res, poses, car)
    _FLEETS[track] = f
    return f


NAN_POSES = ("nan_x", "nan_psi", "inf_psi", "far31")


# ------------------------------------------------------------------------------------------------------------ CPU
def _hand(occupied, pose_cell=(20.5, 20.5), psi=0.0, reach=0.3):
    grid = np.ones((40, 40), np.int8)
    for i, j in occupied:
        grid[j, i] = 0
    pose = np.array([[pose_cell[0] * 0.1, pose_cell[1] * 0.1, psi]])
    return grid, (0.0, 0.0), 0.1, pose, (0.45, 0.25, reach)


def test_hand_cases_at_psi_zero(twin):
    """a 40 x 40 grid of 0.1 m cells, a 0.45 x 0.25 car at the centre of cell (20, 20), psi = 0: c = 1, s = 0 in every libm"""
    def both(*a, **kw):
        w = _hand(*a, **kw)
        law = _law(*w)
        got = _twin_audit(twin, *w)
        assert not law[2][0]
        assert got[0][0] == law[0][0] and (got[1][0] == law[1][0] or (math.isnan(got[1][0]) and math.isnan(law[1][0])))
        return int(got[0][0]), float(got[1][0])

    assert both([(22, 20)]) == (1, 0.0)                                       # its centre is 0.2 ahead, the car reaches 0.225
    c, d = both([(23, 20)])
    assert c == 0 and abs(d - 0.075) <= 1e-15                                 # 0.3 - 0.225
    c, d = both([(20, 22)])
    assert c == 0 and abs(d - 0.075) <= 1e-15                                 # 0.2 - 0.125
    c, d = both([(23, 22)])
    assert c == 0 and abs(d - math.hypot(0.075, 0.075)) <= 1e-15              # the corner's Euclidean distance
    c, d = both([(23, 22), (20, 22), (25, 20)])
    assert c == 0 and abs(d - 0.075) <= 1e-15                                 # the minimum over the cells
    c, d = both([(26, 20)], reach=0.3)
    assert (c, d) == (0, 0.3)                                                 # 0.375 away: inside the window, beyond reach
    assert both([]) == (0, 0.3)                                               # an empty window
    assert both([(38, 38)]) == (0, 0.3)                                       # occupied, but outside the window
    for bad in ((math.nan, 20.5, 0.0), (20.5, math.inf, 0.0), (20.5, 20.5, math.nan)):
        c, d = both([(22, 20)], pose_cell=bad[:2], psi=bad[2])
        assert c == 0 and math.isnan(d)
    # a quarter turn swaps the axes: the cell 0.2 to the side is now ahead (c and s are not exact there: no bit claim)
    w = _hand([(20, 22)], psi=math.pi / 2)
    assert _twin_audit(twin, *w)[0][0] == 1 and _law(*w)[0][0] == 1
    # discs count as the grid does: the disc (22, 20, 1) occupies the cells (21 .. 22, 19 .. 20) with dx^2 + dy^2 <= 1
    grid, origin, res, pose, car = _hand([])
    assert _twin_audit(twin, grid, origin, res, pose, car, [[(23, 20, 1)]])[0][0] == 1      # cell (22, 20) is in it
    got = _twin_audit(twin, grid, origin, res, pose, car, [[(24, 21, 1)]])                   # cells (23, 21), (24, 20), (24, 21), (23, 20)
    assert got[0][0] == 0 and abs(got[1][0] - 0.075) <= 1e-15
    assert _twin_audit(twin, grid, origin, res, pose, car, [[(0, 0, 0), (22, 20, 0)]]) == _twin_audit(twin, grid, origin, res, pose, car)


@pytest.mark.parametrize("track", ["sim", "real"])
def test_twin_equals_the_restated_law_on_seeded_fleets(track, twin):
    f = _fleet(track)
    sp = SPECIAL
    assert f["R"] == dict(sim=24, real=9)[track] and f["poses"].shape[0] >= 2000
    for key, discs in (("law_discs", f["discs"]), ("law_bare", None)):
        law = f[key]
        got = _twin_audit(twin, f["grid"], f["origin"], f["res"], f["poses"], f["car"], discs)
        left_out = _compare(got, law[:2], law[2], f["tol"])
        print("%s %s: cars left out by the tie rule: %d of %d" % (track, key, left_out, B_FLEET))
        assert left_out * 1000 <= B_FLEET                                     # the seeds keep the restatement within the cap
        for k in NAN_POSES:
            assert got[0][sp[k]] == 0 and math.isnan(got[1][sp[k]]), k
        assert (got[0][sp["far20"]], got[1][sp["far20"]]) == (0, f["car"][2])
        ok = ~np.isnan(got[1])
        assert ok.sum() == B_FLEET - len(NAN_POSES)
        # ... and the fleet proves something: contacts, non-contacts, cars with nothing within reach
        n_contact, n_free, n_reach = int(got[0][ok].sum()), int((got[0][ok] == 0).sum()), int((got[1][ok] == f["car"][2]).sum())
        print("contacts %d, non-contacts %d, at reach %d" % (n_contact, n_free, n_reach))
        assert n_contact * 10 >= B_FLEET and n_free * 10 >= B_FLEET and n_reach >= 1
        assert np.all(got[1][ok][got[0][ok] == 1] == 0.0) and np.all(got[1][ok][got[0][ok] == 0] > 0.0)
        assert np.all(got[1][ok] <= f["car"][2])
    # the discs are seen, and the cases are what they claim to be
    with_d, bare = f["law_discs"], f["law_bare"]
    assert np.sum(with_d[0] != bare[0]) >= 20 and np.sum(with_d[1] < bare[1]) >= 100
    assert sorted({len(d) for d in f["discs"]}) == list(range(65))
    assert any(np.any((d[:, 2] == 0) & (d[:, 0] > 0)) for d in f["discs"])   # a zero-radius disc that is not the absent one
    H, W = f["grid"].shape
    cells = np.floor((f["poses"][:, :2] - np.array(f["origin"])) / f["res"])
    for k, want in dict(c00=(0, 0), c10=(W - 1, 0), c01=(0, H - 1), c11=(W - 1, H - 1)).items():
        assert tuple(cells[sp[k]]) == want, k
    assert cells[sp["outside"], 0] < 0 and cells[sp["outside"], 0] + f["R"] >= 0


def test_footprint_fields_and_drop_in(twin):
    from footprint import Footprint
    from MPC import BatchMPC
    fp = Footprint(0.12, 0.06)
    assert (fp.length, fp.width, fp.reach, fp.stop, fp.mode) == (0.12, 0.06, 0.12, False, 1)
    fp2 = Footprint(0.3, 0.2, reach=0.5, stop=True)
    assert (fp2.length, fp2.width, fp2.reach, fp2.stop, fp2.mode) == (0.3, 0.2, 0.5, True, 2)
    assert hasattr(Footprint, "audit") and hasattr(Footprint, "audit_batch")
    assert hasattr(mpmpc.Handle, "rollout_set_audit") and hasattr(mpmpc.Handle, "rollout_audit") and hasattr(mpmpc, "footprint_audit")
    assert hasattr(BatchMPC, "rollout_audit")
    m, rp, car = T.build_world(obstacles=False)
    fp = Footprint(car.length, car.width)
    if mpmpc.device_count() == 0:                                             # no CPU fallback: an error, never a result
        with pytest.raises(mpmpc.MpmpcError, match="rc=%d" % E_HIP):
            fp.audit(car, m)
        return
    st = car.temporal_state
    want = _twin_audit(twin, np.ascontiguousarray(m.data), tuple(m.origin), m.resolution, [[st.x, st.y, st.psi]],
                       (fp.length, fp.width, fp.reach))
    contact, clearance = fp.audit(car, m)
    assert contact == bool(want[0][0]) and abs(clearance - want[1][0]) <= clr_tol(fp.reach, fp.length, fp.width, m.resolution)
    assert (fp.contact, fp.clearance) == (contact, clearance) and not contact and 0 < clearance <= fp.reach


def test_argument_checks_through_the_abi_without_device(built_library, twin):
    lib = mpmpc.load_library(built_library)
    grid = np.ones((40, 50), np.int8)
    pose = np.array([[0.1, 0.1, 0.3], [0.2, 0.1, 0.3]])
    contact, clearance = np.zeros(2, np.int32), np.zeros(2)

    def call(length=0.12, width=0.06, reach=0.1, off=None, discs=None, res=0.01, B=2, data=grid, con=contact):
        off = None if off is None else np.ascontiguousarray(off, np.int32)
        discs = None if discs is None else np.ascontiguousarray(discs, np.int32)
        gp = None if data is None else data.ctypes.data_as(bp)
        R = C.c_int32(-1)
        rc = lib.mpmpc_footprint_audit(0, 40, 50, gp, 0.0, 0.0, res, B, _d(pose), _i(off), _i(discs), length, width, reach, _i(con),
                                       _d(clearance))
        rc2 = twin.fp_emu_check(40, 50, gp, res, B, _d(pose), _i(off), _i(discs), length, width, reach, _i(con), _d(clearance), C.byref(R))
        assert rc2 == (rc if rc == E_ARG else 0)                              # the twin runs the same checks
        return rc, lib.mpmpc_last_error(), R.value

    def refused(word, **kw):
        rc, why, _ = call(**kw)
        assert rc == E_ARG and word in why, (kw, rc, why)

    for v in (0.0, -1.0, np.inf, np.nan):
        refused(b"length", length=v)
        refused(b"width", width=v)
        refused(b"reach must", reach=v)
    refused(b"256 cells", reach=2.5)                                          # R = 257
    refused(b"256 cells", length=5.0, width=1.0, reach=0.1)                   # the diagonal alone
    refused(b"256 cells", reach=1e300)
    refused(b"offsets[0]", off=[1, 1, 1], discs=[[5, 5, 1]])
    refused(b"decrease", off=[0, 2, 1], discs=[[5, 5, 1]] * 2)
    refused(b"64 discs", off=[0, 65, 65], discs=[[5, 5, 1]] * 65)
    refused(b"discs is NULL", off=[0, 1, 1])
    refused(b"leaves the map", off=[0, 1, 1], discs=[[2, 5, 3]])
    refused(b"leaves the map", off=[0, 0, 1], discs=[[48, 5, 3]])
    refused(b"negative radius", off=[0, 0, 1], discs=[[10, 5, -1]])
    refused(b"B must", B=0)
    refused(b"resolution", res=0.0)
    refused(b"NULL", data=None)
    refused(b"NULL", con=None)
    assert lib.mpmpc_rollout_set_audit(None, 1, 0.12, 0.06, 0.1) == E_ARG     # no handle
    assert lib.mpmpc_rollout_audit(None, 2, None, None, None, None, None, None) == E_ARG
    # what passes the checks reaches the device call: without a device that is an error of another kind, never a result
    rc, why, R = call(reach=2.49, off=[0, 64, 64], discs=[[5, 5, 5]] * 64)    # R = 256 and 64 discs: the caps themselves
    assert rc != E_ARG and R == 256
    if mpmpc.device_count() == 0:
        assert rc == E_HIP and why != b""


# ------------------------------------------------------------------------------------------------------------ GPU
def _device(f, sl, car=None, discs=True):
    return mpmpc.footprint_audit(f["grid"], f["origin"], f["res"], f["poses"][sl], *(car or f["car"]),
                                 discs=f["discs"][sl] if discs else None)


@pytest.mark.gpu
@pytest.mark.parametrize("track", ["sim", "real"])
def test_device_equals_the_twin_on_seeded_fleets(track, twin):
    f = _fleet(track)
    left_out = total = 0
    for B in (1, 63, 64, 65, 257):                                            # (the edge poses are cars 33 .. 47)
        sl = slice(0, B)
        for key, with_discs in (("law_discs", True), ("law_bare", False)):
            want = _twin_audit(twin, f["grid"], f["origin"], f["res"], f["poses"][sl], f["car"], f["discs"][sl] if with_discs else None)
            got = _device(f, sl, discs=with_discs)
            assert got[0].dtype == np.int32 and got[0].shape == (B,) and got[1].shape == (B,)
            left_out += _compare(got, want, f[key][2][sl], f["tol"])
            total += B
            again = _device(f, sl, discs=with_discs)
            assert np.array_equal(got[0], again[0]) and np.array_equal(got[1], again[1], equal_nan=True)      # device against device
    assert left_out * 1000 <= total
    got = _device(f, slice(0, 257))
    for k in NAN_POSES:
        assert got[0][SPECIAL[k]] == 0 and math.isnan(got[1][SPECIAL[k]]), k
    assert np.isfinite(np.delete(got[1], [SPECIAL[k] for k in NAN_POSES])).all()
    assert got[0].sum() >= 25 and (got[0] == 0).sum() >= 25


@pytest.mark.gpu
@pytest.mark.parametrize("track,car,R,B", [("real", (0.04, 0.03, 0.05), 2, 257),        # a car smaller than a cell
                                           ("sim", (0.12, 0.06, 0.12), 38, 257),        # the stock car and its default reach
                                           ("sim", (0.5, 0.06, 0.4), 131, 65),
                                           ("sim", (0.12, 0.06, 1.21), 256, 63)])       # the cap: every window is clipped
def test_device_equals_the_twin_across_window_sizes(track, car, R, B, twin):
    f = _fleet(track)
    assert _reach_cells(car, f["res"]) == R and (2 * R + 1) % 64 != 0
    sl = slice(0, B)
    _, _, tie = _law(f["grid"], f["origin"], f["res"], f["poses"][sl], car, f["discs"][sl])
    want = _twin_audit(twin, f["grid"], f["origin"], f["res"], f["poses"][sl], car, f["discs"][sl])
    got = _device(f, sl, car=car)
    left_out = _compare(got, want, tie, clr_tol(car[2], car[0], car[1], f["res"]))
    assert left_out <= 1
    again = _device(f, sl, car=car)
    assert np.array_equal(got[0], again[0]) and np.array_equal(got[1], again[1], equal_nan=True)
    ok = ~np.isnan(got[1])
    assert (got[0][ok] == 0).any() and (R == 2 or got[0][ok].any())


# ---- the audit inside a rollout
B_RO, N_RO, STEPS = 16, 10, 40
STOCK = (0.12, 0.06, 0.12)
LONG = (0.5, 0.06, 0.12)             # longer than the track is wide: contact in corners, none on straights
CHASED = (2, 3, 4)                   # cars with a mover that catches up with them from behind
COVERED = 1                          # the car with a static disc over its start pose


def _world(traffic=True):
    """a handle on Sim_Track with B cars, and per car 2 static discs, 2 movers along the path and (traffic) one group; car
    COVERED starts under a static disc, the cars CHASED have a mover 0.15 m behind them that gains on them"""
    import test_traffic as TT
    g1, grid, origin, res = _g1("sim")
    B, N = B_RO, N_RO
    h, _ = TT._handle("sim", N, B)
    rng = np.random.default_rng(79)
    cum = np.cumsum(g1["segment_lengths"])
    starts = (np.arange(B) * 11 + 3) % g1["x"].size
    poses = np.stack([g1["x"][starts], g1["y"][starts], g1["psi"][starts] + rng.uniform(-0.05, 0.05, B)], 1)
    m = Map.from_grid(grid, origin, res)
    static = [m.obstacle_discs([Obstacle(x + rng.uniform(-0.05, 0.05), y + rng.uniform(-0.05, 0.05), r)
                                for x, y, r in (TT.BASE["sim"][q] for q in rng.choice(len(TT.BASE["sim"]), 2, replace=False))])
              for _ in range(B)]
    static[COVERED][0] = m.obstacle_discs([Obstacle(poses[COVERED, 0], poses[COVERED, 1], 0.02)])[0]
    rows = [np.array([(1, 6, cum[(starts[b] + 8 + 9 * q) % cum.size], rng.uniform(-0.08, 0.08), 0.004, 0.0) for q in range(2)])
            for b in range(B)]
    for b in CHASED:
        rows[b][0] = (1, 6, cum[starts[b]] - 0.15, 0.0, 0.08, 0.0)
    return dict(h=h, grid=grid, origin=origin, res=res, g1=g1, cum=cum, starts=starts, poses=poses, static=static, rows=rows,
                group=np.zeros(B, np.int32), rad=np.full(B, 7, np.int32), slots=3, traffic=traffic, B=B, N=N)


def _run(mode, car=STOCK, world="all", calls=(STEPS,)):
    """one recorded rollout -> dict(w, state, trace, audit (None for mode 0))"""
    w = _world(traffic=world == "all")
    h = w["h"]
    if world != "shared":
        h.rollout_set_obstacles(w["static"])
        h.rollout_set_movers(w["rows"])
        if w["traffic"]:
            h.rollout_set_traffic(w["group"], w["rad"], w["slots"], -1)
    h.rollout_record(STEPS, B=w["B"])
    h.rollout_set_audit(mode, *car)
    h.rollout_init(TS, w["cum"], w["cum"][w["starts"]], w["poses"])
    for n in calls:
        h.rollout_step(n)
    out = dict(w=w, state=h.rollout_state(), trace=h.rollout_trace(), audit=h.rollout_audit() if mode else None, world=world, car=car)
    h.close()
    w["h"] = None
    return out


@pytest.fixture(scope="module")
def runs():
    """computed once, shared by the rollout tests"""
    return dict(audit=_run(1), off=_run(0), single=_run(1, calls=(1,) * STEPS), mixed=_run(1, calls=(7, 1, 12, 20)),
                shared=_run(1, car=LONG, world="shared"), stop=_run(2, world="no traffic"), stop_off=_run(0, world="no traffic"))


def _teacher_forced(r, twin):
    """The accumulators as they follow from the trace alone: for every recorded step k each car's world rebuilt on the host,
    the twin on the recorded pose.  -> (dict of the six accumulators, cars the tie rule leaves out [B] bool, min_step
    unambiguous [B] bool)"""
    import movers
    import traffic
    w, tr, car = r["w"], r["trace"], r["car"]
    B, (H, W), g1 = w["B"], w["grid"].shape, w["g1"]
    reach = car[2]
    tol = clr_tol(reach, car[0], car[1], w["res"])
    acc = dict(contact_steps=np.zeros(B, np.int32), first_contact=np.full(B, -1, np.int32), min_clearance=np.full(B, reach),
               min_step=np.full(B, -1, np.int32), last_contact=np.zeros(B, np.int32), last_clearance=np.full(B, np.nan))
    tie_any = np.zeros(B, bool)
    clr = np.full((STEPS, B), np.inf)
    assert tr["pose"].shape[0] == STEPS
    for k in range(STEPS):
        pose, a = tr["pose"][k], tr["alive"][k]
        audited = np.isfinite(pose[:, 0]) & (a != 0) & (a != -2)              # running when the step began and after localisation
        discs = None
        if r["world"] != "shared":
            lists = []
            tf = traffic.trace_discs(tr, k, w["group"], w["rad"], w["slots"], -1, w["origin"], w["res"], W, H) if w["traffic"] else None
            for b in range(B):
                mv = movers.mover_discs_rows(w["rows"][b], float(k), w["origin"], w["res"], W, H, cum=w["cum"], x=g1["x"], y=g1["y"],
                                             psi=g1["psi"], circular=True)
                lists.append(np.concatenate([w["static"][b], mv] + ([tf[b]] if tf is not None else [])))
            discs = lists
        p = np.where(audited[:, None], pose, 0.0)
        p[~audited] = w["poses"][~audited]                                    # (any finite pose: the verdict is not used)
        con, cl = _twin_audit(twin, w["grid"], w["origin"], w["res"], p, car, discs)
        _, _, tie = _law(w["grid"], w["origin"], w["res"], p, car, discs)
        tie_any |= tie & audited
        for b in np.nonzero(audited)[0]:
            acc["last_contact"][b], acc["last_clearance"][b] = con[b], cl[b]
            clr[k, b] = cl[b]
            if con[b]:
                acc["contact_steps"][b] += 1
                if acc["first_contact"][b] < 0:
                    acc["first_contact"][b] = k
            if cl[b] < acc["min_clearance"][b]:
                acc["min_clearance"][b], acc["min_step"][b] = cl[b], k
    # min_step is the argmin of clearances that two implementations give to within tol: it is compared where the smallest
    # is clear of the runner-up (or ties with it exactly, as the zeros of contact steps do)
    srt = np.sort(np.minimum(clr, reach), 0)
    unambiguous = (srt[1] - srt[0] > 2 * tol) | (srt[1] == srt[0])
    return acc, tie_any, unambiguous, tol


def _same_accumulators(got, want, keep, unambiguous, tol):
    for k in ("contact_steps", "first_contact", "last_contact"):
        assert np.array_equal(got[k][keep], want[k][keep]), (k, got[k], want[k])
    for k in ("min_clearance", "last_clearance"):
        a, b = got[k][keep], want[k][keep]
        assert np.array_equal(np.isnan(a), np.isnan(b)), k
        assert np.all(np.abs(a - b)[~np.isnan(a)] <= tol), (k, a, b)
    assert np.array_equal(got["min_step"][keep & unambiguous], want["min_step"][keep & unambiguous]), (got["min_step"], want["min_step"])


@pytest.mark.gpu
def test_rollout_audit_teacher_forced(runs, twin):
    r = runs["audit"]
    want, tie, unamb, tol = _teacher_forced(r, twin)
    got = r["audit"]
    assert sorted(got) == sorted(ACC) and all(got[k].shape == (B_RO,) for k in ACC)
    print({k: got[k].tolist() for k in ACC})
    assert tie.sum() == 0 and unamb.sum() >= B_RO - 1                         # the cap: 16 cars x 40 steps leave room for none
    _same_accumulators(got, want, ~tie, unamb, tol)
    # the scenario bites: contact after the start, no contact at all, a closest approach that is not the last step
    assert np.any(got["first_contact"] >= 1) and np.any(got["first_contact"] == -1) and np.any(got["contact_steps"] == 0)
    assert got["first_contact"][COVERED] == 0 and all(got["first_contact"][b] >= 1 for b in CHASED)
    assert np.any((got["min_step"] >= 0) & (got["min_step"] != STEPS - 1))
    assert np.all(got["min_clearance"] <= STOCK[2]) and np.all((got["min_step"] == -1) == (got["min_clearance"] == STOCK[2]))
    assert np.all((got["contact_steps"] > 0) == (got["first_contact"] >= 0)) and np.all((got["contact_steps"] > 0) == (got["min_clearance"] == 0))
    # all three kinds of disc were in the audited worlds
    kinds = r["w"]
    assert all(len(s) == 2 for s in kinds["static"]) and all(len(m) == 2 for m in kinds["rows"]) and kinds["traffic"]
    # ... and once more with the shared table only: the base map, a footprint longer than the track is wide
    r = runs["shared"]
    want, tie, unamb, tol = _teacher_forced(r, twin)
    got = r["audit"]
    print({k: got[k].tolist() for k in ACC})
    assert tie.sum() == 0
    _same_accumulators(got, want, ~tie, unamb, tol)
    assert np.any(got["min_clearance"] < LONG[2])


@pytest.mark.gpu
def test_one_call_equals_the_step_by_step_loop(runs):
    a = runs["audit"]
    for other in ("single", "mixed"):
        b = runs[other]
        for k in ACC:
            assert np.array_equal(a["audit"][k], b["audit"][k], equal_nan=True), (other, k)
        for k in a["trace"]:
            assert np.array_equal(a["trace"][k], b["trace"][k], equal_nan=True), (other, k)


@pytest.mark.gpu
def test_the_audit_does_not_disturb_a_run(runs):
    a, b = runs["audit"], runs["off"]
    assert sorted(a["state"]) == sorted(b["state"]) and sorted(a["trace"]) == sorted(b["trace"])
    for k in a["state"]:
        assert np.array_equal(a["state"][k], b["state"][k], equal_nan=True), k
    for k in a["trace"]:
        assert np.array_equal(a["trace"][k], b["trace"][k], equal_nan=True), k
    assert np.any(a["state"]["alive"] == 1) and not np.any(a["state"]["alive"] == -5)
    assert np.any(a["audit"]["contact_steps"] > 0)                            # (there was something to disturb it with)


@pytest.mark.gpu
def test_mode_two_ends_a_car_in_contact(runs):
    a, b = runs["stop"], runs["stop_off"]
    aud, alive, tr = a["audit"], a["state"]["alive"], a["trace"]
    hit = aud["first_contact"] >= 0
    assert hit[COVERED] and all(hit[c] for c in CHASED) and (~hit).sum() >= 4
    for c in np.nonzero(hit)[0]:
        fc = aud["first_contact"][c]
        assert alive[c] == -5 and aud["contact_steps"][c] == 1 and aud["last_contact"][c] == 1 and aud["min_step"][c] == fc
        assert tr["alive"][fc, c] == -5 and (fc == 0 or tr["alive"][fc - 1, c] == 1)
        assert np.array_equal(a["state"]["pose"][c], tr["pose"][fc, c])      # frozen where the contact was found ...
        assert np.all(np.isnan(tr["pose"][fc + 1:, c])) and np.all(tr["alive"][fc:, c] == -5)      # ... and off the record from there
    assert not np.any(alive[~hit] == -5) and np.any(alive[~hit] == 1)
    # a car that was never in contact drove exactly as without the audit (no traffic: the cars do not see each other)
    for k in a["state"]:
        assert np.array_equal(a["state"][k][~hit], b["state"][k][~hit], equal_nan=True), k
    for k in tr:
        assert np.array_equal(tr[k][:, ~hit], b["trace"][k][:, ~hit], equal_nan=True), k
    assert not np.any(b["state"]["alive"] == -5)


@pytest.mark.gpu
def test_rollout_audit_state_errors_and_batch_mpc():
    import test_traffic as TT
    from footprint import Footprint
    from MPC import BatchMPC
    from scipy import sparse
    g1, grid, origin, res = _g1("sim")
    h, tabs = TT._handle("sim", N_RO, 4)
    cum = np.cumsum(g1["segment_lengths"])
    starts = np.arange(4) * 20
    poses = np.stack([g1["x"][starts], g1["y"][starts], g1["psi"][starts]], 1)
    h.rollout_init(TS, cum, cum[starts], poses)
    with pytest.raises(mpmpc.MpmpcError, match="error %d" % E_STATE):        # the audit is off
        h.rollout_audit()
    with pytest.raises(mpmpc.MpmpcError, match="error %d" % E_ARG):
        h.rollout_set_audit(1, 0.12, 0.06, 5.0)                               # 1 000 cells on this map
    with pytest.raises(mpmpc.MpmpcError, match="error %d" % E_ARG):
        h.rollout_set_audit(3, 0.12, 0.06, 0.1)
    h.rollout_set_audit(1, *STOCK)                                            # mid-run: audited from here on
    first = h.rollout_audit()
    assert np.all(first["min_clearance"] == STOCK[2]) and np.all(first["min_step"] == -1) and np.all(np.isnan(first["last_clearance"]))
    h.rollout_step(2)
    h.rollout_init(TS, cum[:], cum[starts[:3]], poses[:3])                    # the setting persists, the accumulators start over
    again = h.rollout_audit()
    assert again["min_step"].shape == (3,) and np.all(again["min_step"] == -1) and np.all(again["contact_steps"] == 0)
    h.rollout_step(3)
    got = h.rollout_audit()
    assert np.all(got["last_clearance"] > 0) and np.all(got["min_step"] <= 2) and np.all(got["last_clearance"] >= got["min_clearance"])
    h.rollout_set_audit(0)
    h.rollout_step(1)
    with pytest.raises(mpmpc.MpmpcError, match="error %d" % E_STATE):
        h.rollout_audit()
    h.close()
    # a handle without a map: the step is refused, not the setting
    tr = TT.scenarios.sim_track()
    h2 = mpmpc.Handle(TT.T.stock_config(N_RO, max_batch=2), mpmpc.default_settings())
    h2.set_path(tr.kappa, tr.v_ref, tr.ds_next)
    h2.set_path_geometry(g1["x"], g1["y"], g1["psi"], g1["border_ub"], g1["border_lb"])
    h2.set_corridor(tabs[0], tabs[1])
    h2.rollout_set_audit(1, *STOCK)
    h2.rollout_init(TS, cum, cum[starts[:2]], poses[:2])
    with pytest.raises(mpmpc.MpmpcError, match="error %d.*set_map" % E_STATE):
        h2.rollout_step(1)
    h2.rollout_set_audit(0)
    h2.rollout_step(1)
    h2.close()
    # BatchMPC: the audit as an argument of rollout
    m, rp, car = T.build_world(obstacles=False)
    Q, R, QN = sparse.diags([1.0, 0.0, 0.0]), sparse.diags([0.5, 0.0]), sparse.diags([1.0, 0.0, 0.0])
    ic = {'umin': np.array([0.0, -np.tan(0.66) / car.length]), 'umax': np.array([1.0, np.tan(0.66) / car.length])}
    sc = {'xmin': np.array([-np.inf] * 3), 'xmax': np.array([np.inf] * 3)}
    B = 4
    bm = BatchMPC(car, N_RO, Q, R, QN, sc, ic, 4.0, max_batch=B, corridor="device")
    cum = np.cumsum(rp.segment_lengths)
    poses = np.array([[rp.waypoints[w].x, rp.waypoints[w].y, rp.waypoints[w].psi] for w in starts])
    plain = bm.rollout(cum[starts], poses, 5)
    assert "audit" not in plain
    fp = Footprint(car.length, car.width, stop=True)
    out = bm.rollout(cum[starts], poses, 5, audit=fp, obstacles=[[Obstacle(poses[b, 0], poses[b, 1], 0.02)] if b == 2 else [] for b in range(B)])
    assert sorted(out["audit"]) == sorted(ACC) and out["audit"]["first_contact"].tolist() == [-1, -1, 0, -1]
    assert out["alive"].tolist() == [1, 1, -5, 1] and np.array_equal(out["pose"][2], poses[2])
    assert all(np.array_equal(bm.rollout_audit()[k], out["audit"][k], equal_nan=True) for k in ACC)
    again = bm.rollout(cum[starts], poses, 5)                                 # a later rollout is unaudited again
    assert all(np.array_equal(again[k], plain[k]) for k in plain)
    with pytest.raises(mpmpc.MpmpcError, match="error %d" % E_STATE):
        bm.rollout_audit()
    bm.close()
