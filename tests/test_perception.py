"""Perceived worlds in the rollout (K0s, mpmpc_perception_scan / mpmpc_rollout_set_perception / mpmpc_rollout_perception): plan
on what the lidar saw.

CPU: a numpy restatement of the law, written here from the header csrc/perception_core.hpp (and lidar_core / wall_core beneath
it), against the host twin of K0s (tests/emul_perception, the same headers) on seeded fleets and on scenes built by hand; the
knowledge law on hand-made sequences; the argument checks through the C ABI; Perception's and BatchMPC.rollout's arguments.
GPU: the device against the twin, one multi-step call against the step-by-step loop that perceives on the host, blind cars,
off means off, state errors, drop-in use.

THE TIE RULE.  A slot's verdict comes from atan2 through the cells' beam intervals, and numpy, glibc and the device each have
their own.  A slot is TIE-DEPENDENT when its verdict changes if every cell interval is widened, or narrowed, by TIE = 1e-9 rad
(best[] recomputed); so is every slot of a scan that test_lidar's rule calls tie-sensitive as a whole (an angle within TIE of
the +-pi wrap).  Such slots are left out of every comparison between two libms - a condition computed by the restatement alone,
not a measurement - and the seeds are such that it leaves out at most 1 % of the slots that lie in some window.  Ranges are
compared as tests/test_lidar.py compares them.  Device against device has no exclusions."""
import ctypes as C
import math

import numpy as np
import pytest

import mpmpc
import mpmpc_testlib as T
import test_lidar as TL
import twins
from map import line_aa

bp = C.POINTER(C.c_int8)
u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
E_ARG, E_STATE = -1, -3
TIE = 1e-9
TS = 0.05
_d, _i, _g1, _angles = T._d, T._i, T.g1_world, TL._angles


# -------------------------------------------------------------------------------------------------------- the twin
@pytest.fixture(scope="module")
def twin():
    """The CPU twin of K0s (tests/emul_perception)."""
    return twins.perception()


@pytest.fixture(scope="module")
def car_twin():
    """The CPU twin of K0c (tests/emul_car), for test_traffic's Fleet and rows."""
    return twins.car()


def _twin_scan(twin, grid, origin, res, poses, angles, rng, discs=None, walls=None):
    poses = np.ascontiguousarray(poses, float).reshape(-1, 3)
    B = poses.shape[0]
    ang = np.ascontiguousarray(angles, float)
    off, flat = T.csr(discs, 3, n=B)
    woff, wflat = T.csr(walls, 4, n=B)
    out, ds, ws = np.full((B, ang.size), -7.0), np.zeros(B, np.uint64), np.zeros(B, np.uint32)
    rc = twin.per_emu_scan(grid.shape[0], grid.shape[1], grid.ctypes.data_as(bp), origin[0], origin[1], res, B, _d(poses), _i(off),
                           _i(flat), _i(woff), _i(wflat), ang.size, _d(ang), float(rng), _d(out), ds.ctypes.data_as(u64p),
                           ws.ctypes.data_as(u32p))
    assert rc == 0
    return out, ds, ws


# ------------------------------------------------------------------------------- the law, restated from the headers
def _wall_cells(wall):
    """wall_core.hpp step 1: the cells of a wall are line_aa's, with the coverage skimage gives them"""
    xs, ys, val = line_aa(int(wall[0]), int(wall[1]), int(wall[2]), int(wall[3]))
    return np.asarray(xs), np.asarray(ys), np.asarray(val, float)


def _scene(grid, origin, res, pose, rng, discs, walls):
    """Steps 1 - 3 of lidar_core.hpp without the beams, in the world grid + discs + walls, and who occupies what: None for a
    NaN row, else dict over the occupied in-range cells: ii, jj, d2, mn, mx, raw, a, on_grid [c], member [slots, c] (disc
    slots first, then wall slots), and per slot whether it has a cell in the window / lies across the window's edge"""
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
    discs = np.asarray(discs if discs is not None else [], np.int64).reshape(-1, 3)
    walls = np.asarray(walls if walls is not None else [], np.int64).reshape(-1, 4)
    nd, nw = discs.shape[0], walls.shape[0]
    hh, ww = max(j1 - j0 + 1, 0), max(i1 - i0 + 1, 0)
    layers = np.zeros((nd + nw, hh, ww), bool)
    in_window, at_edge = np.zeros(nd + nw, bool), np.zeros(nd + nw, bool)
    for q, (dcx, dcy, r) in enumerate(discs.tolist()):
        if r <= 0:
            continue
        # cor_in_disc: dx, dy in [-r, r - 1] and dx^2 + dy^2 <= r^2
        xs, ys = np.arange(dcx - r, dcx + r), np.arange(dcy - r, dcy + r)
        inside = (xs[None, :] - dcx) ** 2 + (ys[:, None] - dcy) ** 2 <= r * r
        yy, xx = np.nonzero(inside)
        px, py = xs[xx], ys[yy]
        keep = (px >= i0) & (px <= i1) & (py >= j0) & (py <= j1)
        layers[q, py[keep] - j0, px[keep] - i0] = True
        in_window[q], at_edge[q] = keep.any(), keep.any() and not keep.all()
    core = np.zeros((nw, hh, ww), bool)          # per wall: the cells that are no anti-aliased neighbours
    for q, wall in enumerate(walls.tolist()):
        px, py, val = _wall_cells(wall)
        keep = (px >= i0) & (px <= i1) & (py >= j0) & (py <= j1)
        layers[nd + q, py[keep] - j0, px[keep] - i0] = True
        major = px if abs(wall[2] - wall[0]) >= abs(wall[3] - wall[1]) else py
        top = np.array([val[k] >= val[major == major[k]].max() for k in range(px.size)], bool)
        core[q, py[keep & top] - j0, px[keep & top] - i0] = True
        in_window[nd + q], at_edge[nd + q] = keep.any(), keep.any() and not keep.all()
    out = dict(nd=nd, nw=nw, in_window=in_window, at_edge=at_edge, psi=psi)
    if hh == 0 or ww == 0:
        out.update(d2=np.zeros(0, np.int64))
        return out
    on_grid = grid[j0:j1 + 1, i0:i1 + 1] == 0
    occ = on_grid | layers.any(0)
    jj, ii = np.nonzero(occ)
    d2 = (cx - (ii + i0)) ** 2 + (cy - (jj + j0)) ** 2
    keep = np.sqrt(d2.astype(float)) < lim
    ii, jj, d2 = ii[keep], jj[keep], d2[keep]
    ks = np.array([-0.5, 0.0, 0.5])
    dx = np.broadcast_to((ii + i0 - cx)[:, None, None] + ks[None, :, None], (ii.size, 3, 3))
    dy = np.broadcast_to((jj + j0 - cy)[:, None, None] + ks[None, None, :], (ii.size, 3, 3))
    raw = (np.arctan2(dy, dx) - psi).reshape(ii.size, 9)
    a = np.where(raw < -math.pi, -np.mod(math.pi + raw, 2 * math.pi) + math.pi, np.mod(math.pi + raw, 2 * math.pi) - math.pi)
    out.update(d2=d2, mn=a.min(1) if ii.size else np.zeros(0), mx=a.max(1) if ii.size else np.zeros(0), raw=raw, a=a,
               on_grid=on_grid[jj, ii], member=layers[:, jj, ii], core=core[:, jj, ii])
    return out


def _see(s, angles, rng, res, widen=0.0):
    """perception_core.hpp, SEEING, with every cell interval widened by `widen` (negative: narrowed) -> (ranges [n],
    seen [slots] bool, hit [c, n], best [n])"""
    n = angles.size
    if s is None:
        return np.full(n, np.nan), np.zeros(0, bool), None, None
    seen = np.zeros(s["nd"] + s["nw"], bool)
    out = np.full(n, float(rng))
    if s["d2"].size == 0:
        return out, seen, None, None
    mn, mx = s["mn"] - widen, s["mx"] + widen
    skip = (mn < -math.pi / 2) & (mx > math.pi / 2)
    hit = (~skip)[:, None] & (mn[:, None] <= angles[None, :]) & (angles[None, :] <= mx[:, None])
    big = np.iinfo(np.int64).max
    best = np.where(hit, s["d2"][:, None], big).min(0)
    out[best < big] = np.sqrt(best[best < big].astype(float)) * res
    owns = np.any(hit & (s["d2"][:, None] == best[None, :]), 1)               # the cell is a nearest hit cell of some beam
    seen = np.any(s["member"] & owns[None, :], 1)
    return out, seen, hit, best


def _whole_tie(s):
    if s is None or s["d2"].size == 0:
        return False
    return bool(np.abs(s["raw"] + math.pi).min() <= TIE or np.abs(np.abs(s["a"]) - math.pi).min() <= TIE)


def _law(scenes, angles, rng, res):
    """-> ranges [B, n], seen (list of bool [slots_b]), tie-dependent slots (list), tie-sensitive beams [B, n]"""
    ranges, seen, tie, beam_tie = [], [], [], []
    for s in scenes:
        r, sn, _, _ = _see(s, angles, rng, res)
        wide, narrow = _see(s, angles, rng, res, TIE)[1], _see(s, angles, rng, res, -TIE)[1]
        t = (sn != wide) | (sn != narrow)
        if _whole_tie(s):
            t[:] = True
        ranges.append(r)
        seen.append(sn)
        tie.append(t)
        if s is None or s["d2"].size == 0:
            beam_tie.append(np.zeros(angles.size, bool))
        else:
            c = dict(d2=s["d2"], mn=s["mn"], mx=s["mx"], skip=(s["mn"] < -math.pi / 2) & (s["mx"] > math.pi / 2), raw=s["raw"], a=s["a"])
            beam_tie.append(TL._beams(c, angles, rng, res)[1])
    return np.array(ranges), seen, tie, np.array(beam_tie)


def _bits(mask, n):
    return np.array([(int(mask) >> q) & 1 for q in range(n)], bool)


# ------------------------------------------------------------------------------------------------ the seeded fleets
_FLEETS = {}


def _fleet(track):
    """test_lidar._fleet - B = 67, 0 .. 64 discs per car, the NaN, far and edge poses - plus 0 .. 16 walls per car around it"""
    if track in _FLEETS:
        return _FLEETS[track]
    f = dict(TL._fleet(track))
    H, W = f["grid"].shape
    rng = np.random.default_rng(911 if track == "sim" else 912)
    R = int(f["range"] / f["res"])
    walls = []
    for b in range(TL.B_FLEET):
        k = b % 17
        with np.errstate(invalid="ignore"):
            cx, cy = np.floor((f["poses"][b, 0] - f["origin"][0]) / f["res"]), np.floor((f["poses"][b, 1] - f["origin"][1]) / f["res"])
        if not (np.isfinite(cx) and np.isfinite(cy) and abs(cx) < 2 ** 20 and abs(cy) < 2 ** 20):
            cx, cy = W // 2, H // 2
        a = np.stack([cx + rng.integers(-R - 3, R + 4, k), cy + rng.integers(-R - 3, R + 4, k)], 1)
        w = np.concatenate([a, a + rng.integers(-R, R + 1, (k, 2))], 1)
        w[:, 0::2] = np.clip(w[:, 0::2], 1, W - 2)
        w[:, 1::2] = np.clip(w[:, 1::2], 1, H - 2)
        walls.append(np.ascontiguousarray(w, np.int32).reshape(-1, 4))
    f["walls"] = walls
    f["scenes"] = [_scene(f["grid"], f["origin"], f["res"], f["poses"][b], f["range"], f["discs"][b], walls[b]) for b in range(TL.B_FLEET)]
    _FLEETS[track] = f
    return f


def _fleet_law(f, ang):
    """the restated law on a fleet, computed once per sensor and shared by the tests"""
    cache = f.setdefault("law", {})
    if ang.size not in cache:
        cache[ang.size] = _law(f["scenes"], ang, f["range"], f["res"])
    return cache[ang.size]


def _compare(f, ang, got_r, got_d, got_w, count=None):
    """a scan of the fleet against the restated law; -> (slots left out, slots in some window)"""
    want_r, seen, tie, beam_tie = _fleet_law(f, ang)
    TL._equal_outside_ties(got_r, want_r, beam_tie)
    left = total = 0
    for b, s in enumerate(f["scenes"]):
        nd, nw = len(f["discs"][b]), len(f["walls"][b])
        got = np.concatenate([_bits(got_d[b], 64), _bits(got_w[b], 16)])
        assert not got[nd:64].any() and not got[64 + nw:].any(), b              # no bit beyond the car's lists
        if s is None:
            assert not got.any(), b                                           # a NaN row sees nothing
            continue
        got = np.concatenate([got[:nd], got[64:64 + nw]])
        keep = ~tie[b]
        assert np.array_equal(got[keep], seen[b][keep]), (b, np.nonzero(got != seen[b])[0], np.nonzero(tie[b])[0])
        left += int((tie[b] & s["in_window"]).sum())
        total += int(s["in_window"].sum())
        if count is not None:
            _categories(f, b, s, ang, seen[b], count)
    return left, total


def _categories(f, b, s, ang, seen, count):
    """what kind of slot is each: the counts the fleet test asserts to be positive"""
    nd = s["nd"]
    discs = np.asarray(f["discs"][b]).reshape(-1, 3)
    count["absent"] += int(np.sum(discs[:, 2] == 0))
    assert not seen[:nd][discs[:, 2] == 0].any()
    count["seen"] += int(seen.sum())
    count["edge"] += int(s["at_edge"].sum())
    if s["d2"].size == 0:
        return
    _, _, hit, best = _see(s, ang, f["range"], f["res"])
    owner = hit & (s["d2"][:, None] == best[None, :])                         # [c, n]: cell c is a nearest hit cell of beam n
    own_cell = owner.any(1)
    for q in range(s["nd"] + s["nw"]):
        mine = s["member"][q]
        if not mine.any():
            continue
        if not hit[mine].any():
            count["outside_fov"] += 1
            continue
        if seen[q]:
            if q >= nd and not (s["core"][q - nd] & mine & own_cell).any():
                count["wall_by_neighbour"] += 1
            continue
        beams = hit[mine].any(0)                                              # beams that cross the slot, all won by nearer cells
        winners = owner[:, beams].any(1)
        others = np.delete(s["member"], q, 0).any(0)
        count["occluded_by_grid"] += bool((winners & s["on_grid"]).any())
        count["occluded_by_primitive"] += bool((winners & others).any())


# ------------------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("track", ["sim", "real"])
def test_twin_equals_the_restated_law_on_seeded_fleets(track, twin):
    f = _fleet(track)
    sp = f["special"]
    left = total = 0
    count = dict(seen=0, occluded_by_grid=0, occluded_by_primitive=0, outside_fov=0, edge=0, absent=0, wall_by_neighbour=0)
    for fov, reso in TL.SENSORS:
        ang = _angles(fov, reso)
        got = _twin_scan(twin, f["grid"], f["origin"], f["res"], f["poses"], ang, f["range"], f["discs"], f["walls"])
        lo, to = _compare(f, ang, *got, count=count if ang.size == 181 else None)
        left, total = left + lo, total + to
        for k in ("nan_x", "nan_psi", "inf_psi", "far31"):
            assert np.all(np.isnan(got[0][sp[k]])) and got[1][sp[k]] == 0 and got[2][sp[k]] == 0, k
        assert got[1][sp["far20"]] == 0 and got[2][sp["far20"]] == 0
    print("slots left out by the tie rule: %d of %d in some window; categories: %s" % (left, total, count))
    assert left * 100 <= total                                                # THE TIE RULE's cap (test 2)
    assert all(v > 0 for v in count.values()), count
    assert [_angles(*s).size for s in TL.SENSORS] == [1, 181, 1025]
    assert sorted({len(d) for d in f["discs"]}) == list(range(65)) and sorted({len(w) for w in f["walls"]}) == list(range(17))
    # bits 31, 32 and 63 are exercised: some car sees a slot there (any sensor)
    ang = _angles(*TL.SENSORS[2])
    _, ds, _ = _twin_scan(twin, f["grid"], f["origin"], f["res"], f["poses"], ang, f["range"], f["discs"], f["walls"])
    hi = np.bitwise_or.reduce(ds)
    assert all(len(f["discs"][b]) == 64 for b in (64,)) and int(hi) >> 32 != 0 and int(hi) & 0xffffffff != 0


def _hand(cells_free=41):
    grid = np.ones((cells_free, cells_free), np.int8)
    return grid, (0.0, 0.0), 1.0, np.array([[20.5, 20.5, 0.0]])


def test_hand_built_scenes(twin):
    grid, origin, res, pose = _hand()
    c = 20

    def both(grid, discs, walls, ang, rng=15.0):
        s = _scene(grid, origin, res, pose[0], rng, discs, walls)
        r, seen, _, _ = _see(s, ang, rng, res)
        tr, td, tw = _twin_scan(twin, grid, origin, res, pose, ang, rng, [discs], [walls])
        nd, nw = len(discs), len(walls)
        assert np.array_equal(tr[0], r)
        assert np.array_equal(np.concatenate([_bits(td[0], 64)[:nd], _bits(tw[0], 16)[:nw]]), seen)
        return r, seen
    none = np.zeros((0, 4), np.int32)
    # two primitives tying in d2 on one beam: disc A holds cell (+3, +4), disc B cell (+4, +3), both d2 = 25, and the beam at
    # the angle of their shared corner (+3.5, +3.5) lies in both intervals - at A's minimum and at B's maximum
    A, B = (c + 3, c + 5, 1), (c + 5, c + 3, 1)          # cells (+2,+5) (+3,+4) (+3,+5) and (+5,+2) (+4,+3) (+5,+3)
    ang = np.array([np.mod(math.pi + np.arctan2(3.5, 3.5), 2 * math.pi) - math.pi])      # (psi = 0: the corner's wrapped angle)
    r, seen = both(grid, np.array([A, B], np.int32), none, ang)
    assert r[0] == 5.0 and seen.tolist() == [True, True]
    r, seen = both(grid, np.array([A, (c + 6, c + 4, 1)], np.int32), none, ang)          # B one cell further out: no tie
    assert r[0] == 5.0 and seen.tolist() == [True, False]
    # one cell in two discs: both are seen; a third disc behind them is not
    ang = np.array([0.0])
    D = np.array([(c + 6, c + 1, 1), (c + 7, c, 1), (c + 9, c + 1, 2)], np.int32)        # the first two both hold cell (+6, 0)
    r, seen = both(grid, D, none, ang)
    assert r[0] == 6.0 and seen.tolist() == [True, True, False]
    # a disc cell on an occupied grid cell: the disc is seen anyway; and a wall in front of everything hides it
    g2 = grid.copy()
    g2[c, c + 6] = 0
    r, seen = both(g2, D[:1], none, ang)
    assert r[0] == 6.0 and seen.tolist() == [True]
    g2[c, c + 4] = 0                                                          # the grid alone is nearer: occluded by the grid
    r, seen = both(g2, D[:1], none, ang)
    assert r[0] == 4.0 and seen.tolist() == [False]
    wall = np.array([(c + 3, c - 4, c + 3, c + 4)], np.int32)
    r, seen = both(grid, D[:1], wall, ang)
    assert r[0] == 3.0 and seen.tolist() == [False, True]
    # absent and radius 0: never seen, whatever the beams
    r, seen = both(grid, np.array([(0, 0, 0), (c + 2, c, 0)], np.int32), none, _angles(360, 1))
    assert np.all(r == 15.0) and not seen.any()


def test_the_tie_rule():
    """the condition alone, on the restatement: at most 1 % of the slots that lie in some window are left out, and the rule
    does flag a verdict that hangs on one ulp - the two discs of the hand-built tie, which share only a corner's angle"""
    left = total = 0
    for track in ("sim", "real"):
        f = _fleet(track)
        for fov, reso in TL.SENSORS:
            _, _, tie, _ = _fleet_law(f, _angles(fov, reso))
            for b, s in enumerate(f["scenes"]):
                if s is not None:
                    left += int((tie[b] & s["in_window"]).sum())
                    total += int(s["in_window"].sum())
    print("slots left out by the tie rule: %d of %d in some window" % (left, total))
    assert total > 10000 and left * 100 <= total
    grid, origin, res, pose = _hand()
    c = 20
    ang = np.array([np.mod(math.pi + np.arctan2(3.5, 3.5), 2 * math.pi) - math.pi])
    s = _scene(grid, origin, res, pose[0], 15.0, np.array([(c + 3, c + 5, 1), (c + 5, c + 3, 1)]), None)
    _, seen, tie, _ = _law([s], ang, 15.0, res)
    assert seen[0].tolist() == [True, True] and tie[0].tolist() == [True, True]      # narrowed by 1e-9, neither cell holds the beam
    _, seen, tie, _ = _law([s], np.array([ang[0] + 0.01]), 15.0, res)
    assert seen[0].tolist() == [True, False] and not tie[0].any()                      # clear of the corner: no tie


def _sequence(twin, scanned, dseen, wseen, n_disc, n_static, n_mover, n_wall, hold, k0=0, reset_at=-1):
    T_ = len(scanned)
    sc = np.ascontiguousarray(scanned, np.int32)
    ds, ws = np.ascontiguousarray(dseen, np.uint64), np.ascontiguousarray(wseen, np.uint32)
    dk, wk = np.zeros(T_, np.uint64), np.zeros(T_, np.uint32)
    df, dl, wf, wl = (np.zeros(64, np.int32), np.zeros(64, np.int32), np.zeros(16, np.int32), np.zeros(16, np.int32))
    twin.per_emu_sequence(T_, n_disc, n_static, n_mover, n_wall, _i(sc), ds.ctypes.data_as(u64p), ws.ctypes.data_as(u32p), k0, hold,
                          reset_at, dk.ctypes.data_as(u64p), wk.ctypes.data_as(u32p), _i(df), _i(dl), _i(wf), _i(wl))
    return dk, wk, df, dl, wf, wl


def _sequence_law(scanned, dseen, wseen, n_disc, n_static, n_mover, n_wall, hold, k0=0, reset_at=-1):
    """perception_core.hpp, KNOWING, in plain Python"""
    first, last = [-1] * (n_disc + n_wall), [-1] * (n_disc + n_wall)
    dk, wk = [], []
    for t, sc in enumerate(scanned):
        k = k0 + t
        if t == reset_at:
            first, last = [-1] * (n_disc + n_wall), [-1] * (n_disc + n_wall)
        known = []
        for q in range(n_disc + n_wall):
            s = ((int(dseen[t]) >> q) & 1) if q < n_disc else ((int(wseen[t]) >> (q - n_disc)) & 1)
            if sc and s:
                last[q] = k
                if first[q] < 0:
                    first[q] = k
            if q >= n_disc or q < n_static:
                known.append(last[q] >= 0)                                    # sticky
            elif q < n_static + n_mover:
                known.append(last[q] >= 0 and k - last[q] <= hold)            # tracked
            else:
                known.append(last[q] == k)                                    # traffic
        dk.append(sum(1 << q for q in range(n_disc) if known[q]))
        wk.append(sum(1 << q for q in range(n_wall) if known[n_disc + q]))
    return dk, wk, first, last


def test_knowledge_law_on_hand_made_sequences(twin):
    # slots: 0, 1 static, 2, 3 movers, 4, 5 traffic; walls 0, 1.  Static 0 seen once at step 1, mover 2 at 1 and 2 and again
    # at 7, traffic 4 at 0, 1, 5; wall 1 at 3; the car stops scanning from step 8 on (its masks are then ignored)
    dseen = [0b010000, 0b010101, 0b000100, 0, 0, 0b010000, 0, 0b000100, 0b111111, 0b111111, 0]
    wseen = [0, 0, 0, 0b10, 0, 0, 0, 0, 0b11, 0b11, 0]
    scanned = [1] * 8 + [0] * 3
    for hold in (0, 3):
        for reset_at in (-1, 4):
            for k0 in (0, 17):
                got = _sequence(twin, scanned, dseen, wseen, 6, 2, 2, 2, hold, k0, reset_at)
                want = _sequence_law(scanned, dseen, wseen, 6, 2, 2, 2, hold, k0, reset_at)
                assert got[0].tolist() == want[0] and got[1].tolist() == want[1], (hold, reset_at, k0)
                assert got[2][:6].tolist() + got[4][:2].tolist() == want[2] and got[3][:6].tolist() + got[5][:2].tolist() == want[3]
                assert np.all(got[2][6:] == -1) and np.all(got[3][6:] == -1) and np.all(got[4][2:] == -1) and np.all(got[5][2:] == -1)
    # ... and the sequences are what they claim to be (hold = 3, no reset, k0 = 0)
    dk, wk, first, last = _sequence_law(scanned, dseen, wseen, 6, 2, 2, 2, 3)
    assert [(m >> 0) & 1 for m in dk] == [0] + [1] * 10                       # sticky from the step it is seen, also while not scanning
    assert [(m >> 1) & 1 for m in dk] == [0] * 11                             # seen only by a car that does not scan: never
    assert [(m >> 2) & 1 for m in dk] == [0, 1, 1, 1, 1, 1, 0, 1, 1, 1, 1]    # held for 3 steps, lost at 6, seen again at 7
    assert [(m >> 4) & 1 for m in dk] == [1, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0]    # traffic: only in the step it is seen
    assert [(m >> 1) & 1 for m in wk] == [0, 0, 0] + [1] * 8 and not any(m & 1 for m in wk)
    assert first[2] == 1 and last[2] == 7 and first[4] == 0 and last[4] == 5
    assert [(m >> 2) & 1 for m in _sequence_law(scanned, dseen, wseen, 6, 2, 2, 2, 0)[0]] == [0, 1, 1, 0, 0, 0, 0, 1, 0, 0, 0]
    assert _sequence_law(scanned, dseen, wseen, 6, 2, 2, 2, 3, 0, 4)[0][4] == 0          # the reset forgets the map too
    # the perceived lists: an unknown disc is (0, 0, 0), an unknown wall the empty box {1, 1, 0, 0, 0, 0}
    discs = np.array([(5, 6, 2), (9, 9, 3), (0, 0, 0)], np.int32)
    walls = np.array([(3, 4, 9, 6), (7, 2, 7, 8)], np.int32)
    od, oh = np.zeros((3, 3), np.int32), np.zeros((2, 6), np.int32)
    twin.per_emu_lists(3, _i(discs), 0b101, 2, _i(walls), 0b10, _i(od), _i(oh))
    assert od.tolist() == [[5, 6, 2], [0, 0, 0], [0, 0, 0]]
    assert oh[0].tolist() == [1, 1, 0, 0, 0, 0] and oh[1].tolist() == [6, 2, 8, 8, 7, 1]


def test_argument_checks_through_the_abi_without_device(built_library, twin):
    lib = mpmpc.load_library(built_library)
    assert {"mpmpc_perception_scan", "mpmpc_rollout_set_perception", "mpmpc_rollout_perception"} <= set(mpmpc.EXPORTS)
    for name in ("mpmpc_perception_scan", "mpmpc_rollout_set_perception", "mpmpc_rollout_perception"):
        assert hasattr(lib, name)
    grid = np.ones((40, 50), np.int8)
    pose = np.array([[0.1, 0.1, 0.3], [0.2, 0.1, 0.3]])
    ang = _angles(180, 1)
    out, ds, ws = np.zeros((2, 2048)), np.zeros(2, np.uint64), np.zeros(2, np.uint32)

    def call(n=None, angles=ang, rng=0.1, off=None, discs=None, woff=None, walls=None, res=0.01, B=2, masks=True):
        angles = np.ascontiguousarray(angles, float)
        n = angles.size if n is None else n
        off, discs, woff, walls = (None if a is None else np.ascontiguousarray(a, np.int32) for a in (off, discs, woff, walls))
        rc = lib.mpmpc_perception_scan(0, 40, 50, grid.ctypes.data_as(bp), 0.0, 0.0, res, B, _d(pose), _i(off), _i(discs), _i(woff),
                                       _i(walls), n, _d(angles), rng, _d(out), ds.ctypes.data_as(u64p) if masks else None,
                                       ws.ctypes.data_as(u32p))
        rc2 = twin.per_emu_check_scan(40, 50, grid.ctypes.data_as(bp), res, B, _d(pose), _i(off), _i(discs), _i(woff), _i(walls), n,
                                      _d(angles), rng, _d(out))
        if masks:
            assert rc2 == (rc if rc == E_ARG else 0)                          # the twin runs the same checks
        return rc, lib.mpmpc_last_error()

    def refused(word, **kw):
        rc, why = call(**kw)
        assert rc == E_ARG and word in why, (kw, rc, why)

    refused(b"n_beams", n=0)
    refused(b"n_beams", angles=np.linspace(-1, 1, 2049))
    refused(b"finite", angles=[-1.0, np.nan, 1.0])
    refused(b"ascending", angles=[-1.0, 0.5, 0.0])
    for r in (0.0, -1.0, np.inf, np.nan):
        refused(b"range", rng=r)
    refused(b"2048 cells", rng=20.49)
    refused(b"decrease", off=[0, 2, 1], discs=[[5, 5, 1]] * 2)
    refused(b"64 discs", off=[0, 65, 65], discs=[[5, 5, 1]] * 65)
    refused(b"leaves the map", off=[0, 1, 1], discs=[[2, 5, 3]])
    refused(b"negative radius", off=[0, 0, 1], discs=[[10, 5, -1]])
    refused(b"16 walls", woff=[0, 17, 17], walls=[[5, 5, 9, 9]] * 17)
    refused(b"end point", woff=[0, 1, 1], walls=[[0, 5, 9, 9]])
    refused(b"B must", B=0)
    refused(b"resolution", res=0.0)
    refused(b"seen_out", masks=False)
    rc, why = call(rng=20.48, off=[0, 64, 64], discs=[[5, 5, 5]] * 64, woff=[0, 16, 16], walls=[[5, 5, 9, 9]] * 16)      # the caps themselves
    assert rc != E_ARG
    if mpmpc.device_count() == 0:
        assert rc == -2 and why != b""
    # the two handle entry points: no handle, no device call
    assert lib.mpmpc_rollout_set_perception(None, ang.size, _d(ang), 0.3, 0) == E_ARG
    assert lib.mpmpc_rollout_set_perception(None, 0, None, 0.0, 0) == E_ARG
    assert lib.mpmpc_rollout_perception(None, 2, None, None, None, None, None, None) == E_ARG
    # ... and the setter's own checks (the library calls the same function)
    chk = lambda a, rng=0.3, hold=0, res=0.005, n=None: twin.per_emu_check_setting(len(a) if n is None else n, _d(np.ascontiguousarray(a, float)), rng, hold, res)
    assert chk(ang) == 0 and chk(ang, hold=7) == 0 and chk(ang, res=math.inf, rng=1e9) == 0
    assert chk(ang, hold=-1) == E_ARG and chk(ang, rng=0.0) == E_ARG and chk(ang, rng=10.25) == E_ARG and chk(ang, n=0) == E_ARG
    assert chk([0.0, -1.0]) == E_ARG and chk([0.0, np.nan]) == E_ARG


def test_perception_and_batch_mpc_arguments():
    from lidar_model import LidarModel
    from perception import Perception
    lm = LidarModel(FoV=180, range=0.3, resolution=1)
    p = Perception(lm, hold=2)
    assert p.hold == 2 and p.range == 0.3 and np.array_equal(p.angles, lm.measurements[0]) and p.angles.flags["C_CONTIGUOUS"]
    assert Perception(lm).hold == 0
    for bad in (-1, 1.5):
        with pytest.raises(ValueError):
            Perception(lm, hold=bad)
    with pytest.raises(TypeError):
        Perception(object())
    assert Perception.slots(0b101, 4).tolist() == [True, False, True, False] and Perception.slots(1 << 63, 64)[63]
    assert hasattr(mpmpc, "perception_scan") and hasattr(mpmpc.Handle, "rollout_set_perception") and hasattr(mpmpc.Handle, "rollout_perception")
    import inspect
    from MPC import BatchMPC
    assert inspect.signature(BatchMPC.rollout).parameters["perception"].default is None

    class NoTable:                                                            # BatchMPC with a host-made corridor: no device map
        corridor_cols = None
        _path = None
    with pytest.raises(ValueError, match="corridor='device'"):
        BatchMPC.rollout(NoTable(), np.zeros(1), np.zeros((1, 3)), 1, perception=p)


# ------------------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("track", ["sim", "real"])
def test_device_equals_the_twin_on_seeded_fleets(track, twin):
    f = _fleet(track)
    left = total = 0
    for fov, reso in TL.SENSORS:
        ang = _angles(fov, reso)
        want = _twin_scan(twin, f["grid"], f["origin"], f["res"], f["poses"], ang, f["range"], f["discs"], f["walls"])
        got = mpmpc.perception_scan(f["grid"], f["origin"], f["res"], f["poses"], ang, f["range"], f["discs"], f["walls"])
        k0l = mpmpc.lidar_scan(f["grid"], f["origin"], f["res"], f["poses"], ang, f["range"], f["discs"], walls=f["walls"])
        assert np.array_equal(got[0], k0l, equal_nan=True)                    # K0l's ranges bit for bit, everywhere
        lo, to = _compare(f, ang, *got)                                       # the law, outside the tie-dependent slots
        left, total = left + lo, total + to
        _, _, tie, _ = _fleet_law(f, ang)
        for b, s in enumerate(f["scenes"]):                                   # ... and the twin
            nd, nw = len(f["discs"][b]), len(f["walls"][b])
            keep = np.ones(nd + nw, bool) if s is None else ~tie[b]
            g = np.concatenate([_bits(got[1][b], 64)[:nd], _bits(got[2][b], 16)[:nw]])
            w = np.concatenate([_bits(want[1][b], 64)[:nd], _bits(want[2][b], 16)[:nw]])
            assert np.array_equal(g[keep], w[keep]), b
        again = mpmpc.perception_scan(f["grid"], f["origin"], f["res"], f["poses"], ang, f["range"], f["discs"], f["walls"])
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(got, again))      # device against device: no exclusions
    assert left * 100 <= total
    # discs only, walls only, neither; B = 1
    ang = _angles(*TL.SENSORS[1])
    b = 20
    one = lambda **kw: mpmpc.perception_scan(f["grid"], f["origin"], f["res"], f["poses"][b:b + 1], ang, f["range"], **kw)
    r, ds, ws = one(discs=f["discs"][b:b + 1])
    assert np.array_equal(r, mpmpc.lidar_scan(f["grid"], f["origin"], f["res"], f["poses"][b:b + 1], ang, f["range"], f["discs"][b:b + 1]))
    assert ws[0] == 0 and ds[0] != 0
    r, ds, ws = one(walls=f["walls"][b + 13:b + 14])
    assert ds[0] == 0
    r, ds, ws = one()
    assert ds[0] == 0 and ws[0] == 0 and np.array_equal(r, mpmpc.lidar_scan(f["grid"], f["origin"], f["res"], f["poses"][b:b + 1], ang, f["range"]))


N10 = 10


class World:
    """B = 48 cars on Sim_Track at N = 10 with 2 static discs, 2 movers and traffic (S = 2) per car (test_traffic's Fleet) plus
    2 walls per car across the road a few waypoints ahead; and the host's side of the perception law"""
    S = 2

    def __init__(self, car_twin, B=48, steps=30, seed=75):
        import test_traffic as TT
        self.TT = TT
        self.fl = TT.Fleet("sim", car_twin, extras=True, shape=(N10, B, steps, seed, (B - 20, 8), (2, 3, 4), 6))
        fl = self.fl
        g1, self.grid, self.origin, self.res = _g1("sim")
        rng = np.random.default_rng(seed + 1)
        n_wp = g1["x"].size
        walls = []
        for b in range(B):
            rows = []
            for ahead in (6, 14):
                w = (int(fl.starts[b]) + ahead + int(rng.integers(0, 4))) % n_wp
                (ux, uy), (lx, ly) = g1["border_ub"][w], g1["border_lb"][w]
                t0, t1 = sorted(rng.uniform(0.0, 1.0, 2))
                pts = [(ux + t * (lx - ux), uy + t * (ly - uy)) for t in (t0 * 0.5, 0.25 + t1 * 0.5)]
                rows.append([int(math.floor((p - o) / self.res)) for pt in pts for p, o in zip(pt, self.origin)])
            walls.append(np.array(rows, np.int32))
        self.walls = walls
        self.B, self.steps = B, steps
        self.ang, self.range, self.hold = _angles(180, 1), 0.3, 2

    def handle(self):
        return self.TT._handle("sim", N10, self.B)[0]

    def set_true(self, h):
        h.rollout_set_obstacles(self.fl.static)
        h.rollout_set_movers(self.fl.rows)
        self.fl.set_traffic(h, self.S)
        h.rollout_set_walls(self.walls)

    def host_loop(self, h, steps, book=None, k0=0):
        """Leg L: perception on the host, step by step, on a handle whose own perception is off"""
        fl, B = self.fl, self.B
        book = book or dict(disc_first=np.full((B, 64), -1, np.int32), disc_last=np.full((B, 64), -1, np.int32),
                            wall_first=np.full((B, 16), -1, np.int32), wall_last=np.full((B, 16), -1, np.int32),
                            disc_known=np.zeros(B, np.uint64), wall_known=np.zeros(B, np.uint32), seen_any=0)
        for k in range(k0, k0 + steps):
            st = h.rollout_state()
            true = fl.discs_of(st, k, self.S, fl.range_cells)
            _, ds, ws = mpmpc.perception_scan(self.grid, self.origin, self.res, st["pose"], self.ang, self.range, true, self.walls)
            seen_d, seen_w = [], []
            for b in range(B):
                n = len(true[b])
                scanned = st["alive"][b] == 1
                dk = wk = 0
                for q in range(n):
                    if scanned and (int(ds[b]) >> q) & 1:
                        book["disc_last"][b, q] = k
                        if book["disc_first"][b, q] < 0:
                            book["disc_first"][b, q] = k
                    last = book["disc_last"][b, q]
                    known = last >= 0 if q < 2 else ((last >= 0 and k - last <= self.hold) if q < 4 else last == k)
                    dk |= int(known) << q
                for q in range(len(self.walls[b])):
                    if scanned and (int(ws[b]) >> q) & 1:
                        book["wall_last"][b, q] = k
                        if book["wall_first"][b, q] < 0:
                            book["wall_first"][b, q] = k
                    wk |= int(book["wall_last"][b, q] >= 0) << q
                book["disc_known"][b], book["wall_known"][b] = dk, wk
                seen_d.append(np.where(_bits(dk, n)[:, None], true[b], 0).astype(np.int32))
                seen_w.append(self.walls[b][_bits(wk, len(self.walls[b]))])
                book["seen_any"] += int(scanned) * (bin(int(ds[b])).count("1") + bin(int(ws[b])).count("1"))
            h.rollout_set_obstacles(seen_d)
            h.rollout_set_walls(seen_w)
            h.rollout_step(1)
        return book


@pytest.fixture(scope="module")
def world(car_twin):  # noqa: F811
    return World(car_twin)


def _same_state(a, b, keys):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


@pytest.mark.gpu
def test_one_call_equals_the_step_by_step_loop(world):
    w = world
    KEYS = w.TT.KEYS + ("x0", "u")
    out = {}
    for name, calls in (("A", (30,)), ("A2", (15, 15))):
        h = w.handle()
        w.set_true(h)
        h.rollout_set_perception(w.ang, w.range, w.hold)
        w.fl.init(h)
        for n in calls:
            h.rollout_step(n)
        out[name] = (h.rollout_state(), h.rollout_corridor(), h.rollout_perception(), h.rollout_obstacles())
        h.close()
    h2 = w.handle()
    w.fl.init(h2)
    book = w.host_loop(h2, 30)
    L, L_rows = h2.rollout_state(), h2.rollout_corridor()
    h2.close()
    for name in ("A", "A2"):
        st, rows, per, true = out[name]
        _same_state(st, L, KEYS)
        assert np.array_equal(rows[0], L_rows[0], equal_nan=True) and np.array_equal(rows[1], L_rows[1], equal_nan=True)
        for k in ("disc_first", "disc_last", "wall_first", "wall_last", "disc_known", "wall_known"):
            assert np.array_equal(per[k], book[k]), (name, k)
        assert all(d.shape == (6, 3) for d in true)                           # rollout_obstacles: the TRUE lists
    per = out["A"][2]
    # the run was worth comparing: things were seen, some statics never, movers were lost again, cars still run
    assert book["seen_any"] > 100 and np.any(per["disc_first"][:, :2] >= 1) and np.any(per["disc_first"][:, :2] == -1)
    assert np.any((per["disc_last"][:, 2:4] >= 0) & (per["disc_last"][:, 2:4] < 29 - w.hold)) and np.any(per["wall_first"][:, :2] >= 0)
    print("alive:", np.unique(out["A"][0]["alive"], return_counts=True), "seen:", book["seen_any"])
    assert np.any(out["A"][0]["alive"] == 1) and np.all(per["disc_first"][:, 6:] == -1) and np.all(per["wall_first"][:, 2:] == -1)


@pytest.mark.gpu
def test_blind_equals_empty(world, car_twin):  # noqa: F811
    """A range of one cell: only the sensor's own cell is in range, so a car sees nothing unless it stands IN a primitive (the
    reference's wrap mirrors angles below -pi, so step 3 does not skip that cell for every heading).  The obstacles here lie
    beside the cars' line - near enough for the footprint to touch, never under the sensor, which the test checks on the
    recorded poses - so nothing is ever seen."""
    w = world
    B, steps = w.B, 12
    g1 = _g1("sim")[0]
    n_wp = g1["x"].size
    cell = lambda x, y: (int(math.floor((x - w.origin[0]) / w.res)), int(math.floor((y - w.origin[1]) / w.res)))
    car = (0.12, 0.06, 0.1)
    runs = {}

    def run(name, static=None, walls=None):
        h = w.handle()
        h.rollout_record(steps, rows=True, B=B)
        if name == "blind":
            h.rollout_set_obstacles(static)
            h.rollout_set_walls(walls)
            h.rollout_set_perception(w.ang, w.res * 1.0, 0)
            h.rollout_set_audit(1, *car)
        else:
            h.rollout_set_obstacles([np.zeros((0, 3), np.int32)] * B)
            h.rollout_set_walls([np.zeros((0, 4), np.int32)] * B)
        w.fl.init(h)
        h.rollout_step(steps)
        runs[name] = dict(st=h.rollout_state(), rows=h.rollout_corridor(), tr=h.rollout_trace())
        if name == "blind":
            runs[name]["per"], runs[name]["aud"] = h.rollout_perception(), h.rollout_audit()
        h.close()
    run("empty")
    # per car a static disc of radius 3 whose centre lies 8 cells beside the pose the car has after half the run on the bare
    # map (the car is 12 cells wide: its footprint will touch it, its sensor passes 5 cells clear), and a wall from the road's
    # border a fifth of the way across, a few waypoints ahead
    static, walls = [], []
    for b in range(B):
        poses = runs["empty"]["tr"]["pose"][:, b]
        x, y, psi = poses[np.nonzero(np.isfinite(poses[:, 0]))[0][:steps // 2 + 1][-1]]
        static.append(np.array([cell(x - 8 * w.res * math.sin(psi), y + 8 * w.res * math.cos(psi)) + (3,)], np.int32))
        v = (int(w.fl.starts[b]) + 9) % n_wp
        (ux, uy), (lx, ly) = g1["border_ub"][v], g1["border_lb"][v]
        walls.append(np.array([cell(ux, uy) + cell(ux + 0.2 * (lx - ux), uy + 0.2 * (ly - uy))], np.int32))
    # ... at least one car's true-world row is not its base-map row (K0c's twin, step 0)
    ub_t, lb_t, flag_t = w.TT._twin_rows(car_twin, "sim", static, w.fl.starts, N10)
    ub_0, lb_0, flag_0 = w.TT._twin_rows(car_twin, "sim", [np.zeros((1, 3), np.int32)] * B, w.fl.starts, N10)
    differ = np.any((ub_t != ub_0) | (lb_t != lb_0), 1) | (flag_t != flag_0)
    print("cars whose true-world row differs from the base map's at step 0:", int(differ.sum()))
    assert differ.sum() >= 1
    run("blind", static, walls)
    a, b = runs["blind"], runs["empty"]
    _same_state(a["st"], b["st"], w.TT.KEYS + ("x0", "u"))
    for k in ("ub", "lb", "pose", "u", "status"):
        assert np.array_equal(a["tr"][k], b["tr"][k], equal_nan=True), k
    assert np.array_equal(a["rows"][0], b["rows"][0], equal_nan=True) and np.array_equal(a["rows"][1], b["rows"][1], equal_nan=True)
    for k in range(steps):                                                    # no sensor ever stands in a primitive
        for c in np.nonzero(np.isfinite(a["tr"]["pose"][k][:, 0]))[0]:
            x, y = cell(*a["tr"]["pose"][k][c, :2])
            dcx, dcy, r = static[c][0]
            assert not (-r <= x - dcx < r and -r <= y - dcy < r and (x - dcx) ** 2 + (y - dcy) ** 2 <= r * r)
            wx, wy, _ = _wall_cells(walls[c][0])
            assert not np.any((wx == x) & (wy == y))
    per = a["per"]
    assert np.all(per["disc_first"] == -1) and np.all(per["wall_first"] == -1) and not per["disc_known"].any() and not per["wall_known"].any()
    # the audit judges the TRUE worlds: what mpmpc.footprint_audit says of the recorded poses
    acc = dict(contact_steps=np.zeros(B, np.int32), first_contact=np.full(B, -1, np.int32), min_clearance=np.full(B, car[2]),
               last_contact=np.zeros(B, np.int32), last_clearance=np.full(B, np.nan))
    n_audited = 0
    for k in range(steps):
        pose, al = a["tr"]["pose"][k], a["tr"]["alive"][k]
        audited = np.isfinite(pose[:, 0]) & (al != 0) & (al != -2)            # running when the step began and after localisation
        p = np.where(audited[:, None], pose, w.fl.poses)                      # (any finite pose: the verdict is not used)
        con, clr = mpmpc.footprint_audit(w.grid, w.origin, w.res, p, *car, discs=static, walls=walls)
        for c in np.nonzero(audited)[0]:
            acc["last_contact"][c], acc["last_clearance"][c] = con[c], clr[c]
            acc["contact_steps"][c] += con[c]
            if con[c] and acc["first_contact"][c] < 0:
                acc["first_contact"][c] = k
            acc["min_clearance"][c] = min(acc["min_clearance"][c], clr[c])
        n_audited += int(audited.sum())
    aud = a["aud"]
    print("alive:", np.unique(a["st"]["alive"], return_counts=True), "audited:", n_audited, "contacts:", int(acc["contact_steps"].sum()))
    for k in acc:
        assert np.array_equal(aud[k], acc[k], equal_nan=True), (k, aud[k], acc[k])
    assert n_audited * 2 >= B * steps and np.any(aud["contact_steps"] > 0)    # blind cars hit what they cannot see


@pytest.mark.gpu
def test_off_means_off(world):
    w = world
    KEYS = w.TT.KEYS + ("x0", "u")
    runs = []
    for toggled in (False, True):
        h = w.handle()
        h.rollout_record(10, rows=True, B=w.B)
        w.set_true(h)
        if toggled:
            h.rollout_set_perception(w.ang, w.range, w.hold)
            h.rollout_set_perception(None)
        w.fl.init(h)
        h.rollout_step(10)
        runs.append((h.rollout_state(), h.rollout_trace(), h.rollout_obstacles()))
        with pytest.raises(mpmpc.MpmpcError, match="error %d" % E_STATE):
            h.rollout_perception()                                            # off: nothing to report
        h.close()
    (a, a_tr, a_d), (b, b_tr, b_d) = runs
    _same_state(a, b, KEYS)
    for k in ("ub", "lb", "pose", "u", "status", "alive"):
        assert np.array_equal(a_tr[k], b_tr[k], equal_nan=True), k
    assert all(np.array_equal(p, q) for p, q in zip(a_d, b_d))
    # the true world reaches the planner: the rows are not those of the bare map
    h = w.handle()
    h.rollout_record(10, rows=True, B=w.B)
    h.rollout_set_obstacles([np.zeros((0, 3), np.int32)] * w.B)
    w.fl.init(h)
    h.rollout_step(10)
    bare = h.rollout_trace()
    h.close()
    assert not np.array_equal(bare["ub"], a_tr["ub"], equal_nan=True)


@pytest.mark.gpu
def test_state_errors(world):
    import scenarios
    import mpmpc_testlib as T
    w = world
    h = w.handle()

    def refused(f, code=E_STATE):
        with pytest.raises(mpmpc.MpmpcError, match="error %d" % code):
            f()
    refused(h.rollout_perception)                                             # perception off
    h.rollout_set_perception(w.ang, w.range, 1)
    w.set_true(h)
    w.fl.init(h)
    refused(h.rollout_perception)                                             # no step since the reset
    h.rollout_step(2)
    per = h.rollout_perception()
    assert per["disc_first"].shape == (w.B, 64) and per["wall_known"].dtype == np.uint32
    lib = h.lib
    assert lib.mpmpc_rollout_perception(h._h, w.B - 1, None, None, None, None, None, None) == E_STATE      # another B
    assert lib.mpmpc_rollout_perception(h._h, w.B, None, None, None, None, None, None) == 0                # any pointer may be NULL
    h.rollout_set_walls(w.walls)                                              # a world setter resets
    refused(h.rollout_perception)
    h.rollout_step(1)
    first = h.rollout_perception()["disc_first"]
    assert np.any(first >= 0) and np.all(first[first >= 0] == 2)             # steps count from rollout_init
    refused(lambda: h.rollout_set_perception(w.ang, w.range, -1), E_ARG)
    refused(lambda: h.rollout_set_perception(w.ang, 0.0, 0), E_ARG)
    refused(lambda: h.rollout_set_perception(w.ang, w.res * 2049, 0), E_ARG)  # more than 2048 cells on the map of the moment
    h.rollout_step(1)                                                         # a refused call leaves the setting as it was
    h.rollout_perception()
    # no per-car setting in force: nothing to perceive, the step runs, nothing to report
    for off in (h.rollout_set_obstacles, h.rollout_set_movers, h.rollout_set_traffic, h.rollout_set_walls):
        off(None)
    w.fl.init(h)
    h.rollout_step(1)
    refused(h.rollout_perception)
    h.close()
    # a step without a map
    tr = scenarios.sim_track()
    g1 = _g1("sim")[0]
    h = mpmpc.Handle(T.stock_config(N10, max_batch=4), mpmpc.default_settings())
    h.set_path(tr.kappa, tr.v_ref, tr.ds_next)
    h.set_path_geometry(g1["x"], g1["y"], g1["psi"], g1["border_ub"], g1["border_lb"])
    n_wp = g1["x"].size
    h.set_corridor(np.full((n_wp, N10), 0.1), np.full((n_wp, N10), -0.1))
    cum = np.cumsum(g1["segment_lengths"])
    starts = np.arange(4) * 20
    h.rollout_set_perception(w.ang, w.range, 0)
    h.rollout_init(TS, cum, cum[starts], np.stack([g1["x"][starts], g1["y"][starts], g1["psi"][starts]], 1))
    refused(lambda: h.rollout_step(1))
    h.rollout_set_perception(None)
    h.rollout_step(1)
    h.close()


@pytest.mark.gpu
def test_drop_in_use():
    from lidar_model import LidarModel
    from map import Obstacle
    from MPC import BatchMPC
    from perception import Perception
    from scipy import sparse
    m, rp, car = T.build_world(obstacles=False)
    Q, R, QN = sparse.diags([1.0, 0.0, 0.0]), sparse.diags([0.5, 0.0]), sparse.diags([1.0, 0.0, 0.0])
    ic = {'umin': np.array([0.0, -np.tan(0.66) / car.length]), 'umax': np.array([1.0, np.tan(0.66) / car.length])}
    sc = {'xmin': np.array([-np.inf] * 3), 'xmax': np.array([np.inf] * 3)}
    B = 8
    bm = BatchMPC(car, N10, Q, R, QN, sc, ic, 4.0, max_batch=B, corridor="device")
    starts = np.arange(B) * 20
    cum = np.cumsum(rp.segment_lengths)
    wps = [rp.waypoints[w] for w in starts]
    poses = np.array([[w.x, w.y, w.psi] for w in wps])
    ahead = [rp.waypoints[(w + 6) % rp.n_waypoints] for w in starts]
    behind = [rp.waypoints[(w - 8) % rp.n_waypoints] for w in starts]
    obstacles = [[Obstacle(a.x, a.y, 0.04), Obstacle(b.x, b.y, 0.04)] for a, b in zip(ahead, behind)]      # one ahead, one out of sight
    p = Perception(LidarModel(FoV=90, range=0.5, resolution=1), hold=1)
    plain = bm.rollout(cum[starts], poses, 4, obstacles=obstacles)
    out = bm.rollout(cum[starts], poses, 4, obstacles=obstacles, perception=p)
    per = out["perception"]
    assert set(per) == {"disc_first", "disc_last", "wall_first", "wall_last", "disc_known", "wall_known"}
    again = bm.handle.rollout_perception()
    assert all(np.array_equal(per[k], again[k]) for k in per) and all(np.array_equal(per[k], bm.rollout_perception()[k]) for k in per)
    assert np.all(per["disc_first"][:, 0] >= 0) and np.all(per["disc_first"][:, 1] == -1)      # the one ahead, never the one behind
    assert np.all(per["disc_known"] == 1) and np.all(per["disc_first"][:, 2:] == -1) and not per["wall_known"].any()
    # the sensor alone, through Perception.scan, agrees with step 0
    _, ds, ws = p.scan(poses, m, discs=[m.obstacle_discs(o) for o in obstacles])
    assert np.array_equal(ds == 1, per["disc_first"][:, 0] == 0) and np.all(ds <= 1) and np.sum(ds == 1) >= B // 2 and not ws.any()
    assert "perception" not in plain and bm.rollout(cum[starts], poses, 4, perception=p)["perception"] is None
    later = bm.rollout(cum[starts], poses, 4, obstacles=obstacles)            # a later rollout perceives nothing again
    assert all(np.array_equal(later[k], plain[k]) for k in plain)
    bm.close()
