"""Corridor commitment in the device rollout (K0k: the KEEP instantiations of K0c, mpmpc_rollout_set_commitment; the law:
csrc/commitment_core.hpp): a waypoint that was in a car's horizon in the step before keeps the side of an obstacle it chose then.

On the CPU the twin (tests/emul_commitment: the header compiled for the host) against commitment.row, a plain-Python restatement
of the law on the host classes' free segments, over the scenes the feature was proposed on - one disc of radius 0.04 m on Sim_Track
at waypoint 60, static at five lateral offsets, appearing, oncoming, crossing at two speeds, the horizon start advancing 1 or 2
waypoints per step from waypoint 20 - and an open Real_Track run onto the clamped end columns; off against the reference and
the K0c twin; the flip counts; the ratio clause on a hand-made line; the memory; the argument checks.  On an MI355X the rollout
teacher-forced against the twin step by step (rows, memory, counters bit for bit), one call against many and a resumed run, off
against a rollout that never heard of the setting, perception and a delay under a committed car, the resets and the error codes.
"""
import ctypes as C
import math

import numpy as np
import pytest

import mpmpc
import mpmpc_testlib as T
import scenarios
import twins
import commitment as K
from commitment import Commitment
from commitment_twin import commitment as load_twin
from map import Map
from reference_path import ReferencePath

_d, _i, _g1, _sm = T._d, T._i, T.g1_world, T.safety_margin
E_ARG, E_STATE = -1, -3
INF = math.inf
TS = 0.05


@pytest.fixture(scope="module")
def lib():
    return load_twin()


# ------------------------------------------------------------------------------------------------------------ worlds
class World:
    """A path on a grid for the twin (K0a's base build, once) and for the restatement (the host classes on a copy of the grid
    with the discs of the moment stamped in; free segments cached per (waypoint, discs near its border line))."""

    def __init__(self, lib, N, grid, origin, res, x, y, psi, kappa, ds_next, bub, blb, circular, sm):
        self.lib, self.N, self.sm, self.circular = lib, N, sm, circular
        self.grid, self.origin, self.res = np.ascontiguousarray(grid, np.int8), origin, res
        self.x, self.y, self.psi, self.ds = (np.ascontiguousarray(a, float) for a in (x, y, psi, ds_next))
        self.bub, self.blb = np.ascontiguousarray(bub, float), np.ascontiguousarray(blb, float)
        self.n_wp = self.x.size
        self.tw = lib.cmt_twin_new(grid.shape[0], grid.shape[1], T._b(self.grid), origin[0], origin[1], res, self.n_wp, _d(self.x),
                                   _d(self.y), _d(self.psi), _d(self.ds), 1 if circular else 0, _d(self.bub), _d(self.blb), N,
                                   2 * sm, sm)
        assert self.tw
        self.map = Map.from_grid(self.grid, origin, res)
        self.rp = ReferencePath.from_tables(self.map, self.x, self.y, self.psi, kappa, circular=circular, border_ub=self.bub,
                                            border_lb=self.blb)
        cu = np.floor((self.bub - np.asarray(origin)) / res).astype(int)
        cl = np.floor((self.blb - np.asarray(origin)) / res).astype(int)
        self.box = np.concatenate([np.minimum(cu, cl) - 2, np.maximum(cu, cl) + 2], 1)      # x0, y0, x1, y1 with a margin
        self.cache = {}

    def __del__(self):
        self.lib.cmt_twin_free(self.tw)

    def on_path(self, i, e):
        """the cell of the point e to the left of waypoint i"""
        i %= self.n_wp
        px, py = self.x[i] - e * math.sin(self.psi[i]), self.y[i] + e * math.cos(self.psi[i])
        return self.map.w2m(px, py)

    def disc(self, i, e, radius=0.04):
        return self.on_path(i, e) + (int(np.ceil(radius / self.res)),)

    # --- the twin: one step of B cars
    def step(self, wp_id, discs, keep, mem, counts, walls=None):
        B, N = len(discs), self.N
        off, flat = T.csr([np.asarray(d, np.int32).reshape(-1, 3) for d in discs], 3, pad=False)
        woff = wflat = None
        if walls is not None:
            woff, wflat = T.csr([np.asarray(w, np.int32).reshape(-1, 4) for w in walls], 4)
        wp = np.ascontiguousarray(wp_id, np.int32)
        kp = np.ascontiguousarray(keep, float)
        mw, mr = np.ascontiguousarray(mem[0], np.int32), np.ascontiguousarray(mem[1], float)
        ub, lb, flag = np.zeros((B, N)), np.zeros((B, N)), np.zeros(B, np.int32)
        nw, nr = np.zeros((B, N), np.int32), np.zeros((B, N, 6))
        rc = self.lib.cmt_twin_rows(self.tw, B, _i(wp), _i(off), _i(flat), None if woff is None else _i(woff),
                                    None if wflat is None else _i(wflat), _d(kp), _i(mw), _d(mr), _d(ub), _d(lb), _i(flag), _i(nw),
                                    _d(nr), _i(counts))
        assert rc == 0
        return ub, lb, flag, (nw, nr)

    # --- the restatement: one step of one car
    def segments(self, discs):
        discs = [tuple(int(v) for v in d) for d in np.asarray(discs).reshape(-1, 3).tolist()]

        def of(i):
            x0, y0, x1, y1 = self.box[i]
            near = tuple(d for d in discs if d[0] - d[2] <= x1 and d[0] + d[2] - 1 >= x0 and d[1] - d[2] <= y1 and d[1] + d[2] - 1 >= y0)
            if (i, near) not in self.cache:
                self.map.data[:] = self.grid
                for cx, cy, r in near:
                    yy, xx = np.ogrid[-r:r, -r:r]
                    self.map.data[cy - r:cy + r, cx - r:cx + r][xx ** 2 + yy ** 2 <= r ** 2] = 0
                self.cache[(i, near)] = [(u[0], u[1], l[0], l[1]) for u, l in
                                         self.rp._compute_free_segments(self.rp.waypoints[i], 2 * self.sm)]
            return self.cache[(i, near)]
        return of

    def law(self, wp_id, discs, keep, mem_wp, mem_rows):
        return K.row(self.x.tolist(), self.y.tolist(), self.psi.tolist(), self.ds.tolist(), self.circular, int(wp_id), self.N,
                     self.segments(discs), self.sm, float(keep), list(mem_wp), [list(r) for r in mem_rows])

    def empty(self, B):
        return np.full((B, self.N), K.EMPTY, np.int32), np.zeros((B, self.N, 6))


_WORLDS = {}


def _track_world(lib, track, N):
    if (track, N) not in _WORLDS:
        g1, grid, origin, res = _g1(track)
        _WORLDS[(track, N)] = World(lib, N, grid, origin, res, g1["x"], g1["y"], g1["psi"], g1["kappa"], g1["ds_next"], g1["border_ub"],
                                    g1["border_lb"], track == "sim", _sm(track))
    return _WORLDS[(track, N)]


def _line_world(lib, N=10):
    """a hand-made world: a free grid of 2 m x 2 m at 0.01 m, a straight open path along x at y = 1 with a waypoint every 0.15 m
    and the borders 0.4 m to either side"""
    if ("line", N) not in _WORLDS:
        n = 12
        x, y = 0.1 + 0.15 * np.arange(n), np.full(n, 1.0)
        bub, blb = np.stack([x, y + 0.4], 1), np.stack([x, y - 0.4], 1)
        _WORLDS[("line", N)] = World(lib, N, np.ones((200, 200), np.int8), (0.0, 0.0), 0.01, x, y, np.zeros(n), np.zeros(n),
                                     np.full(n, 0.15), bub, blb, False, 0.03)
    return _WORLDS[("line", N)]


# the scenes the feature was proposed on: name -> (discs of step k on world w, static?)
def _scenes(w):
    out = {}
    for e in (0.0, 0.005, -0.005, 0.01, 0.02):
        out["static e=%g" % e] = (lambda k, d=w.disc(60, e): [d], True)
    out["appearing"] = (lambda k, d=w.disc(60, 0.0): [d] if k >= 25 else [], False)
    out["oncoming"] = (lambda k: [w.disc(90 - k, 0.0)], False)
    for v in (0.002, 0.004):
        out["crossing v=%g" % v] = (lambda k, v=v: [w.disc(60, -0.06 + v * k)], False)
    return out


KEEPS = np.array([0.0, INF, 4.0, 1.0])
STRIDES = ((1, 45), (2, 25))      # waypoints per step, steps


def _run_twin(w, disc_of_step, stride, steps, keep=KEEPS, w0=20):
    """every car of `keep` in the same world -> per step (ub, lb, flag, memory), and the counters at the end"""
    B = len(keep)
    mem, counts, out = w.empty(B), np.zeros((3, B), np.int32), []
    for k in range(steps):
        ub, lb, flag, mem = w.step([w0 + k * stride] * B, [disc_of_step(k)] * B, keep, mem, counts)
        out.append((ub, lb, flag, mem))
    return out, counts


# ------------------------------------------------------------------------------------------------------------ CPU
def _against_the_law(w, disc_of_step, wp_of_step, steps, keep=KEEPS):
    B = len(keep)
    mem, counts = w.empty(B), np.zeros((3, B), np.int32)
    law_mem = [([K.EMPTY] * w.N, [[0.0] * 6] * w.N) for _ in range(B)]
    law_counts = np.zeros((3, B), np.int64)
    for k in range(steps):
        d, wp = disc_of_step(k), wp_of_step(k)
        ub, lb, flag, mem = w.step([wp] * B, [d] * B, keep, mem, counts)
        for b in range(B):
            v, lu, ll, nw, nr, c = w.law(wp, d, keep[b], *law_mem[b])
            law_mem[b] = (nw, nr)
            law_counts[:, b] += c
            assert v == flag[b], (k, b)
            assert np.array_equal(ub[b], lu, equal_nan=True) and np.array_equal(lb[b], ll, equal_nan=True), (k, b)
            assert np.array_equal(mem[0][b], nw) and np.array_equal(mem[1][b], np.array(nr)), (k, b)
        assert np.array_equal(counts, law_counts), k
    return counts


@pytest.mark.parametrize("N", [10, 30, 70])
def test_twin_equals_the_restated_law_bit_exact(N, lib):
    w = _track_world(lib, "sim", N)
    kept = 0
    for name, (discs, _) in _scenes(w).items():
        for stride, steps in STRIDES:
            counts = _against_the_law(w, discs, lambda k: 20 + k * stride, steps)
            kept += counts[0].sum()
    assert kept > 0      # rule 1 decided columns


def test_twin_equals_the_restated_law_on_the_open_route(lib):
    """Real_Track, N = 10: the horizon start runs to the last waypoint but one, so the last columns are clamped to the route's end
    (duplicates in the memory); a disc on the path 12 waypoints before the end gives them something to choose"""
    w = _track_world(lib, "real", 10)
    d = w.disc(w.n_wp - 12, 0.0, 0.25)
    counts = _against_the_law(w, lambda k: [d], lambda k: w.n_wp - 32 + k, 30)
    assert counts[0].sum() > 0
    out, _ = _run_twin(w, lambda k: [d], 1, 30, w0=w.n_wp - 32)
    wp = out[-1][3][0][1]
    assert (wp == w.n_wp - 1).sum() >= 2      # the clamped end columns are duplicates


@pytest.mark.parametrize("track", ["sim", "real"])
def test_off_is_the_reference_and_the_k0c_twin(track, lib):
    N = 30
    w = _track_world(lib, track, N)
    g1, grid, origin, res = _g1(track)
    car = twins.car()
    arrs = [np.ascontiguousarray(g1[k], float) for k in ("x", "y", "psi", "ds_next", "border_ub", "border_lb")]
    d = [w.disc(60, 0.0, 0.04 if track == "sim" else 0.25)]
    starts = np.arange(20, 60, dtype=np.int32)
    B = starts.size
    mem, counts = w.empty(B), np.zeros((3, B), np.int32)
    for rnd in range(2):      # (the second round with the first one's memory: an off car does not read it)
        ub, lb, flag, mem = w.step(starts, [d] * B, np.zeros(B), mem, counts)
        off, flat = T.csr([np.asarray(d, np.int32)] * B, 3, pad=False)
        ub2, lb2, flag2 = np.zeros((B, N)), np.zeros((B, N)), np.zeros(B, np.int32)
        assert car.car_emu_rows(grid.shape[0], grid.shape[1], T._b(grid), origin[0], origin[1], res, arrs[0].size,
                                *[_d(a) for a in arrs[:4]], 1 if track == "sim" else 0, _d(arrs[4]), _d(arrs[5]), N, 2 * w.sm, w.sm, B,
                                _i(starts), _i(off), _i(flat), _d(ub2), _d(lb2), _i(flag2)) == 0
        assert np.array_equal(ub, ub2, equal_nan=True) and np.array_equal(lb, lb2, equal_nan=True) and np.array_equal(flag, flag2)
    assert counts[0].sum() == 0 and counts[1].sum() == 0
    # the host classes (the tolerance of the K0c tests for this comparison: none)
    w.map.data[:] = w.grid
    cx, cy, r = d[0]
    yy, xx = np.ogrid[-r:r, -r:r]
    w.map.data[cy - r:cy + r, cx - r:cx + r][xx ** 2 + yy ** 2 <= r ** 2] = 0
    for j, s in enumerate(starts[::4]):
        u, l, _ = w.rp.update_path_constraints(int(s) + 1, N, 2 * w.sm, w.sm)
        assert flag[4 * j] == 0 and np.array_equal(ub[4 * j], u) and np.array_equal(lb[4 * j], l)
    w.map.data[:] = w.grid


def test_flip_counts(lib):
    """the reason for the feature: the reference's law moves a waypoint's corridor to the other side of a disc on the path in the
    step the disc reaches column 0; a committed car never does in a static world - the remembered candidate is still there"""
    w = _track_world(lib, "sim", 30)
    for name, (discs, static) in _scenes(w).items():
        if not static:
            continue
        for stride, steps in STRIDES:
            _, counts = _run_twin(w, discs, stride, steps)
            print("%s stride %d: moved %s kept %s switched %s" % (name, stride, counts[2], counts[0], counts[1]))
            if name in ("static e=0", "static e=0.005", "static e=-0.005"):
                assert counts[2][0] >= 1, (name, stride)
            assert counts[2][1] == 0, (name, stride)


def test_ratio_clause_on_a_hand_made_line(lib):
    """Waypoint 5 of the straight path: a disc on the path splits its border line (0.8 m) into a left (upper) and a right
    candidate; the car stands (wp_id = 0) and remembers the side the chain chose in step 0.  A second disc then moves in from
    that side's border by one cell per step, so the kept side shrinks.  With switch_ratio = 2 the column switches in the first
    step in which the other candidate is more than twice as long as the kept one - computed here from the host classes'
    segments - `switched` is 1 from then on and the row has changed sides; with inf it never switches."""
    w = _line_world(lib)
    cx, cy = w.map.w2m(w.x[5], 1.0)
    wall = (cx, cy + 2, 6)
    keep = np.array([2.0, INF])
    B = 2
    counts = np.zeros((3, B), np.int32)
    ub, lb, flag, mem = w.step([0] * B, [[wall]] * B, keep, w.empty(B), counts)
    assert np.all(flag == 0) and counts.sum() == 0 and np.array_equal(ub[0], ub[1])
    side = 1 if lb[0][4] > 0 else -1                          # column 4 is waypoint 5: left of the path, or right of it
    assert (ub[0][4] < 0) == (side < 0)

    def discs(k):                                              # radius 14: the neighbours' lines, 15 cells away, stay free
        return [wall, (cx, cy + side * (54 - k), 14)]

    switched_at, want_at = None, None
    for k in range(1, 26):
        segs = w.segments(discs(k))(5)
        assert len(segs) == 2
        spans = [math.sqrt((s[0] - s[2]) ** 2 + (s[1] - s[3]) ** 2) for s in segs]      # [left, right]
        kept, other = (0, 1) if side > 0 else (1, 0)
        if want_at is None and spans[other] > 2 * spans[kept]:
            want_at = k
        before = counts.copy()
        ub, lb, flag, mem = w.step([0] * B, [discs(k)] * B, keep, mem, counts)
        assert np.all(flag == 0)
        assert np.array_equal(counts[0] - before[0], [1, 1])     # one multi-segment column, decided from memory
        if switched_at is None and counts[1][0] > 0:
            switched_at = k
        now = 1 if lb[0][4] > 0 else -1
        assert now == (side if switched_at is None else -side), k      # ratio 2: the kept side, then the longest
        assert (1 if lb[1][4] > 0 else -1) == side, k                   # inf: the kept side throughout
    assert want_at is not None and 1 < want_at < 25 and switched_at == want_at
    assert counts[1].tolist() == [1, 0] and counts[2].tolist() == [1, 0]      # the switch is the one move


def test_the_lowest_column_wins_among_duplicates(lib):
    w = _line_world(lib)
    cx, cy = w.map.w2m(w.x[5], 1.0)
    d = [(cx, cy, 6)]                                          # on the path: two candidates of equal length
    counts = np.zeros((3, 1), np.int32)
    ub0, lb0, _, mem0 = w.step([0], [d], [0.0], w.empty(1), counts)
    left = np.array([ub0[0][4], lb0[0][4], w.x[5], 1.0 + ub0[0][4] + w.sm, w.x[5], 1.0 + lb0[0][4] - w.sm])
    assert left[1] > 0                                         # (the first maximum of equal spans: the upper, left one)
    right = np.array([-lb0[0][4], -ub0[0][4], w.x[5], 1.0 - lb0[0][4] + w.sm, w.x[5], 1.0 - ub0[0][4] - w.sm])
    for lo, hi, sign in ((left, right, 1), (right, left, -1)):
        mw, mr = w.empty(1)
        mw[0][2], mw[0][7] = 5, 5
        mr[0][2], mr[0][7] = lo, hi
        ub, lb, _, _ = w.step([0], [d], [INF], (mw, mr), counts)
        assert np.sign(ub[0][4]) == sign and np.sign(lb[0][4]) == sign
        v, lu, ll, *_ = w.law(0, d, INF, mw[0], mr[0])
        assert np.array_equal(ub[0], lu) and np.array_equal(lb[0], ll)


def test_a_resumed_twin_run_equals_the_unbroken_one(lib):
    w = _track_world(lib, "sim", 30)
    discs = _scenes(w)["crossing v=0.002"][0]
    whole, counts = _run_twin(w, discs, 1, 45)
    B = len(KEEPS)
    mem = tuple(a.copy() for a in whole[19][3])
    c2 = np.zeros((3, B), np.int32)
    for k in range(20, 45):
        ub, lb, flag, mem = w.step([20 + k] * B, [discs(k)] * B, KEEPS, mem, c2)
        assert np.array_equal(ub, whole[k][0], equal_nan=True) and np.array_equal(lb, whole[k][1], equal_nan=True)
        assert np.array_equal(mem[0], whole[k][3][0]) and np.array_equal(mem[1], whole[k][3][1])
    _, c1 = _run_twin(w, discs, 1, 20)
    assert np.array_equal(c1 + c2, counts)


def test_argument_checks_and_exports_without_device(lib, built_library):
    ml = mpmpc.load_library(built_library)
    one = np.ones(1)
    assert ml.mpmpc_rollout_set_commitment(None, 1, _d(one), None, None) == E_ARG      # no handle
    assert ml.mpmpc_rollout_commitment(None, 1, None, None, None) == E_ARG
    raw = C.CDLL(built_library)
    for name in ("mpmpc_rollout_set_commitment", "mpmpc_rollout_commitment"):
        assert name in mpmpc.EXPORTS and hasattr(raw, name)
    for name in ("rollout_set_commitment", "rollout_commitment"):
        assert hasattr(mpmpc.Handle, name)

    def check(keep, B=None, max_batch=8, N=30, wp=None, rows=None):
        k = np.ascontiguousarray(keep, float)
        return lib.cmt_emu_check(k.size if B is None else B, max_batch, N, _d(k), None if wp is None else _i(wp), None if rows is None else _d(rows))
    assert check([0.0, 1.0, 4.0, INF]) == 0
    for bad in (0.5, -1.0, math.nan, -INF, 0.999):
        assert check([1.0, bad]) == E_ARG, bad
    assert check([1.0], B=0) == E_ARG and check([1.0] * 9) == E_ARG      # B outside [1, max_batch]
    wp, rows = np.full((2, 30), -1, np.int32), np.zeros((2, 30, 6))
    assert check([1.0, 0.0], wp=wp, rows=rows) == 0
    assert check([1.0, 0.0], wp=wp) == E_ARG and check([1.0, 0.0], rows=rows) == E_ARG
    wp[1, 3] = -2
    assert check([1.0, 0.0], wp=wp, rows=rows) == E_ARG
    # the 256 MiB cap: B x N x 104 + 20 B bytes
    assert lib.cmt_emu_budget() == 256 << 20 == K.BUDGET
    for B, N in ((7, 30), (1 << 20, 255)):
        assert lib.cmt_emu_bytes(B, N) == B * N * 104 + 20 * B == K.block_bytes(B, N)
    top = (256 << 20) // (255 * 104 + 20)
    big = np.ones(top + 1)
    assert check(big[:top], max_batch=1 << 20, N=255) == 0 and check(big, max_batch=1 << 20, N=255) == E_ARG
    # the Python front end
    assert np.array_equal(Commitment().keep(3), [INF] * 3) and np.array_equal(Commitment([0, 2.0]).keep(2), [0.0, 2.0])
    for bad in (0.5, -1.0, math.nan, [1.0, 0.5]):
        with pytest.raises(ValueError):
            Commitment(bad).keep(2)
    with pytest.raises(ValueError):
        Commitment([1.0, 2.0, 3.0]).keep(2)


# ------------------------------------------------------------------------------------------------------------ GPU
KEYS = ("s", "pose", "cc", "wp_id", "x0", "u", "status", "counter", "alive")


def _handle(track, N, B, routes=False):
    tr = scenarios.sim_track() if track == "sim" else scenarios.real_track()
    g1, grid, origin, res = _g1(track)
    h = mpmpc.Handle(T.stock_config(N, max_batch=B, track=None if track == "sim" else tr), mpmpc.default_settings())
    h.set_path(tr.kappa, tr.v_ref, tr.ds_next)
    h.set_map(grid, origin, res)
    h.set_path_geometry(g1["x"], g1["y"], g1["psi"], g1["border_ub"], g1["border_lb"])
    if routes:      # the one path as a fleet of one route: what mpmpc_rollout_reroute needs
        h.set_routes([0, g1["x"].size], [1 if track == "sim" else 0])
        h.set_car_routes(np.zeros(B, np.int32))
    h.rollout_warm_start(False)
    sm = _sm(track)
    h.build_corridor(N, 2 * sm, sm, want_tables=False)
    return h


def _init(h, track, starts):
    g1 = _g1(track)[0]
    cum = np.cumsum(g1["segment_lengths"])
    starts = np.asarray(starts)
    h.rollout_init(TS, cum, cum[starts], np.stack([g1["x"][starts], g1["y"][starts], g1["psi"][starts]], 1))


def _same_state(a, b):
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k


class Forced:
    """The twin teacher-forced by a running rollout: after every device step it takes the step's wp_id and the discs the step
    planned with, runs the twin from its own memory of the step before and compares rows, memory and counters bit for bit."""

    def __init__(self, w, h, keep, walls=None, mem=None):
        self.w, self.h, self.keep, self.walls = w, h, np.asarray(keep, float), walls
        self.B = self.keep.size
        self.mem = w.empty(self.B) if mem is None else mem
        self.counts = np.zeros((3, self.B), np.int32)
        self.wp = []

    def check(self, planned=None):
        h = self.h
        st = h.rollout_state()
        discs = h.rollout_obstacles() if planned is None else planned
        ub, lb, flag, self.mem = self.w.step(st["wp_id"], discs, self.keep, self.mem, self.counts, self.walls)
        got_ub, got_lb = h.rollout_corridor()
        got = h.rollout_commitment()
        assert np.array_equal(got_ub, ub, equal_nan=True) and np.array_equal(got_lb, lb, equal_nan=True)
        assert np.array_equal(got["wp"], self.mem[0]) and np.array_equal(got["rows"], self.mem[1])
        assert np.array_equal(np.stack([got["kept"], got["switched"], got["moved"]]), self.counts)
        self.wp.append(st["wp_id"].copy())
        return st, got


FLEET_KEEP = np.array([0.0, 0.0, 0.0, INF, INF, 4.0, 1.0])
DISC_AT = 60      # the waypoint of the fleet's discs, as in the table: the closed loop passes it around step 40


def _fleet_worlds(w):
    """cars 0 - 2 off, 3 - 6 on: the three static discs of the table (cars 0, 1 off; car 3 inf), a crossing mover (car 2, off),
    a wall across the middle of the lane (car 4, inf), an oncoming mover (car 5, ratio 4) and no discs (car 6, ratio 1)"""
    res, g1 = w.res, _g1("sim")[0]
    cum = np.cumsum(g1["segment_lengths"])
    static = [[w.disc(DISC_AT, 0.0)], [w.disc(DISC_AT, 0.005)], [], [w.disc(DISC_AT, -0.005)], [], [], []]
    r = int(np.ceil(0.04 / res))
    i = DISC_AT % w.n_wp
    nx, ny = -math.sin(w.psi[i]), math.cos(w.psi[i])
    crossing = (0, r, w.x[i] - 0.06 * nx, w.y[i] - 0.06 * ny, 0.002 * nx, 0.002 * ny)      # 2 mm per step across the lane
    oncoming = (1, r, cum[(DISC_AT + 30) % w.n_wp], 0.0, -(cum[21] - cum[20]), 0.0)          # a waypoint per step towards the car
    movers = [np.zeros((0, 6))] * 7
    movers[2], movers[5] = np.array([crossing]), np.array([oncoming])
    walls = [np.zeros((0, 4), np.int32)] * 7
    walls[4] = np.array([w.on_path(DISC_AT, 0.03) + w.on_path(DISC_AT, -0.03)], np.int32)
    return static, movers, walls


@pytest.fixture(scope="module")
def fleet(lib):
    """the fleet's run, once: 45 steps of rollout_step(1), every step teacher-forced against the twin"""
    w = _track_world(lib, "sim", 30)
    static, movers, walls = _fleet_worlds(w)
    h = _handle("sim", 30, 7)
    h.rollout_set_walls(walls)
    h.rollout_set_obstacles(static)
    h.rollout_set_movers(movers)
    _init(h, "sim", [20] * 7)
    h.rollout_set_commitment(FLEET_KEEP)
    f = Forced(w, h, FLEET_KEEP, walls)
    for k in range(45):
        h.rollout_step(1)
        st, got = f.check()
    ub, lb = h.rollout_corridor()
    h.close()
    return dict(w=w, state=st, commitment=got, wp=np.array(f.wp), rows=(ub, lb), static=static, movers=movers, walls=walls)


@pytest.mark.gpu
def test_device_equals_the_twin_teacher_forced(fleet):
    c, wp = fleet["commitment"], fleet["wp"]
    print("wp_id at the end %s, kept %s switched %s moved %s" % (wp[-1], c["kept"], c["switched"], c["moved"]))
    assert np.all(wp[-1][[0, 1, 3]] >= DISC_AT - 1)            # the closed loop reached the static discs (column 0 met them)
    assert c["moved"][[0, 1]].sum() >= 1                       # off cars in static worlds: the reference's law flips
    assert c["moved"][3] == 0 and c["moved"][4] == 0           # inf cars in static worlds never do
    assert np.all(c["kept"][:3] == 0) and np.all(c["switched"][:5] == 0) and c["kept"][3] > 0 and c["kept"][4] > 0


@pytest.mark.gpu
def test_a_lane_owns_two_columns_and_the_replay_crosses_column_64(lib):
    """N = 70: a disc on the path at waypoint 84 / 85 of cars at waypoint 20 - its multi-segment columns straddle columns 63 / 64"""
    w = _track_world(lib, "sim", 70)
    keep = np.array([0.0, INF, 2.0])
    h = _handle("sim", 70, 3)
    d = [w.disc(84, 0.0), w.disc(85, 0.005)]
    h.rollout_set_obstacles([d] * 3)
    _init(h, "sim", [20] * 3)
    h.rollout_set_commitment(keep)
    f = Forced(w, h, keep)
    multi = set()
    for k in range(8):
        h.rollout_step(1)
        st, got = f.check()
        segs = w.segments(d)
        multi |= {c for c in range(70) if len(segs(K.wp_index(int(st["wp_id"][1]) + 1 + c, w.n_wp, True))) >= 2}
    h.close()
    print("multi-segment columns seen: %s, kept %s" % (sorted(multi), got["kept"]))
    assert any(c <= 63 for c in multi) and any(c >= 64 for c in multi) and got["kept"][1] > 0


@pytest.mark.gpu
def test_open_route_through_its_end(lib):
    """Real_Track, N = 10: the cars start 14 waypoints before the last one and drive until the route ends under them (alive -2);
    that step's horizon holds the clamped end column twice"""
    w = _track_world(lib, "real", 10)
    keep = np.array([0.0, INF, 2.0])
    h = _handle("real", 10, 3)
    d = [w.disc(w.n_wp - 6, 0.0, 0.25)]
    h.rollout_set_obstacles([d] * 3)
    _init(h, "real", [w.n_wp - 15] * 3)
    h.rollout_set_commitment(keep)
    f = Forced(w, h, keep)
    for k in range(40):
        h.rollout_step(1)
        st, got = f.check()
        if np.all(st["alive"] != 1):
            break
    h.close()
    print("steps %d alive %s kept %s" % (k + 1, st["alive"], got["kept"]))
    assert np.all(st["alive"] == -2)
    assert np.all((got["wp"] == w.n_wp - 1).sum(1) >= 2) and got["kept"][1] > 0


@pytest.mark.gpu
def test_one_call_equals_many_and_a_resumed_run(fleet):
    w = fleet["w"]

    def start():
        h = _handle("sim", 30, 7)
        h.rollout_set_walls(fleet["walls"])
        h.rollout_set_obstacles(fleet["static"])
        h.rollout_set_movers(fleet["movers"])
        _init(h, "sim", [20] * 7)
        h.rollout_set_commitment(FLEET_KEEP)
        return h

    def end(h):
        out = (h.rollout_state(), h.rollout_corridor(), h.rollout_commitment())
        h.close()
        return out
    h = start()
    h.rollout_step(30)
    one = end(h)
    h = start()
    for _ in range(30):
        h.rollout_step(1)
    many = end(h)
    h = start()
    h.rollout_step(15)
    half = h.rollout_commitment()
    h.rollout_set_commitment(FLEET_KEEP, memory=(half["wp"], half["rows"]))      # (the setter zeroes the counters)
    h.rollout_step(15)
    resumed = end(h)
    for other in (many, resumed):
        _same_state(one[0], other[0])
        assert np.array_equal(one[1][0], other[1][0], equal_nan=True) and np.array_equal(one[1][1], other[1][1], equal_nan=True)
        assert np.array_equal(one[2]["wp"], other[2]["wp"]) and np.array_equal(one[2]["rows"], other[2]["rows"])
    for k in ("kept", "switched", "moved"):
        assert np.array_equal(one[2][k], many[2][k]) and np.array_equal(one[2][k], half[k] + resumed[2][k]), k
    assert np.array_equal(one[0]["wp_id"], fleet["wp"][29])      # and the fleet's step-by-step run is the same run


@pytest.mark.gpu
def test_off_means_off(fleet):
    def run(setting):
        h = _handle("sim", 30, 7)
        h.rollout_set_walls(fleet["walls"])
        h.rollout_set_obstacles(fleet["static"])
        h.rollout_set_movers(fleet["movers"])
        _init(h, "sim", [20] * 7)
        setting(h)
        h.rollout_step(30)
        out = (h.rollout_state(), h.rollout_corridor())
        h.close()
        return out
    never = run(lambda h: None)
    zeros = run(lambda h: h.rollout_set_commitment(np.zeros(7)))
    null = run(lambda h: (h.rollout_set_commitment(FLEET_KEEP), h.rollout_set_commitment(None)))
    for other in (zeros, null):
        _same_state(never[0], other[0])
        assert np.array_equal(never[1][0], other[1][0], equal_nan=True) and np.array_equal(never[1][1], other[1][1], equal_nan=True)


@pytest.mark.gpu
def test_with_perception_and_with_a_delay(fleet):
    """the known world changes under a committed car: a disc enters the row when the lidar first sees it; under a delay of 2 the
    rows belong to the predicted pose"""
    w = fleet["w"]
    from lidar_model import LidarModel
    lm = LidarModel(FoV=180, range=0.6, resolution=3)
    h = _handle("sim", 30, 7)
    h.rollout_set_walls(fleet["walls"])
    h.rollout_set_obstacles(fleet["static"])
    h.rollout_set_movers(fleet["movers"])
    h.rollout_set_perception(np.ascontiguousarray(lm.measurements[0], float), lm.range, 2)
    _init(h, "sim", [20] * 7)
    h.rollout_set_commitment(FLEET_KEEP)
    per_walls = [np.asarray(x, np.int32).reshape(-1, 4) for x in fleet["walls"]]
    f = Forced(w, h, FLEET_KEEP, per_walls)
    seen_late = False
    for k in range(25):
        h.rollout_step(1)
        p = h.rollout_perception()
        true = h.rollout_obstacles()
        planned = [np.where(((int(p["disc_known"][b]) >> np.arange(len(true[b]), dtype=object)) & 1).astype(bool)[:, None], true[b], 0)
                   .astype(np.int32).reshape(-1, 3) for b in range(7)]
        f.walls = [per_walls[b] if (int(p["wall_known"][b]) & 1) or len(per_walls[b]) == 0 else np.zeros((1, 4), np.int32) for b in range(7)]
        seen_late |= k > 0 and any(len(true[b]) and not (int(p["disc_known"][b]) & 1) for b in range(7))
        f.check(planned)
    h.close()
    assert seen_late      # a disc was still unknown after the first step: the known world did change under the committed cars
    h = _handle("sim", 30, 7)
    h.rollout_set_walls(fleet["walls"])
    h.rollout_set_obstacles(fleet["static"])
    h.rollout_set_movers(fleet["movers"])
    _init(h, "sim", [20] * 7)
    h.rollout_set_delay(np.full(7, 2, np.int32))
    h.rollout_set_commitment(FLEET_KEEP)
    f = Forced(w, h, FLEET_KEEP, fleet["walls"])
    for k in range(25):
        h.rollout_step(1)
        f.check()
    h.close()


@pytest.mark.gpu
def test_resets(lib):
    """rollout_init, the setter and a re-route empty the memory (the re-route: of the cars it accepts); a new disc list keeps it"""
    w = _track_world(lib, "sim", 30)
    keep = np.array([INF, INF, 0.0])
    d = [[w.disc(40, 0.0)]] * 3
    h = _handle("sim", 30, 3, routes=True)
    h.rollout_set_obstacles(d)
    _init(h, "sim", [20] * 3)
    h.rollout_set_commitment(keep)
    f = Forced(w, h, keep)
    for _ in range(3):
        h.rollout_step(1)
        st, got = f.check()
    assert np.all(got["wp"] >= 0) and got["kept"][0] > 0
    # a disc-list change keeps the memory: the next step is the twin's from the memory it had
    h.rollout_set_obstacles([[w.disc(40, 0.0), w.disc(44, 0.02)]] * 3)
    h.rollout_step(1)
    f.check()
    # a re-route of car 1 onto its own route: its memory is emptied, the others' stay
    acc = h.rollout_reroute([-1, 0, -1])
    assert acc.tolist() == [False, True, False]
    f.mem[0][1], f.mem[1][1] = K.EMPTY, 0.0
    h.rollout_step(1)
    st, got = f.check()
    # the setter: empty memory, counters zero
    h.rollout_set_commitment(keep)
    f.mem, f.counts = w.empty(3), np.zeros((3, 3), np.int32)
    h.rollout_step(1)
    st, got = f.check()
    assert got["kept"].sum() == 0
    # rollout_init: the setting stays, memory and counters start over
    h.rollout_step(1)
    f.check()
    _init(h, "sim", [20] * 3)
    f.mem, f.counts = w.empty(3), np.zeros((3, 3), np.int32)
    h.rollout_step(1)
    st, got = f.check()
    assert got["kept"].sum() == 0
    h.close()


def _code(e):
    return int(str(e.value).split("mpmpc error ")[1].split(":")[0])


@pytest.mark.gpu
def test_state_and_argument_errors(lib):
    w = _track_world(lib, "sim", 30)
    g1, grid, origin, res = _g1("sim")
    h = _handle("sim", 30, 3)
    _init(h, "sim", [20] * 3)
    keep = np.array([INF, 2.0, 0.0])
    for bad in ([0.5, 1, 1], [-1.0, 1, 1], [math.nan, 1, 1], [1.0] * 4):
        with pytest.raises(mpmpc.MpmpcError) as e:
            h.rollout_set_commitment(np.array(bad, float))
        assert _code(e) == E_ARG, bad
    h.rollout_set_commitment(keep)
    with pytest.raises(mpmpc.MpmpcError) as e:      # a refused call leaves the setting in force: the step still wants its world
        h.rollout_set_commitment(np.array([0.5, 1, 1]))
    with pytest.raises(mpmpc.MpmpcError) as e:      # the shared table has no per-car memory
        h.rollout_step(1)
    assert _code(e) == E_STATE and "per-car world" in str(e.value)
    h.rollout_set_obstacles([[]] * 3)
    with pytest.raises(mpmpc.MpmpcError) as e:      # the getter before a step
        h.rollout_commitment()
    assert _code(e) == E_STATE
    tr = scenarios.sim_track()
    h.rollout_set_lookahead(tr.ds_next / tr.v_ref, 5)
    with pytest.raises(mpmpc.MpmpcError) as e:      # lookahead in force
        h.rollout_step(1)
    assert _code(e) == E_STATE and "lookahead" in str(e.value)
    h.rollout_set_lookahead(None)
    h.rollout_step(2)
    got = h.rollout_commitment()
    assert np.all(got["wp"] >= 0) and got["kept"].sum() == 0      # an empty world: nothing to choose
    h.rollout_set_commitment(np.full(2, INF))
    with pytest.raises(mpmpc.MpmpcError) as e:      # another number of cars
        h.rollout_step(1)
    assert _code(e) == E_STATE
    h.rollout_set_commitment(keep)
    h.set_map(grid, origin, res)                    # a change of map: everything made on it is to be made again
    sm = _sm("sim")
    h.build_corridor(30, 2 * sm, sm, want_tables=False)
    h.rollout_set_obstacles([[]] * 3)
    _init(h, "sim", [20] * 3)
    with pytest.raises(mpmpc.MpmpcError) as e:
        h.rollout_step(1)
    assert _code(e) == E_STATE and "mpmpc_rollout_set_commitment" in str(e.value)
    h.rollout_set_commitment(keep)
    h.rollout_step(1)
    h.close()


@pytest.mark.gpu
def test_batchmpc_rollout_takes_a_commitment():
    """rollout(commitment=...): with no per-car world an empty one is put in force and the run is the plain one bit for bit; with
    obstacles the commitment's state comes back; with a lookahead it is refused; a later rollout has none again"""
    from MPC import BatchMPC
    from lookahead import Lookahead
    from map import Obstacle
    from scipy import sparse
    m, rp, car = T.build_world(obstacles=False)
    Q, R, QN = sparse.diags([1.0, 0.0, 0.0]), sparse.diags([0.5, 0.0]), sparse.diags([1.0, 0.0, 0.0])
    ic = {'umin': np.array([0.0, -np.tan(0.66) / car.length]), 'umax': np.array([1.0, np.tan(0.66) / car.length])}
    sc = {'xmin': np.array([-np.inf] * 3), 'xmax': np.array([np.inf] * 3)}
    B, N, steps = 4, 30, 12
    bm = BatchMPC(car, N, Q, R, QN, sc, ic, 4.0, max_batch=B, corridor="device")
    cum = np.cumsum(rp.segment_lengths)
    wp = rp.waypoints[20]
    s0, poses = np.full(B, cum[20]), np.tile([wp.x, wp.y, wp.psi], (B, 1))
    plain = bm.rollout(s0, poses, steps)
    kept = bm.rollout(s0, poses, steps, commitment=Commitment())
    c = kept.pop("commitment")
    assert np.all(c["kept"] == 0) and np.all(c["moved"] == 0) and np.all(c["wp"] >= 0)
    _same_state(plain, kept)
    w = rp.waypoints[40]
    obs = [[Obstacle(w.x, w.y, 0.04)]] * B
    out = bm.rollout(s0, poses, steps, obstacles=obs, commitment=Commitment([0.0, INF, 4.0, 1.0]))
    c = out["commitment"]
    assert c["kept"][0] == 0 and np.all(c["kept"][1:] > 0) and set(c) == set(mpmpc.Handle.COMMITMENT_FIELDS)
    assert bm.rollout(s0, poses, 0, obstacles=obs, commitment=Commitment())["commitment"] is None
    with pytest.raises(ValueError, match="lookahead"):
        bm.rollout(s0, poses, steps, obstacles=obs, commitment=Commitment(), lookahead=Lookahead(5))
    again = bm.rollout(s0, poses, steps)
    assert "commitment" not in again
    _same_state(plain, again)
    with pytest.raises(mpmpc.MpmpcError):
        bm.handle.rollout_commitment()
