"""Lidar localisation of the device rollout: the distance field K0d and the scan match K3l (csrc/localiser_core.hpp,
csrc/mpmpc_localiser.hpp, localiser.py).  CPU: the twin (the header compiled for the host, tests/emul_localiser) against numpy -
the field against brute force, the match against Localiser.match, the tie-break, the range noise, the step, the argument checks,
the python surface - and whether it localises at all.  GPU: off changes nothing, K0d and the match against the twin (bit for bit
outside the band in which another libm's cos / sin may choose another cell), K3l step by step in rollouts with and without
plant, delay, routes and a world the base map does not hold, one call against many and a resumed run, the schedule, cars that
end, whether it helps, the error codes, BatchMPC."""
import ctypes as C
import inspect
import math
import types

import numpy as np
import pytest

import mpmpc
import mpmpc_testlib as T
import localiser_twin
import twins
import test_delay as TD      # (its Sim_Track starts and state comparisons)
import test_lidar as TL      # (the lidar twin's scans)
import test_traffic as TT    # (its Sim_Track handle on the device's map)
from delay import Delay, nominal
from estimator import Estimator, wrap
from localiser import COUNTS, STATS, Localiser, fresh
from plant import Plant, philox4x32, variate

E_ARG, E_STATE = -1, -3
TS, L_CAR = TD.TS, TD.L_CAR
BAND = 1e-9      # cells: a case whose nearest endpoint lies closer to a cell boundary is not compared across libms
_same_bits, _equal_states, _code, _starts, _in_flight = TD._same_bits, TD._equal_states, TD._code, TD._starts, TD._in_flight
dp, cip, i8p, u8p = localiser_twin.dp, localiser_twin.cip, localiser_twin.i8p, localiser_twin.u8p


def _d(a):
    return None if a is None else a.ctypes.data_as(dp)


def _i(a):
    return a.ctypes.data_as(cip)


@pytest.fixture(scope="module")
def twin():
    """The CPU twin of K0d / K3l (tests/emul_localiser)."""
    return localiser_twin.localiser()


@pytest.fixture(scope="module")
def lid():
    return twins.lidar()


def _lidar(n_beams=None, fov=270.0, reso=3.0, rng=1.0):
    """what Localiser takes of a lidar_model.LidarModel (constructing that one would load the device library)"""
    ang = TL._angles(fov, reso) if n_beams is None else (np.zeros(1) if n_beams == 1 else np.linspace(-2.3, 2.3, n_beams))
    return types.SimpleNamespace(measurements=np.stack([ang, np.full(ang.size, rng)]), range=rng)


def _sim_map():
    g1, grid, origin, res = T.g1_world("sim")
    return g1, np.ascontiguousarray(grid, np.int8), origin, res


def _twin_field(twin, grid, D):
    grid = np.ascontiguousarray(grid, np.int8)
    out = np.zeros(grid.shape, np.uint8)
    twin.lc_emu_field(grid.shape[0], grid.shape[1], grid.ctypes.data_as(i8p), int(D), out.ctypes.data_as(u8p))
    return out


def _twin_match(twin, L, grid, origin, res, priors, ranges, hit=None, field=None):
    grid = np.ascontiguousarray(grid, np.int8)
    field = _twin_field(twin, grid, L.D) if field is None else np.ascontiguousarray(field, np.uint8)
    pr = np.ascontiguousarray(priors, float).reshape(-1, 3)
    B = pr.shape[0]
    rg = np.ascontiguousarray(ranges, float).reshape(B, L.angles.size)
    ht = None if hit is None else np.ascontiguousarray(hit, np.uint8).reshape(B, L.angles.size)
    out = dict(fix=np.full((B, 3), 7.0), score=np.full(B, -7, np.int32), cand=np.full(B, -7, np.int32), hits=np.full(B, -7, np.int32),
               min_edge=np.full(B, -7.0))
    twin.lc_emu_match(grid.shape[0], grid.shape[1], grid.ctypes.data_as(i8p), field.ctypes.data_as(u8p), origin[0], origin[1], res, B, _d(pr),
                      _d(rg), None if ht is None else ht.ctypes.data_as(u8p), L.angles.size, _d(L.angles), L.range, L.D, L.m, L.W, L.T,
                      L.step_psi, L.min_hits, _d(out["fix"]), _i(out["score"]), _i(out["cand"]), _i(out["hits"]), _d(out["min_edge"]))
    return out


def _equal_matches(a, b, keys=("fix", "score", "cand", "hits", "min_edge")):
    for k in keys:
        same = np.array_equal(a[k], b[k]) if a[k].dtype.kind == "i" else _same_bits(a[k], b[k])
        assert same, (k, a[k], b[k])


def _brute_field(grid, D):
    """min(cap, min d2) by definition, every cell against every occupied cell"""
    H, W = grid.shape
    jj, ii = np.nonzero(np.asarray(grid) == 0)
    j, i = np.mgrid[0:H, 0:W]
    out = np.full((H, W), D * D + 1, np.int64)
    if jj.size:
        dj, di = jj[None, None, :] - j[:, :, None], ii[None, None, :] - i[:, :, None]
        d2 = di * di + dj * dj
        ok = (np.abs(di) <= D) & (np.abs(dj) <= D) & (d2 <= D * D)
        out = np.minimum(out, np.where(ok, d2, D * D + 1).min(axis=2))
    return out.astype(np.uint8)


FIELD_GRIDS = {
    "random": lambda: (np.random.default_rng(1).random((33, 40)) > 0.06).astype(np.int8),
    "narrow": lambda: (np.random.default_rng(2).random((3, 50)) > 0.1).astype(np.int8),
    "free": lambda: np.ones((20, 17), np.int8),
    "border": lambda: np.pad(np.ones((18, 25), np.int8), 1),
}


# ------------------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("D", [1, 4, 15])
@pytest.mark.parametrize("name", sorted(FIELD_GRIDS))
def test_field_equals_brute_force(twin, name, D):
    grid = FIELD_GRIDS[name]()
    want = _brute_field(grid, D)
    got = _twin_field(twin, grid, D)
    assert np.array_equal(got, want)
    L = Localiser(_lidar(), D, 1, 0, 0, 0.0)
    assert np.array_equal(L.field(grid), want) and np.array_equal(L.field(types.SimpleNamespace(data=grid)), want)
    assert want.max() <= D * D + 1 and (name != "free" or np.all(want == D * D + 1))
    if name == "border":
        assert np.all(want[0] == 0) and np.all(want[:, -1] == 0) and want[1, 1] == 1
    H, W = grid.shape
    for i, j in ((-1, 0), (0, -1), (W, 0), (0, H), (-2 ** 40, 3), (3, 2 ** 40)):      # outside the grid: cap
        assert twin.lc_emu_field_at(got.ctypes.data_as(u8p), W, H, D, i, j) == D * D + 1
    assert twin.lc_emu_field_at(got.ctypes.data_as(u8p), W, H, D, W - 1, H - 1) == want[H - 1, W - 1]


MATCH_CASES = [(1, 0, 0), (1, 3, 2), (61, 0, 0), (61, 8, 1), (61, 3, 2), (257, 8, 1), (257, 0, 0)]


def _match_inputs(lid, n_beams, W, T, seed=5, B=64):
    """64 (prior, scan) pairs on Sim_Track: scans of the lidar twin from random poses near the path, priors displaced by up to
    4 cells and 0.04 rad; the last pairs are the edge cases - a prior off the map, a NaN prior, min_hits - 1 and min_hits hits"""
    g1, grid, origin, res = _sim_map()
    rng = np.random.default_rng(seed + 100 * n_beams + 10 * W + T)
    L = Localiser(_lidar(n_beams, rng=0.6), D=5, step_cells=1 + (W > 3), window=W, headings=T, step_psi=0.02 if T else 0.0, min_hits=1)
    w = rng.integers(0, 200, B)
    poses = np.stack([g1["x"][w] + rng.uniform(-0.02, 0.02, B), g1["y"][w] + rng.uniform(-0.02, 0.02, B),
                      g1["psi"][w] + rng.uniform(-0.3, 0.3, B)], 1)
    ranges, _ = TL._twin_scan(lid, grid, origin, res, poses, L.angles, L.range)
    priors = poses + np.stack([rng.uniform(-4, 4, B) * res, rng.uniform(-4, 4, B) * res, rng.uniform(-0.04, 0.04, B)], 1)
    priors[B - 1] = (origin[0] - 50.0, origin[1] + 0.3, 0.4)      # off the map: every endpoint off the grid
    priors[B - 2] = (np.nan, priors[B - 2, 1], 0.0)
    priors[B - 3, 2] = np.inf
    ranges[B - 4] = L.range      # no hit at all
    ranges[B - 1] = 0.5 * L.range      # (every beam of the pair off the map is a hit)
    return L, grid, origin, res, priors, ranges


@pytest.mark.parametrize("n_beams,W,T", MATCH_CASES)
def test_match_twin_equals_numpy(twin, lid, n_beams, W, T):
    L, grid, origin, res, priors, ranges = _match_inputs(lid, n_beams, W, T)
    B = priors.shape[0]
    got = _twin_match(twin, L, grid, origin, res, priors, ranges)
    want = L.match(grid, origin, res, priors, ranges)
    _equal_matches(got, want)
    assert L.n_candidates == (2 * T + 1) * (2 * W + 1) ** 2 and (W, T) != (8, 1) or L.n_candidates == 867
    centre = (T * (2 * W + 1) + W) * (2 * W + 1) + W
    assert got["cand"][B - 1] == centre and _same_bits(got["fix"][B - 1], priors[B - 1])      # all-cap scores: dead reckoning
    assert got["score"][B - 1] == n_beams * L.cap and got["hits"][B - 1] == n_beams
    for i in (B - 2, B - 3, B - 4):      # a prior that is not finite, no hits: no match, the fix is the prior
        assert got["cand"][i] == -1 and got["score"][i] == -1 and _same_bits(got["fix"][i], priors[i])
    assert got["hits"][B - 4] == 0
    moved = (got["cand"][:B - 4] >= 0) & (got["cand"][:B - 4] != centre)
    assert W == 0 or moved.sum() > B // 4
    # min_hits - 1 and min_hits hits
    h0 = int(got["hits"][0])
    if h0 >= 1:
        for need, matched in ((h0, True), (h0 + 1, False)):
            Lh = Localiser(_lidar(n_beams, rng=0.6), L.D, L.m, W, T, L.step_psi, min_hits=need)
            one = _twin_match(twin, Lh, grid, origin, res, priors[:1], ranges[:1])
            assert (one["cand"][0] >= 0) == matched and one["hits"][0] == h0
            _equal_matches(one, Lh.match(grid, origin, res, priors[:1], ranges[:1]))


def test_the_tie_break(twin):
    """one beam straight ahead of a prior in a cell's centre: score(a, c) = F(ci + a, cj + c)"""
    H, W_ = 48, 64
    origin, res = (0.0, 0.0), 0.1
    L = Localiser(_lidar(1, rng=5.0), D=3, step_cells=1, window=6, headings=1, step_psi=0.001, min_hits=1)
    prior = np.array([[20.5 * res, 24.5 * res, 0.0]])
    ranges = np.array([[10.0 * res]])      # the endpoint: cell (30, 24)
    centre = (1 * 13 + 6) * 13 + 6
    free = np.ones((H, W_), np.int8)
    m = _twin_match(twin, L, free, origin, res, prior, ranges)      # an all-cap field: the centre candidate, dead reckoning
    assert m["cand"][0] == centre and m["score"][0] == L.cap and _same_bits(m["fix"], prior)
    _equal_matches(m, L.match(free, origin, res, prior, ranges))
    for cells, want in (([(31, 24), (27, 24)], (1, 0, 0)),        # two zeros, at a = 1 and a = -3: the one nearer the centre
                        ([(30, 26), (25, 24)], (0, 2, 0)),        # ... at c = 2 and a = -5
                        ([(32, 24), (28, 24)], (-2, 0, 0)),       # equally near: the lower idx
                        ([(30, 24)], (0, 0, 0))):                 # under the endpoint: three headings tie, t = 0 wins
        grid = free.copy()
        for i, j in cells:
            grid[j, i] = 0
        m = _twin_match(twin, L, grid, origin, res, prior, ranges)
        assert L.candidate(m["cand"][0]) == want and m["score"][0] == 0, (cells, L.candidate(m["cand"][0]))
        assert _same_bits(m["fix"][0], prior[0] + np.array([want[0] * res, want[1] * res, 0.0]))
        _equal_matches(m, L.match(grid, origin, res, prior, ranges))


def test_range_noise(twin):
    """the twin's noise is the numpy restatement's; a draw depends on (seed, car0 + car, j, beam) only; blocks 16 .. 527"""
    L = Localiser(_lidar(61, rng=0.6), 5, 1, 2, 0, 0.0, sigma_r=0.013, seed=0xDEADBEEF12345678, car0=7, step0=-4)
    B, n = 9, L.angles.size
    rng = np.random.default_rng(3)
    raw = np.where(rng.random((B, n)) < 0.7, rng.uniform(0.0, 0.6, (B, n)), 0.6)
    raw[0, 0] = np.nan
    for k in (0, 1, 17, 2 ** 33):
        want, hit = L.noisy(k, raw)
        got, got_hit = raw.copy(), np.zeros((B, n), np.uint8)
        for i in range(B):
            twin.lc_emu_noise(L.sigma_r, L.seed & 0xFFFFFFFFFFFFFFFF, L.car0 + i, k - L.step0, n, L.range, _d(got[i]), got_hit[i].ctypes.data_as(u8p))
        assert _same_bits(got, want) and np.array_equal(got_hit.astype(bool), hit) and np.array_equal(hit, raw < 0.6)
        assert _same_bits(got[~hit], raw[~hit]) and np.all(got[hit] != raw[hit]) and np.all(np.abs(got[hit] - raw[hit]) < L.sigma_r)
        assert _same_bits(L.car(3).variates(k, 2), L.variates(k, B)[3:5])      # independent of B and of the other cars
    assert not np.array_equal(L.variates(0, 1), L.variates(1, 1))
    # the blocks: beam b is word b & 3 of block 16 + (b >> 2) - none of 0 .. 2 (the plant's and the estimator's)
    full = Localiser(_lidar(2048, rng=0.6), 5, 1, 0, 0, 0.0, sigma_r=1.0, seed=5, car0=2)
    v = full.variates(6, 1)[0]
    key = np.array([5, 0], np.uint64)
    for b in (0, 3, 4, 2047):
        blk = 16 + (b >> 2)
        assert 16 <= blk <= 527
        assert v[b] == variate(philox4x32(np.array([2, 6, 0, blk], np.uint64), key))[b & 3]


def _check(twin, L=None, fix0=None, B=4, res=0.005, **kw):
    a = dict(angles=np.linspace(-1, 1, 9), range_m=0.5, D=5, m=1, W=3, T=2, step_psi=0.01, min_hits=3, sigma_r=0.0, period=1)
    a.update(kw)
    ang = None if a["angles"] is None else np.ascontiguousarray(a["angles"], float)
    why = C.c_char_p()
    rc = twin.lc_emu_check(0 if ang is None else ang.size, _d(ang), a["range_m"], res, a["D"], a["m"], a["W"], a["T"], a["step_psi"],
                           a["min_hits"], a["sigma_r"], a["period"], B, _d(fix0), C.byref(why))
    return rc, why.value.decode()


def test_argument_checks(twin):
    assert _check(twin) == (0, "")
    assert _check(twin, fix0=np.zeros((4, 3))) == (0, "")
    for kw, word in ((dict(D=0), "D must be in [1, 15]"), (dict(D=16), "D must be in [1, 15]"), (dict(m=0), "translation step"),
                     (dict(W=-1), "W must be in [0, 16]"), (dict(W=17), "W must be in [0, 16]"), (dict(T=-1), "T must be in [0, 8]"),
                     (dict(T=9), "T must be in [0, 8]"), (dict(step_psi=-0.1), "step_psi"), (dict(step_psi=np.nan), "step_psi"),
                     (dict(step_psi=np.inf), "step_psi"), (dict(step_psi=0.0), "> 0 when T > 0"), (dict(min_hits=0), "min_hits"),
                     (dict(sigma_r=-1e-3), "sigma_r"), (dict(sigma_r=np.nan), "sigma_r"), (dict(sigma_r=np.inf), "sigma_r"),
                     (dict(period=0), "period"), (dict(angles=np.linspace(-1, 1, 1639)), "at most 8192"),
                     (dict(angles=np.array([0.0, -0.1])), "ascending"), (dict(angles=np.array([0.0, np.nan])), "not finite"),
                     (dict(angles=np.zeros(2049), T=0, step_psi=0.0), "n_beams must be in [1, 2048]"), (dict(angles=None), "n_beams"),
                     (dict(range_m=0.0), "range must be positive"), (dict(range_m=np.inf), "range must be positive"),
                     (dict(range_m=11.0), "more than 2048 cells")):
        rc, why = _check(twin, **kw)
        assert rc == -1 and word in why, (kw, why)
    assert _check(twin, T=0, step_psi=0.0) == (0, "")
    assert _check(twin, angles=np.linspace(-1, 1, 1638)) == (0, "")      # 5 * 1638 = 8190
    bad = np.zeros((4, 3))
    bad[3, 1] = np.inf
    rc, why = _check(twin, fix0=bad)
    assert rc == -1 and "fix0 must be finite" in why
    # the python class refuses the same
    for kw in (dict(D=0), dict(step_cells=0), dict(window=17), dict(headings=9), dict(step_psi=-1.0), dict(min_hits=0), dict(sigma_r=-1.0),
               dict(period=0), dict(step_psi=0.0)):
        a = dict(D=5, step_cells=1, window=3, headings=2, step_psi=0.01)
        a.update(kw)
        with pytest.raises(ValueError, match="localiser"):
            Localiser(_lidar(), **a)
    with pytest.raises(ValueError, match="8192"):
        Localiser(_lidar(1639), 5, 1, 3, 2, 0.01)


def test_python_surface():
    from MPC import BatchMPC
    assert "localiser" in inspect.signature(BatchMPC.rollout).parameters
    for name in ("rollout_set_localiser", "rollout_localiser"):
        assert hasattr(mpmpc.Handle, name)
    assert hasattr(mpmpc, "distance_field") and hasattr(mpmpc, "scan_match")
    assert mpmpc.Handle.LOCALISER_FIELDS == ("fix", "prior", "cand", "score", "hits", "ranges") + STATS + COUNTS
    header = open(T.ROOT + "/include/mpmpc.h").read()
    for name in ("mpmpc_distance_field", "mpmpc_scan_match", "mpmpc_rollout_set_localiser", "mpmpc_rollout_localiser"):
        assert name in mpmpc.EXPORTS and "int %s(" % name in header
    assert set(fresh(2, 5)) == set(mpmpc.Handle.LOCALISER_FIELDS) | {"primed"} and fresh(2, 5)["ranges"].shape == (2, 5)
    L = Localiser(_lidar(), 6, 2, 3, 1, 0.02, min_hits=4, sigma_r=0.01, period=3, seed=9, car0=1, step0=-2)
    assert set(L.setting()) == set(inspect.signature(mpmpc.Handle.rollout_set_localiser).parameters) - {"self", "B", "fix0"}
    assert L.cap == 37 and L.n_candidates == 3 * 49 and L.candidate(0) == (-3, -3, -1) and L.candidate(3 * 49 - 1) == (3, 3, 1)
    assert L.scheduled(-2) and not L.scheduled(0) and L.scheduled(1) and L.car(4).car0 == 5
    core = open(T.ROOT + "/multi-purpose-mpc_amd/csrc/plant_core.hpp").read()
    assert "Blocks 16 .. 527" in core


def test_batchmpc_refuses_bad_combinations():
    """ValueError before any device call: the stand-in's handle fails on every use"""
    from MPC import BatchMPC

    class NoDevice:
        def __getattr__(self, name):
            raise AssertionError("device call: " + name)
    bm = BatchMPC.__new__(BatchMPC)
    bm._path, bm.corridor_cols, bm.handle = types.SimpleNamespace(), None, NoDevice()
    L = Localiser(_lidar(), 6, 1, 3, 1, 0.02)
    with pytest.raises(ValueError, match="localiser needs corridor='device'"):
        bm.rollout(np.zeros(2), np.zeros((2, 3)), 1, localiser=L)
    bm.corridor_cols = 30
    with pytest.raises(ValueError, match="localiser and an assumed delay of 8"):
        bm.rollout(np.zeros(2), np.zeros((2, 3)), 1, localiser=L, delay=Delay(8))
    with pytest.raises(ValueError, match="localiser and an assumed delay of 8"):
        bm.rollout(np.zeros(2), np.zeros((2, 3)), 1, localiser=L, delay=Delay(2, assumed=[1, 8]))
    with pytest.raises(AssertionError, match="device call"):      # (an assumed delay below 8 passes the argument checks)
        bm.rollout(np.zeros(2), np.zeros((2, 3)), 1, localiser=L, delay=Delay(8, assumed=7))


def _twin_step(twin, L, car, k, grid, field, origin, res, ranges, pose, cmd, st):
    """K3l of the twin for one car on the state dict `st` (fresh's keys, one car's values), in place"""
    fix, prior = np.array(st["fix"], float), np.zeros(3)
    primed, cand, score, hits = C.c_int(int(st["primed"])), C.c_int(-7), C.c_int(-7), C.c_int(-7)
    stats, cnt = np.array([st[k_] for k_ in STATS], float), np.array([st[k_] for k_ in COUNTS], np.int32)
    rg = np.array(ranges, float)
    twin.lc_emu_step(grid.shape[0], grid.shape[1], grid.ctypes.data_as(i8p), field.ctypes.data_as(u8p), origin[0], origin[1], res, L.D, L.m, L.W,
                     L.T, L.step_psi, L.min_hits, L.sigma_r, L.period, L.seed & 0xFFFFFFFFFFFFFFFF, L.car0 + car, k - L.step0, L_CAR, TS,
                     L.angles.size, _d(L.angles), L.range, _d(rg), _d(np.ascontiguousarray(pose, float)), _d(np.ascontiguousarray(cmd, float)),
                     _d(fix), _d(prior), C.byref(primed), C.byref(cand), C.byref(score), C.byref(hits), _d(stats), _i(cnt))
    out = dict(fix=fix, prior=prior, primed=primed.value, cand=cand.value, score=score.value, hits=hits.value, ranges=rg)
    out.update(dict(zip(STATS, stats)), **dict(zip(COUNTS, cnt)))
    return out


def test_step_twin_equals_numpy(twin, lid):
    """an open loop of 12 steps, 6 cars: the true car drives a mismatched model, the localiser dead-reckons with the nominal one;
    period 2, range noise, and a car that loses its hits for two steps"""
    g1, grid, origin, res = _sim_map()
    B, steps = 6, 12
    L = Localiser(_lidar(61, rng=0.6), D=5, step_cells=1, window=3, headings=1, step_psi=0.01, min_hits=4, sigma_r=0.004, period=2, seed=11,
                  car0=3, step0=-1)
    field = _twin_field(twin, grid, L.D)
    w = np.array([3, 40, 77, 110, 150, 190])
    pose = np.stack([g1["x"][w], g1["y"][w], g1["psi"][w]], 1)
    st = fresh(B, L.angles.size)
    seen = dict(matched=0, lost=0, unscheduled=0)
    for k in range(steps):
        cmd = np.stack([np.full(B, 0.6), 0.1 * np.sin(0.3 * k + np.arange(B))], 1)
        ranges, _ = TL._twin_scan(lid, grid, origin, res, pose, L.angles, L.range)
        if k in (5, 7):
            ranges[2, 3:] = L.range      # three hits at most: lost
        new = L.update(k, pose, cmd, ranges, st, grid, origin, res, L_CAR, TS, field=field)
        for i in range(B):
            one = _twin_step(twin, L, i, k, grid, field, origin, res, ranges[i], pose[i], cmd[i], {k_: v[i] for k_, v in st.items()})
            for k_ in ("fix", "prior") + STATS:
                assert _same_bits(one[k_], new[k_][i]), (k, i, k_)
            for k_ in ("cand", "score", "hits") + COUNTS:
                assert one[k_] == new[k_][i], (k, i, k_)
            if one["hits"] >= 0:
                assert _same_bits(one["ranges"], new["ranges"][i]), (k, i)
        seen["matched"] += int((new["cand"] >= 0).sum())
        seen["unscheduled"] += int((new["hits"] < 0).sum())
        st = new
        pose = np.array([nominal(tuple(pose[i]), 0.0, 1.04 * cmd[i, 0], cmd[i, 1] + 0.02, 0.0, 0.0, 0.0, 1.05 * L_CAR, TS)[0] for i in range(B)])
    assert np.all(st["steps"] == steps) and st["lost"][2] == 2 and st["lost"].sum() == 2 and seen["matched"] > 4 * B
    assert np.array_equal(st["matched"] + st["lost"], np.full(B, 6)) and seen["unscheduled"] == B * 6      # scans at k = 1, 3, .. 11


LOCALISES = dict(offset=(3, -2), D=6, W=4, T=1, step_psi=0.03)


def _sound_waypoints(ahead=1):
    """Sim_Track's waypoints whose heading - and that of the `ahead` - 1 waypoints behind them - lies in (-3.0, -0.05).  K0l is the
    reference's lidar, and that wraps a cell's angle atan2(dy, dx) - psi by MIRRORING it when it is below -pi
    (csrc/lidar_core.hpp, step 3): at a heading above 0 - and at every heading ro_drive has carried past pi - the cells behind
    the car on its right are reported by the beams behind it on its left, and the scan is not the map's.  At headings in
    [-pi, 0] no angle falls below -pi and the scan is geometrically the map's; the tests that ask whether matching HELPS take
    their poses there ("K0d / K3l")."""
    psi = TD._sim()[0]["psi"]
    n = psi.size
    return np.array([w for w in range(n) if all(-3.0 < psi[(w + q) % n] < -0.05 for q in range(ahead))])


def _localises_inputs(lid):
    """the poses at Sim_Track's waypoints with a heading in (-3.0, -0.05), scanned in the base map; the priors displaced by (3, -2)
    cells - three and two candidate steps, inside the window of 4.  Chosen on the CPU: the twin alone satisfies the assertion
    (profiles/localiser/README.md)."""
    g1, grid, origin, res = _sim_map()
    c = LOCALISES
    L = Localiser(_lidar(rng=1.0), D=c["D"], step_cells=1, window=c["W"], headings=c["T"], step_psi=c["step_psi"])
    w = _sound_waypoints()
    poses = np.stack([g1["x"][w] + 0.0011, g1["y"][w] - 0.0007, g1["psi"][w]], 1)      # (off the cells' centres and borders)
    ranges, _ = TL._twin_scan(lid, grid, origin, res, poses, L.angles, L.range)
    priors = poses + np.array([c["offset"][0] * res, c["offset"][1] * res, 0.0])
    return L, grid, origin, res, poses, priors, ranges


def _position_errors(fix, priors, poses):
    return (float(np.hypot(*(fix[:, :2] - poses[:, :2]).T).sum()), float(np.hypot(*(priors[:, :2] - poses[:, :2]).T).sum()))


def test_it_localises(twin, lid):
    """the summed position error of the fixes is below that of the priors; no threshold is fixed.  Twin: 0.3035 m against
    1.2439 m over the 69 poses (printed below)."""
    L, grid, origin, res, poses, priors, ranges = _localises_inputs(lid)
    m = _twin_match(twin, L, grid, origin, res, priors, ranges)
    e_fix, e_prior = _position_errors(m["fix"], priors, poses)
    print("it localises (twin): summed position error of the fixes %.4f m, of the priors %.4f m; min_edge %.2e" %
          (e_fix, e_prior, m["min_edge"].min()))
    assert np.all(m["cand"] >= 0) and e_fix < e_prior


# ------------------------------------------------------------------------------------------------------------ GPU
def _set(h, L, B, **kw):
    a = L.setting()
    a.update(kw)
    h.rollout_set_localiser(B, **a)


def _handle(N, B):
    """Sim_Track on the device's map, the corridor built from it"""
    h, _ = TT._handle("sim", N, B)
    return h


def _cum():
    return TD._sim()[2]


def _equal_outside_band(got, want, what=""):
    """fix, score, cand and hits bit for bit wherever the twin's nearest endpoint is at least BAND from a cell boundary;
    -> the number of cases left out"""
    keep = ~(want["min_edge"] < BAND)
    assert np.array_equal(got["hits"], want["hits"]), what
    for k in ("score", "cand"):
        assert np.array_equal(got[k][keep], want[k][keep]), (what, k, np.flatnonzero(got[k] != want[k]))
    assert _same_bits(got["fix"][keep], want["fix"][keep]), what
    return int((~keep).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(FIELD_GRIDS) + ["sim"])
def test_device_field_equals_the_twin(twin, name):
    grid = _sim_map()[1] if name == "sim" else FIELD_GRIDS[name]()
    for D in (1, 6, 15):
        assert np.array_equal(mpmpc.distance_field(grid, D), _twin_field(twin, grid, D)), D
    for D in (0, 16):
        with pytest.raises(mpmpc.MpmpcError, match="D must be in"):
            mpmpc.distance_field(grid, D)


@pytest.mark.gpu
@pytest.mark.parametrize("n_beams,W,T", MATCH_CASES + [(1638, 1, 2)])
def test_device_match_equals_the_twin(twin, lid, n_beams, W, T):
    """the CPU cases, and 5 * 1638 = 8 190 endpoint cells (all of the workgroup's LDS the law allows)"""
    L, grid, origin, res, priors, ranges = _match_inputs(lid, n_beams, W, T, B=64 if n_beams < 1000 else 8)
    want = _twin_match(twin, L, grid, origin, res, priors, ranges)
    got = mpmpc.scan_match(grid, origin, res, priors, ranges, L.angles, L.range, L.D, L.m, L.W, L.T, L.step_psi, L.min_hits)
    skipped = _equal_outside_band(got, want)
    print("scan_match against the twin, n_beams=%d W=%d T=%d: %d of %d cases in the band" % (n_beams, W, T, skipped, priors.shape[0]))
    assert 100 * skipped <= priors.shape[0]


@pytest.mark.gpu
def test_it_localises_on_the_device(twin, lid):
    L, grid, origin, res, poses, priors, ranges = _localises_inputs(lid)
    got = mpmpc.scan_match(grid, origin, res, priors, ranges, L.angles, L.range, L.D, L.m, L.W, L.T, L.step_psi, L.min_hits)
    e_fix, e_prior = _position_errors(got["fix"], priors, poses)
    print("it localises (device): summed position error of the fixes %.4f m, of the priors %.4f m" % (e_fix, e_prior))
    assert np.all(got["cand"] >= 0) and e_fix < e_prior
    assert _equal_outside_band(got, _twin_match(twin, L, grid, origin, res, priors, ranges)) == 0


@pytest.mark.gpu
def test_off_changes_nothing():
    """the localiser set and switched off (before the rollout starts, and again between its steps) against a handle that never
    had it: the same bits"""
    N, B, steps = 10, 64, 20
    w, s0, poses = _starts(B, 41)
    L = Localiser(_lidar(), 6, 1, 3, 1, 0.02, sigma_r=0.002, period=2, seed=5)
    out = []
    for touched in (False, True):
        h = _handle(N, B)
        if touched:
            _set(h, L, B)
            h.rollout_set_localiser(0)
        h.rollout_init(TS, _cum(), s0, poses)
        h.rollout_step(steps // 2)
        if touched:
            _set(h, L, B)
            h.rollout_set_localiser(0)
            with pytest.raises(mpmpc.MpmpcError):
                h.rollout_localiser()
        h.rollout_step(steps - steps // 2)
        out.append(h.rollout_state())
        h.close()
    _equal_states(out[1], out[0])
    assert (out[0]["alive"] == 1).sum() > B // 2


WORLD_DISCS = 2      # per car: one static disc and one mover that the base map does not hold


def _step_setup(case, B, N):
    """-> (handle, cum, s0, poses, route-aware path data or None)"""
    g1, grid, origin, res = _sim_map()
    if case == "two_routes":
        cat, first, circ = TD._two_routes()
        route = (np.arange(B) % 2).astype(np.int32)
        wp = np.where(route == 0, np.arange(B) * 11 % 180, np.arange(B) * 5 % 60).astype(int)
        g = first[route] + wp
        h = mpmpc.Handle(T.stock_config(N, max_batch=B, circular=False))
        h.set_path(cat["kappa"], cat["v_ref"], cat["ds_next"])
        h.set_corridor(cat["ub"], cat["lb"])
        h.set_routes(first, circ)
        h.set_path_geometry(cat["x"], cat["y"], cat["psi"], cat["border_ub"], cat["border_lb"])
        h.set_car_routes(route)
        h.set_map(grid, origin, res)
        return h, cat["cum_lengths"], cat["cum_lengths"][g], np.stack([cat["x"][g] + 0.00113, cat["y"][g] - 0.00071, cat["psi"][g]], 1)
    h = _handle(N, B)
    w, s0, poses = _starts(B, 42, last=160)
    w[0], s0[0], poses[0] = 198, _cum()[198], (g1["x"][198], g1["y"][198], g1["psi"][198])      # finishes the lap within the run
    poses = poses + np.array([0.00113, -0.00071, 0.0])      # (off the waypoints' lattice: no endpoint on a cell boundary to 1e-9)
    if case == "world":
        from map import Map, Obstacle
        m = Map.from_grid(grid, origin, res)
        cum = _cum()
        static = [m.obstacle_discs([Obstacle(g1["x"][(w[b] + 12) % 200] + 0.03, g1["y"][(w[b] + 12) % 200] - 0.02, 0.04)]) for b in range(B)]
        rows = [np.array([(1, 6, cum[(w[b] + 7) % cum.size], 0.05, 0.004, 0.0)]) for b in range(B)]
        h.rollout_set_obstacles(static)
        h.rollout_set_movers(rows)
    return h, _cum(), s0, poses


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["plain", "plant", "delay", "plant_delay", "two_routes", "world"])
def test_k3l_matches_the_twin_step_by_step(twin, case):
    """one step per call.  The twin's prior comes from the device's last fix and command (u, or entry c of the register) and may
    differ from the device's by what cos / sin / tan differ by (4 ulp of a result below 1 through Ts v and Ts v / L, as K3e's
    test bounds it); the match then runs on the DEVICE's prior and ranges: fix, candidate, score and hits bit for bit outside the
    band, the counters equal, the sums to 1e-12 relative.  Cars that are not running are not written."""
    N, B, steps = 10, 16, 14
    g1, grid, origin, res = _sim_map()
    h, cum, s0, poses = _step_setup(case, B, N)
    L = Localiser(_lidar(rng=0.8), D=6, step_cells=1, window=3, headings=1, step_psi=0.01, min_hits=5, period=1 if case != "delay" else 2,
                  seed=3, car0=1)
    field = _twin_field(twin, grid, L.D)
    plant = Plant(seed=7, **dict(TD.NOISY, position_noise=0.0, heading_noise=0.0)) if case.startswith("plant") else None
    delayed = case.endswith("delay")
    c = (np.arange(B) % 3).astype(np.int32)
    if plant is not None:
        h.rollout_set_plant(plant.params(B), plant.seed)
    h.rollout_init(TS, cum, s0, poses)
    if delayed:
        h.rollout_set_delay(c, c, _in_flight(B))
    _set(h, L, B)
    prev = fresh(B, L.angles.size)
    u_prev, q_prev = np.zeros((B, 2)), _in_flight(B)
    mine = {k: np.zeros(B) for k in STATS}
    cnt = {k: np.zeros(B, np.int32) for k in COUNTS}
    skipped = compared = 0
    worst_prior = 0.0
    ulp4 = 4 * 2.0 ** -52
    for k in range(steps):
        before = h.rollout_state()
        h.rollout_step(1)
        st, lc = h.rollout_state(), h.rollout_localiser()
        on = before["alive"] == 1
        for i in np.flatnonzero(on):
            pose = before["pose"][i]
            cnt["steps"][i] += 1
            if not prev["primed"][i]:
                assert _same_bits(lc["fix"][i], pose) and _same_bits(lc["prior"][i], pose)
                assert lc["cand"][i] == lc["score"][i] == lc["hits"][i] == -1
            else:
                cmd = q_prev[i, c[i]] if delayed else u_prev[i]
                want_prior = np.array(nominal(tuple(float(v) for v in prev["fix"][i]), 0.0, float(cmd[0]), float(cmd[1]), 0.0, 0.0, 0.0, L_CAR, TS)[0])
                dpr = float(np.max(np.abs(want_prior - lc["prior"][i])))
                worst_prior = max(worst_prior, dpr)
                assert dpr <= 1e-14 + ulp4 * TS * abs(cmd[0]) * (1.0 + 1.0 / L_CAR), (k, i, dpr)
                if not L.scheduled(k):
                    assert _same_bits(lc["fix"][i], lc["prior"][i]) and lc["cand"][i] == lc["score"][i] == lc["hits"][i] == -1
                else:
                    m = _twin_match(twin, L, grid, origin, res, lc["prior"][i], lc["ranges"][i], field=field)
                    assert m["hits"][0] == lc["hits"][i], (k, i)
                    if m["min_edge"][0] < BAND:
                        skipped += 1
                    else:
                        compared += 1
                        assert m["cand"][0] == lc["cand"][i] and m["score"][0] == lc["score"][i] and _same_bits(m["fix"][0], lc["fix"][i]), (k, i)
                    if lc["cand"][i] < 0:
                        cnt["lost"][i] += 1
                        assert _same_bits(lc["fix"][i], lc["prior"][i])
                    else:
                        cnt["matched"][i] += 1
                        a, cc, t = L.candidate(lc["cand"][i])
                        cnt["edge"][i] += int(abs(a) == L.W or abs(cc) == L.W or abs(t) == L.T)
            e2 = float((lc["fix"][i, 0] - pose[0]) ** 2 + (lc["fix"][i, 1] - pose[1]) ** 2)
            mine["err2_sum"][i] += e2
            mine["err2_max"][i] = max(mine["err2_max"][i], e2)
            mine["head2_sum"][i] += wrap(float(lc["fix"][i, 2]), float(pose[2])) ** 2
            mine["prior2_sum"][i] += float((lc["prior"][i, 0] - pose[0]) ** 2 + (lc["prior"][i, 1] - pose[1]) ** 2)
        for k_ in COUNTS:
            assert np.array_equal(lc[k_], cnt[k_]), (k, k_, lc[k_], cnt[k_])
        for k_ in STATS:
            assert np.allclose(lc[k_], mine[k_], rtol=1e-12, atol=0.0), (k, k_)
        off = ~on      # a car that is not running keeps what it had
        for k_ in ("fix", "prior") + STATS:
            assert _same_bits(lc[k_][off], prev[k_][off]), (k, k_)
        for k_ in ("cand", "score", "hits") + COUNTS:
            assert np.array_equal(lc[k_][off], prev[k_][off]), (k, k_)
        prev = dict(lc, primed=np.where(on, 1, prev["primed"]))
        u_prev = st["u"]
        if delayed:
            q_prev = h.rollout_delay()["queue"]
    h.close()
    print("K3l against the twin, %s: %d matches compared, %d in the band, prior within %.2e; matched %d, lost %d, edge %d" %
          (case, compared, skipped, worst_prior, cnt["matched"].sum(), cnt["lost"].sum(), cnt["edge"].sum()))
    assert compared > 4 * B and 100 * skipped <= compared + skipped
    if case != "two_routes":
        assert st["alive"][0] != 1 and cnt["steps"][0] < steps      # the car that finished its lap


@pytest.mark.gpu
def test_the_world_is_scanned_not_the_base_map():
    """a static disc and a mover in front of every car: the localiser's ranges are mpmpc_lidar_scan's of the true pose in the
    car's world of that step, bit for bit, and differ from the base map's"""
    N, B = 10, 16
    g1, grid, origin, res = _sim_map()
    h, cum, s0, poses = _step_setup("world", B, N)
    L = Localiser(_lidar(rng=0.8), 6, 1, 3, 1, 0.01, min_hits=5)
    h.rollout_init(TS, cum, s0, poses)
    _set(h, L, B)
    h.rollout_step(1)
    before = h.rollout_state()
    h.rollout_step(1)
    lc, discs = h.rollout_localiser(), h.rollout_obstacles()      # (the movers' discs of step 1: K0m ran in front of K0l)
    h.close()
    want = mpmpc.lidar_scan(grid, origin, res, before["pose"], L.angles, L.range, discs)
    bare = mpmpc.lidar_scan(grid, origin, res, before["pose"], L.angles, L.range)
    on = before["alive"] == 1
    assert on.sum() > B // 2 and _same_bits(lc["ranges"][on], want[on])
    assert np.any(want[on] != bare[on])


@pytest.mark.gpu
def test_one_call_equals_many_and_a_resumed_run():
    """a mismatched plant, per-car delays, range noise and a period of 2; the resumed run takes fix0 and step0 = -at, the plant's
    act0 and the saved register (which holds the command of the last step)"""
    N, B, steps, at = 10, 32, 20, 8
    w, s0, poses = _starts(B, 44, last=160)
    plant = Plant(seed=4242, car0=5, **TD.NOISY)
    L = Localiser(_lidar(rng=0.8), 6, 1, 3, 1, 0.01, min_hits=5, sigma_r=0.003, period=2, seed=17, car0=3)
    d = (np.arange(B) % 4).astype(np.int32)
    h = _handle(N, B)
    h.rollout_warm_start(False)
    h.rollout_set_plant(plant.params(B), plant.seed, plant.car0)
    cum = _cum()

    def start():
        h.rollout_init(TS, cum, s0, poses)
        h.rollout_set_delay(d, d, _in_flight(B))
    start()
    _set(h, L, B)
    h.rollout_step(steps)
    want, want_lc = h.rollout_state(), h.rollout_localiser()
    start()      # (rollout_init un-primes the cars and zeroes the statistics; the setting and the field stay)
    for t in range(steps):
        if t == at:
            saved, saved_pl, saved_dl, saved_lc = h.rollout_state(), h.rollout_plant(), h.rollout_delay(), h.rollout_localiser()
        h.rollout_step(1)
    got, got_lc = h.rollout_state(), h.rollout_localiser()
    _equal_states(got, want)
    for k in mpmpc.Handle.LOCALISER_FIELDS:
        assert np.array_equal(got_lc[k], want_lc[k]) if got_lc[k].dtype.kind == "i" else _same_bits(got_lc[k], want_lc[k]), k
    # resumed from the save
    h.rollout_init(TS, cum, saved["s"], saved["pose"], saved["cc"])
    h.rollout_set_counters(saved["counter"])
    h.rollout_set_plant(plant.params(B), plant.seed, plant.car0, step0=-at, act0=saved_pl["act"])
    h.rollout_set_delay(d, d, saved_dl["queue"])
    _set(h, L, B, step0=-at, fix0=saved_lc["fix"])
    h.rollout_step(steps - at)
    res, res_lc = h.rollout_state(), h.rollout_localiser()
    h.close()
    on = saved["alive"] == 1      # (a resumed run starts every car alive: the cars that were running at the save are compared)
    assert on.sum() > B // 4 and (want["alive"] == 1)[on].sum() > B // 4
    _equal_states({k: res[k][on] for k in TD.KEYS}, {k: want[k][on] for k in TD.KEYS})
    for k in ("fix", "prior", "ranges"):
        assert _same_bits(res_lc[k][on], want_lc[k][on]), k
    still = on & (want["alive"] == 1)      # the statistics start over with the resumed run
    assert np.all(res_lc["steps"][still] == steps - at) and np.all(want_lc["steps"][still] == steps)
    assert want_lc["matched"].sum() > 0 and not _same_bits(want_lc["fix"], want["pose"])


@pytest.mark.gpu
def test_the_schedule():
    """period = 3, step0 = -1: the cars scan on the steps 2, 5, 8, ... (step 0 primes); elsewhere the fix is the prior"""
    N, B, steps = 10, 16, 12
    w, s0, poses = _starts(B, 45, last=150)
    L = Localiser(_lidar(rng=0.8), 6, 1, 3, 1, 0.01, min_hits=5, period=3, step0=-1)
    h = _handle(N, B)
    h.rollout_set_plant(Plant(wheelbase_scale=1.05, speed_gain=0.97).params(B))
    h.rollout_init(TS, _cum(), s0, poses)
    _set(h, L, B)
    scans = 0
    for k in range(steps):
        h.rollout_step(1)
        lc = h.rollout_localiser()
        if k > 0 and L.scheduled(k):
            scans += 1
            assert np.all(lc["hits"] >= 0) and np.all(lc["matched"] + lc["lost"] == scans)
        else:
            assert np.all(lc["hits"] == -1) and np.all(lc["cand"] == -1) and _same_bits(lc["fix"], lc["prior"])
            assert np.all(lc["matched"] + lc["lost"] == scans)
    h.close()
    assert scans == 4 and np.all(lc["steps"] == steps) and lc["matched"].sum() > 2 * B


HELPS = dict(N=10, B=64, steps=30, seed=46)


@pytest.mark.gpu
def test_the_localiser_helps():
    """64 cars, 30 steps, a plant with wheelbase and gain mismatch.  The fixes are closer to the truth than dead reckoning
    (err2_sum < prior2_sum, summed over the fleet), and with an Estimator on top the controller's summed ey_sq (the plant's
    statistics) is no worse than with W = T = 0, which is dead reckoning alone.  No ratio is fixed; the figures are printed and
    recorded in profiles/localiser/README.md.  The cars start on the stretches of Sim_Track whose headings lie in (-3.0, -0.05)
    (_sound_waypoints: where the reference's lidar reports the map; started anywhere on the lap the matcher follows a partly
    mirrored scan and err2_sum is 22.6 against a prior2_sum of 21.4 m^2).  Measured on an MI355X: matching err2_sum 0.2820 against
    prior2_sum 0.3442 m^2 (dead reckoning alone: 4.6265), ey_sq with the Estimator on top 0.4767 m^2 matching against 2.6519 m^2
    dead reckoning (without the Estimator 0.2763 against 2.6519)."""
    N, B, steps = HELPS["N"], HELPS["B"], HELPS["steps"]
    g1, cum = TD._sim()[0], _cum()
    w = np.random.default_rng(HELPS["seed"]).choice(_sound_waypoints(ahead=14), B)      # (30 steps are some 12 waypoints)
    s0, poses = cum[w], np.stack([g1["x"][w], g1["y"][w], g1["psi"][w]], 1)
    plant = Plant(wheelbase_scale=1.08, speed_gain=0.95)
    est = Estimator(1e-6, 1e-6, 1e-5, 1e-4)
    out = {}
    for name, W, T in (("matching", 3, 2), ("dead reckoning", 0, 0)):
        L = Localiser(_lidar(rng=1.0), 6, 1, W, T, 0.01 if T else 0.0, min_hits=5)
        for e in (None, est):
            h = _handle(N, B)
            h.rollout_set_plant(plant.params(B))
            h.rollout_init(TS, _cum(), s0, poses)
            if e is not None:
                h.rollout_set_estimator(e.params(B), e.seed, e.car0, e.step0)
            _set(h, L, B)
            h.rollout_step(steps)
            out[name, e is not None] = (h.rollout_state(), h.rollout_plant(), h.rollout_localiser())
            h.close()
    for key, (st, pl, lc) in sorted(out.items()):
        print("%s, estimator %s: err2_sum %.4e, prior2_sum %.4e, ey_sq %.4e m^2; alive %d, matched %d, lost %d, edge %d" %
              (key[0], key[1], lc["err2_sum"].sum(), lc["prior2_sum"].sum(), pl["ey_sq"].sum(), (st["alive"] == 1).sum(), lc["matched"].sum(),
               lc["lost"].sum(), lc["edge"].sum()))
    lc = out["matching", False][2]
    assert lc["matched"].sum() > B * steps // 2 and lc["err2_sum"].sum() < lc["prior2_sum"].sum()
    dead = out["dead reckoning", False][2]
    assert _same_bits(dead["err2_sum"], dead["prior2_sum"]) and np.all(dead["edge"] == 0)      # one candidate: the fix is the prior
    assert out["matching", True][1]["ey_sq"].sum() <= out["dead reckoning", True][1]["ey_sq"].sum()


@pytest.mark.gpu
def test_state_and_argument_errors():
    N, B = 10, 8
    g1, grid, origin, res = _sim_map()
    w, s0, poses = _starts(B, 47, last=160)
    L = Localiser(_lidar(rng=0.8), 6, 1, 3, 1, 0.01, min_hits=5, period=2)
    cum = _cum()
    # no map
    h = TD._handle(N, B)
    with pytest.raises(mpmpc.MpmpcError) as err:
        _set(h, L, B)
    assert _code(err) == E_STATE and "mpmpc_set_map" in str(err.value)
    h.close()
    h = _handle(N, B)
    h.rollout_init(TS, cum, s0, poses)
    with pytest.raises(mpmpc.MpmpcError) as err:
        h.rollout_localiser()      # no localiser
    assert _code(err) == E_STATE
    _set(h, L, B)
    with pytest.raises(mpmpc.MpmpcError) as err:
        h.rollout_localiser()      # no step under it yet
    assert _code(err) == E_STATE
    h.rollout_step(3)
    h.rollout_step(3)
    want, want_lc = h.rollout_state(), h.rollout_localiser()
    # a refused call leaves the running setting's next step unchanged
    h.rollout_init(TS, cum, s0, poses)
    h.rollout_step(3)
    for kw in (dict(D=0), dict(D=16), dict(m=0), dict(W=17), dict(T=9), dict(step_psi=np.nan), dict(step_psi=0.0), dict(min_hits=0),
               dict(sigma_r=-1.0), dict(sigma_r=np.inf), dict(period=0), dict(range_m=0.0), dict(range_m=20.0),
               dict(angles=np.array([0.1, 0.0])), dict(angles=np.linspace(-1, 1, 1639), T=2), dict(fix0=np.full((B, 3), np.nan))):
        with pytest.raises(mpmpc.MpmpcError) as err:
            _set(h, L, B, **kw)
        assert _code(err) == E_ARG, kw
    with pytest.raises(mpmpc.MpmpcError) as err:
        _set(h, L, B + 1)      # more than max_batch
    assert _code(err) == E_ARG
    h.rollout_step(3)
    got, got_lc = h.rollout_state(), h.rollout_localiser()
    _equal_states(got, want)
    for k in mpmpc.Handle.LOCALISER_FIELDS:
        assert np.array_equal(got_lc[k], want_lc[k], equal_nan=True), k
    # an assumed delay of 8: refused with both settings named, and the step runs once either is changed
    h.rollout_set_delay(np.full(B, 8, np.int32))
    with pytest.raises(mpmpc.MpmpcError) as err:
        h.rollout_step(1)
    assert _code(err) == E_STATE and "mpmpc_rollout_set_localiser" in str(err.value) and "mpmpc_rollout_set_delay" in str(err.value)
    h.rollout_set_delay(np.full(B, 8, np.int32), np.full(B, 7, np.int32))
    h.rollout_step(1)
    h.rollout_set_delay(None)
    h.rollout_step(1)
    # a map changed since the setting
    h.set_map(grid, origin, res)
    h.build_corridor(N, 2 * T.safety_margin("sim"), T.safety_margin("sim"), want_tables=False)
    with pytest.raises(mpmpc.MpmpcError) as err:
        h.rollout_step(1)
    assert _code(err) == E_STATE and "changed since mpmpc_rollout_set_localiser" in str(err.value)
    _set(h, L, B)
    h.rollout_step(1)
    # a step of another B
    h.rollout_init(TS, cum, s0[:5], poses[:5])
    with pytest.raises(mpmpc.MpmpcError) as err:
        h.rollout_step(1)
    assert _code(err) == E_STATE and "another number of cars" in str(err.value)
    h.rollout_set_localiser(0)
    h.rollout_step(1)      # without a localiser: any B the rollout holds
    with pytest.raises(mpmpc.MpmpcError) as err:
        h.rollout_localiser()
    assert _code(err) == E_STATE
    h.close()
    # the handle-free entry points
    for kw, word in ((dict(D=0), "D must be"), (dict(W=17), "W must be"), (dict(T=1, step_psi=0.0), "step_psi"), (dict(min_hits=0), "min_hits")):
        a = dict(D=5, m=1, W=2, T=0, step_psi=0.0, min_hits=1)
        a.update(kw)
        with pytest.raises(mpmpc.MpmpcError, match=word):
            mpmpc.scan_match(grid, origin, res, np.zeros((2, 3)), np.zeros((2, 5)), np.linspace(-1, 1, 5), 0.5, **a)


@pytest.mark.gpu
def test_batchmpc_rollout_takes_a_localiser():
    """BatchMPC.rollout(..., localiser=...) returns "localiser"; with plant, delay, estimator, perception and obstacles their
    outputs stay in place; a following rollout without it is bit-equal to a controller that never had one"""
    from MPC import BatchMPC
    from lidar_model import LidarModel
    from map import Obstacle
    from perception import Perception
    from scipy import sparse
    m, rp, car = T.build_world(obstacles=False)
    Q, R, QN = sparse.diags([1.0, 0.0, 0.0]), sparse.diags([0.5, 0.0]), sparse.diags([1.0, 0.0, 0.0])
    ic = {'umin': np.array([0.0, -np.tan(0.66) / car.length]), 'umax': np.array([1.0, np.tan(0.66) / car.length])}
    sc = {'xmin': np.array([-np.inf] * 3), 'xmax': np.array([np.inf] * 3)}
    B, N, steps = 8, 10, 12
    w, s0, poses = _starts(B, 48, last=160)
    lidar = LidarModel(270, 0.8, 3.0)
    L = Localiser(lidar, 6, 1, 3, 1, 0.01, min_hits=5, sigma_r=0.002, seed=4)

    def make():
        return BatchMPC(car, N, Q, R, QN, sc, ic, 4.0, max_batch=B, corridor="device")
    fresh_bm = make()
    plain = fresh_bm.rollout(s0, poses, steps)
    fresh_bm.close()
    assert "localiser" not in plain
    bm = make()
    out = bm.rollout(s0, poses, steps, localiser=L)
    lc = out["localiser"]
    assert set(lc) == set(mpmpc.Handle.LOCALISER_FIELDS) and lc["fix"].shape == (B, 3) and lc["ranges"].shape == (B, lidar.n_measurements)
    on = out["alive"] == 1
    assert on.sum() >= B // 2 and np.all(lc["steps"][on] == steps) and np.all((lc["matched"] + lc["lost"])[on] == steps - 1)
    plant = Plant(wheelbase_scale=1.05, speed_gain=0.97)
    est = Estimator(1e-6, 1e-6, 1e-5, 1e-4)
    obstacles = [[Obstacle(float(rp.waypoints[(int(w[b]) + 15) % 200].x), float(rp.waypoints[(int(w[b]) + 15) % 200].y), 0.03)] for b in range(B)]
    out = bm.rollout(s0, poses, steps, localiser=L, plant=plant, delay=Delay(2, queue0=_in_flight(B)), estimator=est,
                     perception=Perception(lidar), obstacles=obstacles)
    assert set(out["localiser"]) == set(mpmpc.Handle.LOCALISER_FIELDS) and set(out["plant"]) == set(mpmpc.Handle.PLANT_FIELDS)
    assert set(out["delay"]) == set(mpmpc.Handle.DELAY_FIELDS) and set(out["estimator"]) == set(mpmpc.Handle.ESTIMATOR_FIELDS)
    assert out["perception"] is not None and out["localiser"]["matched"].sum() > 0
    assert bm.rollout(s0, poses, 0, localiser=L)["localiser"] is None
    again = bm.rollout(s0, poses, steps)      # off again
    _equal_states(again, plain)
    with pytest.raises(mpmpc.MpmpcError):
        bm.handle.rollout_localiser()
    bm.close()
