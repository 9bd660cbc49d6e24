"""Lookahead for traffic in the device rollout (K3t, K0ht, mpmpc_rollout_set_lookahead_traffic): every column of a car's horizon
is built against the cars of its traffic slots where their own plans of the step before put them at the step the column is
reached (csrc/traffic_lookahead_core.hpp).

CPU: the host twin (tests/emul_traffic_lookahead, the same traffic_lookahead_core.hpp) against the numpy restatement of the law
in lookahead.py - plan tracks, occupants, horizon discs, bit for bit, on both tracks and on a route view, over synthetic plans
that hold every branch of the law; "it matters" by construction; the budget, the exports.
GPU: fleets of test_lookahead's sizes with test_traffic's group recipe (groups of 2 .. 8, followers in the leader's lane).
After every step the tracks, the occupants, the horizon discs, the rows and the verdicts are the restated law's and the twin's -
plain, with walls, on two routes, under perception, with movers in the same fleet; off means off; zero times change nothing;
one call equals single steps; the first step after rollout_init / rollout_reroute plans on frozen discs; the refusals."""
import ctypes as C

import numpy as np
import pytest

import lookahead as LK
import mpmpc
import mpmpc_testlib as T
import scenarios
import test_lookahead as TL
import test_movers as TM
import test_traffic as TT
import twins

bp = C.POINTER(C.c_int8)
E_ARG, E_STATE = -1, -3
TS = TM.TS
MAX_LEAD = TL.MAX_LEAD
OFF = LK.TRACK_OFF
# N, B, steps (test_lookahead.SHAPES' sizes), seed, groups (test_traffic's recipe: followers GAPS waypoints apart in the
# leader's lane), singletons; the rest of the fleet has negative groups.  The seeds: the CPU has no emulation of a whole rollout
# step (the solve), so they were chosen on the first GPU run - the first ones tried, 91 and 92, left more than half of the B x steps
# car-steps to compare in every test below (the counts are printed).
SHAPES = dict(sim=(30, 64, 12, 91, (2, 3, 4, 5, 6, 7, 8), 6), real=(70, 32, 8, 92, (2, 3, 4, 8), 4))


_d, _i, _i32 = T._d, T._i, T._i32


@pytest.fixture(scope="module")
def twin():
    """The CPU twin of K3t, K0t<true>, K0ht and K0c<WALLS, true, true> (tests/emul_traffic_lookahead)."""
    return twins.traffic_lookahead()


@pytest.fixture(scope="module")
def car_twin():
    """The CPU twin of K0c (tests/emul_car): test_traffic's Fleet draws cars again whose plain step-0 row it finds blocked."""
    return twins.car()


# ------------------------------------------------------------------------------------------------ the two sides of a step
class Frame:
    """what traffic_core.hpp reads of a map (test_traffic._ranked's argument), from a test_lookahead.Ctx"""

    def __init__(self, c):
        self.ox, self.oy, self.res, self.W, self.H = c.origin[0], c.origin[1], c.res, int(c.grid.shape[1]), int(c.grid.shape[0])


def who_slots_law(pose, alive, group, rad, S, range_cells, f):
    """(who [B, S], slots [B, S, 3]) of the state a step finds: test_traffic's restated ranking, and who it ranks"""
    rk = TT._ranked(pose, alive, group, rad, f)
    who, out = np.full((len(rk), S), -1, np.int32), np.zeros((len(rk), S, 3), np.int32)
    for b, cand in enumerate(rk):
        if cand is None:
            continue
        if range_cells >= 0:
            cand = [k for k in cand if k[0] <= range_cells * range_cells]
        for t, k in enumerate(cand[:S]):
            who[b, t], out[b, t] = k[1], k[2:5]
    return who, out


def who_slots_twin(twin, c, pose, alive, group, rad, S, range_cells):
    pose = np.ascontiguousarray(pose, float)
    B = pose.shape[0]
    out, who = np.full((B, S, 3), -7, np.int32), np.full((B, S), -7, np.int32)
    assert twin.tlk_emu_slots(B, _d(pose), _i(_i32(alive)), _i(_i32(group)), _i(_i32(rad)), S, range_cells, c.grid.shape[0], c.grid.shape[1],
                              c.origin[0], c.origin[1], c.res, _i(out), _i(who)) == 0
    return who, out


def tracks_law(c, z, wp, status, alive, route=None):
    f, n, circ = c.views(route, np.asarray(wp).size)
    return LK.plan_tracks(z, wp, status, alive, c.a["x"], c.a["y"], c.a["psi"], c.origin, c.res, n_wp=n, circular=circ, first=f)


def tracks_twin(twin, c, z, wp, status, alive, route=None):
    z = np.ascontiguousarray(z, float)
    B, N = z.shape[0], (z.shape[1] - 3) // 5
    valid, cells, tm = np.full(B, -7, np.int32), np.full((B, N + 1, 2), -7, np.int32), np.full((B, N + 1), -7.0)
    twin.tlk_emu_tracks(B, N, _d(z), _i(_i32(wp)), _i(_i32(status)), _i(_i32(alive)), _i(c.headers(route)), c.n_wp, int(c.circular),
                        _d(c.a["x"]), _d(c.a["y"]), _d(c.a["psi"]), c.grid.shape[0], c.grid.shape[1], c.origin[0], c.origin[1], c.res,
                        _i(valid), _i(cells), _d(tm))
    return dict(valid=valid != 0, cells=cells, tm=tm)


def same_tracks(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("valid", "cells", "tm"))


def no_tracks(B, N):
    return dict(valid=np.zeros(B, bool), cells=np.zeros((B, N + 1, 2), np.int32), tm=np.zeros((B, N + 1)))


def discs_law(c, who, slots, lead, tracks):
    return LK.traffic_discs(who, slots, lead, tracks, TS, c.grid.shape[1], c.grid.shape[0])


def discs_twin(twin, c, who, slots, lead, tracks):
    B, S = who.shape
    N = lead.shape[1]
    out = np.full((B, S, N, 3), -7, np.int32)
    twin.tlk_emu_discs(B, S, N, TS, c.grid.shape[0], c.grid.shape[1], _i(_i32(who)), _i(_i32(slots)), _i(_i32(lead)),
                       _i(_i32(tracks["valid"])), _i(_i32(tracks["cells"])), _d(np.ascontiguousarray(tracks["tm"], float)), _i(out))
    return out


def rows_twin(twin, c, wp, N, disc_lists, S=0, tz=None, look=None, walls=None, route=None):
    """K0c's rows for one disc list per car (the lists K0c plans from at the step): S traffic slots at the end of every list and
    tz [B, S, N, 3] - the traffic rows; tz None - the plain-traffic rows.  look = (movers' rows per car, hz) or None."""
    B = len(disc_lists)
    off, flat = T.csr(disc_lists, 3, pad=False)
    woff, wflat = T.csr(walls, 4, pad=False)
    car = hz = None
    if look is not None:
        rows, hz = look
        car = np.zeros((B + 1, 2), np.int32)
        car[1:, 0] = np.cumsum([len(r) for r in rows])
        car[:B, 1] = [len(disc_lists[b]) - len(rows[b]) - S for b in range(B)]
        hz = _i32(hz)
    ub, lb, flag = np.zeros((B, N)), np.zeros((B, N)), np.zeros(B, np.int32)
    a = c.a
    rc = twin.tlk_emu_rows(c.grid.shape[0], c.grid.shape[1], c.grid.ctypes.data_as(bp), c.origin[0], c.origin[1], c.res, c.n_wp, _d(a["x"]),
                           _d(a["y"]), _d(a["psi"]), _d(a["ds_next"]), int(c.circular), _d(a["border_ub"]), _d(a["border_lb"]), N, 2 * c.sm,
                           c.sm, B, _i(_i32(wp)), _i(off), _i(flat), _i(woff), _i(wflat), _i(c.headers(route)), _i(car), _i(hz), S,
                           None if tz is None else _i(_i32(tz)), _d(ub), _d(lb), _i(flag))
    assert rc == 0
    return ub, lb, flag


# ------------------------------------------------------------------------------------------------------------ CPU
B_SYN, S_SYN = 12, 3


def _synthetic(c, N, rng, wp, route=None):
    """B_SYN plans that hold the law's branches, at local waypoints wp: -> z, status, alive, who, slots, lead, and what is where"""
    B = B_SYN
    z = np.zeros((B, 5 * N + 3))
    ey = rng.uniform(-0.06, 0.06, (B, N + 1))
    t = np.concatenate([np.zeros((B, 1)), np.cumsum(rng.uniform(0.6, 1.4, (B, N)) * TS, 1)], 1)
    t[0, 5] = t[0, 4] - 1e-9                       # a dip below tolerance: the running maximum holds tm[5] = tm[4]
    t[0, 9:12] = t[0, 8]                           # ... and a plateau
    t[1, 3], t[1, N] = np.nan, np.nan              # a NaN is never taken
    t[2, 1:] = np.cumsum(np.full(N, 1e-3))         # a plan that ends early: tau lies beyond tm[N] from the second column on
    t[3, 1:7] = np.linspace(0.02, 0.19, 6)
    t[3, 7] = 4.0 * TS                             # tau == tm[7] exactly for a column with lead 3
    t[3, 8:] = 4.0 * TS + np.cumsum(rng.uniform(0.6, 1.4, N - 7) * TS)
    assert t[3, 6] < 4.0 * TS
    t[4, 0] = 0.3                                  # tm[0] is 0.0 whatever t_0 holds
    t[9, 2] = np.inf                               # an infinite time is taken: the plan never gets past stage 1
    ey[4, 6] = np.nan                              # a stage whose cell fails the guard ...
    ey[4, 8] = 1e300                               # ... beyond 2^30 cells
    ey[4, 10] = -np.inf
    ey[5, 4:] = -50.0                              # a predicted square that leaves the grid (cells far below 0, within 2^30)
    z[:, 0:3 * (N + 1):3], z[:, 2:3 * (N + 1):3] = ey, t
    z[:, 1:3 * (N + 1):3] = rng.uniform(-0.1, 0.1, (B, N + 1))
    status = np.array([1, 2, -2, 1, 1, 1, 1, 3, 1, 1, -1, 1], np.int32)      # cars 7, 10: the solve was not usable
    alive = np.array([1, 1, 1, 1, 1, 1, -1, 1, 0, 1, 1, -3], np.int32)       # cars 6, 8, 11: not running after the step
    who = rng.integers(0, B, (B, S_SYN)).astype(np.int32)
    who[:, 0] = (np.arange(B) + 1) % B             # every car is somebody's first slot
    who[2, 1], who[5, 2] = -1, -1                  # empty slots
    trk = tracks_law(c, z, wp, status, alive, route)
    slots = np.zeros((B, S_SYN, 3), np.int32)
    for b in range(B):
        for s_ in range(S_SYN):
            if who[b, s_] >= 0:
                cell = trk["cells"][who[b, s_], 0]
                slots[b, s_] = (cell[0], cell[1], int(rng.integers(3, 9))) if cell[0] != OFF else (40, 40, 5)
    slots[0, 0, 2] = 0                             # r == 0: seen, occupies no cell
    slots[0, 1] = 0                                # an occupant whose disc of step k is absent (off the grid at the step itself)
    lead = np.sort(rng.integers(0, 12, (B, N)), 1).astype(np.int32)
    lead[:, 0] = 0                                 # L == 0: the step-k disc
    lead[2, 2:6] = 3                               # the viewer of car 3 (who[2, 0] == 3) has columns with lead 3
    lead[1] = np.arange(N) + 1                     # one viewer runs through every lead
    lead[6] = 1 << 20                              # saturated leads: everybody at their plan's end
    return z, status, alive, who, slots, lead, trk


def _check_synthetic(twin, c, N, wp, route=None):
    rng = np.random.default_rng(7)
    z, status, alive, who, slots, lead, trk = _synthetic(c, N, rng, wp, route)
    got = tracks_twin(twin, c, z, wp, status, alive, route)
    assert same_tracks(got, trk)
    assert got["cells"].dtype == np.int32 and trk["cells"].dtype == np.int32
    tm, cells = trk["tm"], trk["cells"]
    # the cases are what they claim to be
    assert trk["valid"].tolist() == [True] * 6 + [False] * 3 + [True, False, False]
    assert tm[0, 5] == tm[0, 4] and np.all(tm[0, 8:12] == tm[0, 8]) and np.all(tm[:, 1:] >= tm[:, :-1]) and np.all(tm[:, 0] == 0)
    assert tm[1, 3] == tm[1, 2] and tm[1, N] == tm[1, N - 1] and not np.isnan(tm).any()
    assert z[4, 2] == 0.3 and tm[4, 1] == z[4, 5] < 0.3              # (t_0 itself is never read)
    assert tm[9, 2] == np.inf and np.all(tm[9, 2:] == np.inf)
    assert cells[4, 6].tolist() == [OFF, 0] and cells[4, 8].tolist() == [OFF, 0] and cells[4, 10].tolist() == [OFF, 0]
    H, W = c.grid.shape
    c5 = cells[5, 4:].astype(np.int64)
    assert np.all((c5[:, 0] < 0) | (c5[:, 1] < 0) | (c5[:, 0] > W) | (c5[:, 1] > H)) and np.all(c5[:, 0] != OFF)      # off the grid, yet cells
    # K3t's scan of the times in chunks of 64 gives the recurrence's bits (and at a horizon of four chunks)
    for src in (z, _long_plan(rng)):
        Nn = (src.shape[1] - 3) // 5
        for b in range(src.shape[0]):
            scan = np.full(Nn + 1, -7.0)
            twin.tlk_emu_times_scan(Nn, _d(np.ascontiguousarray(src[b])), _d(scan))
            want = LK.plan_tracks(src[b:b + 1], [0], [1], [1], c.a["x"], c.a["y"], c.a["psi"], c.origin, c.res)["tm"][0]
            assert np.array_equal(scan, want), b
    # the horizon discs
    tz = discs_twin(twin, c, who, slots, lead, trk)
    assert np.array_equal(tz, discs_law(c, who, slots, lead, trk)) and tz.dtype == np.int32
    frozen = np.repeat(slots[:, :, None, :], N, 2)
    still = np.broadcast_to((lead == 0)[:, None, :], tz.shape[:3])
    assert still[:, :, 0].sum() >= 10 * S_SYN and np.array_equal(tz[still], frozen[still])       # L == 0
    assert np.array_equal(tz[2, 1], frozen[2, 1]) and not tz[2, 1].any()                 # an empty slot
    for b in range(B_SYN):
        for s_ in range(S_SYN):
            if who[b, s_] >= 0 and not trk["valid"][who[b, s_]]:
                assert np.array_equal(tz[b, s_], frozen[b, s_])                          # an invalid neighbour: frozen
    assert who[2, 0] == 3 and np.all(tz[2, 0, 2:6, :2] == cells[3, 7])                   # tau == tm[7]: stage 7, not 6
    assert who[1, 0] == 2 and np.all(tz[1, 0, 1:, :2] == cells[2, N])                    # beyond tm[N]: held at the plan's end
    assert who[3, 0] == 4
    gone = [col for col in range(N) if cells[4, np.sum(tm[4] <= (lead[3, col] + 1) * TS) - 1, 0] == OFF and lead[3, col] > 0]
    assert gone and not tz[3, 0, gone].any()                                             # a stage without a cell: absent
    assert who[4, 0] == 5
    left = lead[4] >= 4
    assert left.any() and not tz[4, 0, left].any() and tz[4, 0, 1:][lead[4, 1:] > 0].shape[0] > 0      # the square leaves the grid
    assert who[8, 0] == 9 and np.all(tz[8, 0][lead[8] > 0][:, :2] == cells[9, 1])       # tm = inf from stage 2 on
    assert np.all(tz[0, 0, :, 2] == 0) and np.any(tz[0, 0, :, :2] != slots[0, 0, :2])    # r == 0 moves along (K0c's gate drops it)
    for s_ in range(S_SYN):                                                              # saturated leads: the plan's last finite stage
        n = who[6, s_]
        if n >= 0 and trk["valid"][n] and n not in (4, 5) and slots[6, s_, 2] > 0:
            last = np.sum(tm[n] <= ((1 << 20) + 1) * TS) - 1
            assert np.all(tz[6, s_, :, :2] == cells[n, last]), s_
    return trk, tz


def _long_plan(rng, N=200):
    """one plan of N = 200 stages: four chunks of K3t's scan, maxima that cross the chunk borders, NaNs on them"""
    z = np.zeros((3, 5 * N + 3))
    t = np.cumsum(rng.uniform(-0.5, 1.0, (3, N + 1)) * TS, 1)
    t[0, 63], t[0, 64], t[0, 128] = 9.0, np.nan, np.nan
    t[1, 60:70] = -1.0
    t[2, :] = -np.abs(t[2])                          # never above tm[0] = 0
    z[:, 2:3 * (N + 1):3] = t
    return z


@pytest.mark.parametrize("track", ["sim", "real"])
def test_twin_equals_the_restated_law(track, twin):
    c = TL.ctx(track)
    N = SHAPES[track][0]
    wp = np.arange(B_SYN) * 13 % (c.n_wp - N - 2)
    # a circular path wraps within the horizon; an open one clamps to its last waypoint
    wp[:3] = [c.n_wp - 3, c.n_wp - 1, 0] if c.circular else [c.n_wp - N + 5, c.n_wp - 2, c.n_wp - N // 2]
    trk, _ = _check_synthetic(twin, c, N, wp)
    rows = LK.column_rows(wp, N + 1, c.n_wp, c.circular, 0)
    if c.circular:
        assert rows[0, 3] == 0 and rows[0, 2] == c.n_wp - 1
    else:
        assert np.all(rows[1, 1:] == c.n_wp - 1) and np.all(trk["cells"][1, 1:, 0] != OFF)


def test_route_view_of_the_law(twin):
    """route fleets: the stages wrap / clamp inside the car's route, rows by global row"""
    c, first, circ = TL._route_ctx()
    N = 30
    n = np.diff(first)
    route = (np.arange(B_SYN) % 2).astype(np.int32)
    wp = np.array([int(w) % (n[r] - N - 2) for r, w in zip(route, np.arange(B_SYN) * 17)], np.int32)
    wp[0], wp[1], wp[2], wp[3] = n[0] - 3, n[1] - 5, n[0] - 1, n[1] - N + 2
    trk, _ = _check_synthetic(twin, c, N, wp, route)
    # stage 3 of car 0 is the lap's first row again; car 1's stages from 4 on all lie at its open route's last row
    z0 = np.zeros((1, 5 * N + 3))
    at = lambda row: tracks_law(c, z0, [row], [1], [1], np.array([0], np.int32))["cells"][0, 0]
    on1 = lambda row: tracks_law(c, z0, [row], [1], [1], np.array([1], np.int32))["cells"][0, 0]
    zz = np.zeros((B_SYN, 5 * N + 3))
    flat = tracks_law(c, zz, wp, np.ones(B_SYN), np.ones(B_SYN), route)["cells"]
    assert np.array_equal(flat[0, 3], at(0)) and np.array_equal(flat[0, 2], at(n[0] - 1))
    assert np.all(flat[1, 4:] == on1(n[1] - 1)) and not np.array_equal(flat[1, 3], flat[1, 4])


@pytest.mark.parametrize("track", ["sim", "real"])
def test_occupants_twin_equals_the_restated_law(track, twin):
    """tr_slots_car's optional output: who sits in the slots test_traffic's law case fills"""
    case = TT._law_case(track)
    c = TL.ctx(track)
    f = Frame(c)
    for S, rng_cells in TT.SETTINGS[track][:3]:
        who, out = who_slots_twin(twin, c, case["pose"], case["alive"], case["group"], case["rad"], S, rng_cells)
        want_who, want = who_slots_law(case["pose"], case["alive"], case["group"], case["rad"], S, rng_cells, f)
        assert np.array_equal(out, want) and np.array_equal(who, want_who), (S, rng_cells)
        assert (who >= 0).sum() > 100 and (who < 0).sum() > 100 and np.array_equal(who < 0, ~np.any(out != 0, 2) & (who < 0))
        seen = who[who >= 0]
        assert np.all(case["alive"][seen] == 1) and np.all(case["group"][seen] >= 0)


def test_it_matters_by_construction(twin):
    """One viewer at waypoint w0 of Sim_Track, one neighbour in its only slot whose disc of step k lies off the road, in a corner
    of the map; the neighbour's track puts stages 5 .. 8 on the centre line at the waypoint of the viewer's column 6 and every
    other stage back in the corner; tm[j] = j * Ts and lead[c] = c, so column c reads stage c + 1: the disc moves onto the road
    for columns 4 .. 7 and nowhere else.  The traffic rows differ from the plain-traffic rows at column 6, and only at columns
    whose disc moved."""
    c = TL.ctx("sim")
    N, w0, r = 30, 40, 6
    corner = (20, 20)
    z0 = np.zeros((1, 5 * N + 3))
    on_road = tracks_law(c, z0, [w0 + 1 + 6], [1], [1])["cells"][0, 0]
    cells = np.tile(np.array(corner, np.int32), (2, N + 1, 1))
    cells[1, 5:9] = on_road
    trk = dict(valid=np.array([True, True]), cells=cells, tm=np.tile(np.arange(N + 1) * TS, (2, 1)))
    who = np.array([[1], [-1]], np.int32)
    slots = np.array([[corner + (r,)], [(0, 0, 0)]], np.int32)
    lead = np.tile(np.arange(N, dtype=np.int32), (2, 1))
    tz = discs_twin(twin, c, who, slots, lead, trk)
    assert np.array_equal(tz, discs_law(c, who, slots, lead, trk))
    moved = np.any(tz[0, 0] != slots[0, 0], 1)
    assert np.flatnonzero(moved).tolist() == [4, 5, 6, 7] and np.all(tz[0, 0, 4:8] == (on_road[0], on_road[1], r))
    lists = [slots[0], slots[1]]
    wp = np.array([w0, w0 + 60], np.int32)
    plain = rows_twin(twin, c, wp, N, lists, S=1)
    ahead = rows_twin(twin, c, wp, N, lists, S=1, tz=tz)
    base = rows_twin(twin, c, wp, N, [np.zeros((1, 3), np.int32)] * 2, S=1)
    assert not plain[2].any() and not ahead[2].any()
    assert np.array_equal(plain[0], base[0]) and np.array_equal(plain[1], base[1])       # in the corner it touches nothing
    differ = (plain[0][0] != ahead[0][0]) | (plain[1][0] != ahead[1][0])
    print("columns whose rows differ:", np.flatnonzero(differ).tolist())
    assert differ[6] and not differ[~moved].any()
    assert np.array_equal(plain[0][1], ahead[0][1]) and np.array_equal(plain[1][1], ahead[1][1])       # the car that sees nobody
    # the gate: an entry with r == 0 in the list K0c plans from keeps the staged entry in every column
    unseen = rows_twin(twin, c, wp, N, [np.zeros((1, 3), np.int32)] * 2, S=1, tz=tz)
    assert np.array_equal(unseen[0], base[0]) and np.array_equal(unseen[1], base[1])


def test_setting_validation_and_exports_without_device(twin, built_library):
    lib = mpmpc.load_library(built_library)
    one = np.zeros(4, np.int32)
    assert lib.mpmpc_rollout_set_lookahead_traffic(None, 1) == E_ARG
    assert lib.mpmpc_rollout_tracks(None, 1, _i(one), None, None) == E_ARG
    assert lib.mpmpc_rollout_lookahead_traffic(None, 1, _i(one), None) == E_ARG
    raw = C.CDLL(built_library)
    for name in ("mpmpc_rollout_set_lookahead_traffic", "mpmpc_rollout_tracks", "mpmpc_rollout_lookahead_traffic"):
        assert name in mpmpc.EXPORTS and hasattr(raw, name)
    for name in ("rollout_set_lookahead_traffic", "rollout_tracks", "rollout_lookahead_traffic"):
        assert hasattr(mpmpc.Handle, name)
    # the budget: B x S x N x 12 bytes against the lookahead's 256 MiB
    assert twin.tlk_emu_budget() == 256 << 20
    assert twin.tlk_emu_table_bytes(64, 4, 30) == 64 * 4 * 30 * 12
    assert twin.tlk_emu_table_bytes(11650, 64, 30) <= twin.tlk_emu_budget() < twin.tlk_emu_table_bytes(11651, 64, 30)
    assert twin.tlk_emu_table_bytes(1 << 20, 64, 255) == (1 << 20) * 64 * 255 * 12       # (64-bit)
    # the Python front end
    assert LK.Lookahead(5).traffic is False and LK.Lookahead(5, traffic=True).traffic is True
    assert LK.Lookahead(5, [0.1], True).max_lead == 5 and LK.TRACK_OFF == -2 ** 31


# ------------------------------------------------------------------------------------------------------------ GPU
_FLEETS = {}


def fleet(track, car_twin, extras=False):
    """test_traffic's Fleet at this file's shapes: groups of 2 .. 8 that follow each other, singletons, cars that see nobody"""
    key = (track, extras)
    if key not in _FLEETS:
        N, B, steps, seed, small, n_single = SHAPES[track]
        _FLEETS[key] = TT.Fleet(track, car_twin, extras=extras, shape=(N, B, steps, seed, (0, 0), small, n_single))
    return _FLEETS[key]


class Setup:
    """the per-car settings of a run and the traffic's parameters"""

    def __init__(self, group, rad, S, range_cells, static=None, rows=None, walls=None, route=None):
        self.group, self.rad, self.S, self.range_cells = _i32(group), _i32(rad), S, range_cells
        self.static, self.rows, self.walls, self.route = static, rows, walls, route

    def apply(self, h):
        if self.walls is not None:
            h.rollout_set_walls(self.walls)
        if self.static is not None:
            h.rollout_set_obstacles(self.static)
        if self.rows is not None:
            h.rollout_set_movers(self.rows)
        h.rollout_set_traffic(self.group, self.rad, self.S, self.range_cells)


def _check_steps(h, c, twin, su, N, B, steps, seg, max_lead, gate=None, prev=None):
    """after every step of a step-by-step run: who and the true slots against the law on the pre-step state, rollout_lookahead()
    and rollout_lookahead_traffic() against the restated laws (the tracks: those the step before left), rollout_corridor() and
    the verdicts against the twin's rows (cars the step planned for), and rollout_tracks() against plan_tracks of download().z.
    gate(k, true lists) -> the lists K0c planned from (perception), else the true ones.  -> car-steps compared, car-steps whose
    rows differ from the plain-traffic twin's, the tracks the last step left"""
    f = Frame(c)
    prev = no_tracks(B, N) if prev is None else prev
    compared = mattered = 0
    for k in range(steps):
        before = h.rollout_state()
        h.rollout_step(1)
        st = h.rollout_state()
        who_l, slots_l = who_slots_law(before["pose"], before["alive"], su.group, su.rad, su.S, su.range_cells, f)
        who, tz = h.rollout_lookahead_traffic()
        assert who.dtype == np.int32 and who.shape == (B, su.S) and np.array_equal(who, who_l), k
        true = h.rollout_obstacles()
        assert np.array_equal(np.array([d[len(d) - su.S:] for d in true]), slots_l), k
        lead, hz = h.rollout_lookahead()
        assert np.array_equal(lead, c.leads_law(st["wp_id"], N, seg, max_lead, su.route)), k
        look = None
        if su.rows is not None:
            assert np.array_equal(hz, c.discs_law(su.rows, k, 0, lead, su.route)), k
            look = (su.rows, hz)
        else:
            assert hz.shape[0] == 0
        want = discs_law(c, who_l, slots_l, lead, prev)
        assert tz.shape == (B, su.S, N, 3) and np.array_equal(tz, want), k
        assert np.array_equal(want, discs_twin(twin, c, who_l, slots_l, lead, prev)), k
        lists = true if gate is None else gate(k, true)
        ub, lb, flag = rows_twin(twin, c, st["wp_id"], N, lists, S=su.S, tz=tz, look=look, walls=su.walls, route=su.route)
        got_ub, got_lb = h.rollout_corridor()
        planned = (before["alive"] == 1) & np.isin(st["alive"], (1, -1, -3, -4))
        assert np.array_equal(got_ub[planned], ub[planned], equal_nan=True) and np.array_equal(got_lb[planned], lb[planned], equal_nan=True), k
        assert np.all(st["alive"][planned & (flag == 1)] == -3) and np.all(st["alive"][planned & (flag == 2)] == -4)
        assert not np.any(np.isin(st["alive"][planned & (flag == 0)], (-3, -4)))
        plain = rows_twin(twin, c, st["wp_id"], N, lists, S=su.S, look=look, walls=su.walls, route=su.route)
        mattered += int((planned & (np.any((plain[0] != ub) | (plain[1] != lb), 1) | (plain[2] != flag)) & ((flag == 0) | (plain[2] == 0))).sum())
        compared += int(planned.sum())
        # the tracks this step leaves
        got = h.rollout_tracks()
        z = h.download(B).z.reshape(B, -1)
        prev = tracks_law(c, z, st["wp_id"], st["status"], st["alive"], su.route)
        assert same_tracks(got, prev), (k, [key for key in prev if not np.array_equal(got[key], prev[key])])
        assert same_tracks(prev, tracks_twin(twin, c, z, st["wp_id"], st["status"], st["alive"], su.route)), k
    return compared, mattered, prev


def _open(track, N, B, su, seg, max_lead, on=True):
    h, _ = TT._handle(track, N, B)
    su.apply(h)
    h.rollout_set_lookahead(seg, max_lead)
    if on:
        h.rollout_set_lookahead_traffic(True)
    return h


@pytest.mark.gpu
@pytest.mark.parametrize("track,S,with_walls", [("sim", 4, False), ("sim", 1, False), ("real", 4, False), ("sim", 4, True)])
def test_every_step_equals_the_law_and_the_twin(track, S, with_walls, twin, car_twin):
    N, B, steps = SHAPES[track][:3]
    c, fl = TL.ctx(track), fleet(track, car_twin)
    walls = TL._walls_of(c, fl, np.random.default_rng(5)) if with_walls else None
    su = Setup(fl.group, fl.rad, S, fl.range_cells, walls=walls)
    h = _open(track, N, B, su, c.seg_default, MAX_LEAD)
    fl.init(h)
    compared, mattered, trk = _check_steps(h, c, twin, su, N, B, steps, c.seg_default, MAX_LEAD)
    st = h.rollout_state()
    h.close()
    print("%s S=%d walls=%s: %d car-steps compared, %d with rows the traffic lookahead changed; valid tracks %d; alive %s" %
          (track, S, with_walls, compared, mattered, int(trk["valid"].sum()), dict(zip(*np.unique(st["alive"], return_counts=True)))))
    assert compared * 2 >= B * steps and mattered >= 1


def _route_fleet(c, first, circ, N, B, rng):
    """the lap (route 0, circular) and the open second half of it (route 1: local waypoint i is the lap's 100 + i): groups of
    2 .. 6 whose cars follow each other 4 .. 8 waypoints apart ALTERNATING between the two routes, the rest alone on the lap"""
    route, wp, group, rad = np.zeros(B, np.int32), np.zeros(B, np.int64), np.full(B, -1), np.zeros(B, int)
    b = 0
    for q, n in enumerate((2, 3, 4, 5, 6)):
        lap = int(rng.integers(102, 112)) + 3 * q
        for k in range(n):
            route[b] = (k + q) % 2
            wp[b] = lap - 100 if route[b] else lap
            group[b], rad[b] = q, int(rng.integers(6, 11))
            lap += int(rng.integers(4, 9))
            b += 1
    wp[b:] = rng.integers(0, 95, B - b)
    group[b:] = np.where(np.arange(B - b) % 2 == 0, 50 + np.arange(B - b), -1)
    rad[b:] = 6
    g = first[route] + wp
    return route, wp.astype(np.int32), group, rad, c.cum[g], np.stack([c.a["x"][g], c.a["y"][g], c.a["psi"][g]], 1)


@pytest.mark.gpu
def test_routes_every_step_and_the_first_step_after_a_reroute(twin):
    N, B, steps = 30, 32, 10
    c, first, circ = TL._route_ctx()
    route, wp, group, rad, s, poses = _route_fleet(c, first, circ, N, B, np.random.default_rng(33))
    assert all(len(set(route[group == q])) == 2 for q in range(5))          # every group spans both routes
    su = Setup(group, rad, 4, -1, route=route)
    h = mpmpc.Handle(T.stock_config(N, max_batch=B, circular=False), mpmpc.default_settings())
    h.set_path(c.cat["kappa"], c.cat["v_ref"], c.cat["ds_next"])
    h.set_routes(first, circ)
    h.set_map(c.grid, c.origin, c.res)
    h.set_path_geometry(c.a["x"], c.a["y"], c.a["psi"], c.a["border_ub"], c.a["border_lb"])
    assert h.build_corridor(N, 2 * c.sm, c.sm, want_tables=False)[2] == 0
    h.set_car_routes(route)
    h.rollout_warm_start(False)
    su.apply(h)
    h.rollout_set_lookahead(c.seg_default, MAX_LEAD)
    h.rollout_set_lookahead_traffic(True)
    h.rollout_init(TS, c.cum, s, poses)
    compared, mattered, trk = _check_steps(h, c, twin, su, N, B, steps, c.seg_default, MAX_LEAD)
    st = h.rollout_state()
    print("routes: %d car-steps compared, %d changed by the traffic lookahead; alive %s" %
          (compared, mattered, dict(zip(*np.unique(st["alive"], return_counts=True)))))
    assert compared * 2 >= B * steps and mattered >= 1 and trk["valid"].sum() * 2 >= B
    # a reroute - here one that keeps every car on its route - makes every track invalid: one step on frozen discs, then tracks again
    assert not h.rollout_reroute(np.full(B, -1, np.int32)).any()
    with pytest.raises(mpmpc.MpmpcError):
        h.rollout_tracks()
    _check_steps(h, c, twin, su, N, B, 2, c.seg_default, MAX_LEAD)          # (its first step: against no tracks)
    # the routes change: the settings are void, like the per-car ones
    h.set_routes(first, circ[::-1].copy())
    with pytest.raises(mpmpc.MpmpcError):
        h.rollout_step(1)
    h.close()


def _run(h, fl, steps):
    fl.init(h)
    h.rollout_step(steps)
    return h.rollout_state(), h.rollout_corridor()


@pytest.mark.gpu
def test_off_means_off_and_zero_times_change_nothing(car_twin):
    """movers in the fleet, so that rollout_lookahead() has something to return with the flag off"""
    track = "sim"
    N, B, steps = SHAPES[track][:3]
    c, fl = TL.ctx(track), fleet(track, car_twin, extras=True)
    su = Setup(fl.group, fl.rad, 4, fl.range_cells, static=fl.static, rows=fl.rows)
    never = _open(track, N, B, su, c.seg_default, MAX_LEAD, on=False)       # a handle that never heard of the flag
    want = _run(never, fl, steps)
    want_look = never.rollout_lookahead()
    for getter in (never.rollout_tracks, never.rollout_lookahead_traffic):
        with pytest.raises(mpmpc.MpmpcError):
            getter()
    h = _open(track, N, B, su, c.seg_default, MAX_LEAD)
    on = _run(h, fl, steps)
    assert not np.array_equal(on[0]["s"], want[0]["s"])                      # on, the run differs ...
    h.rollout_set_lookahead_traffic(False)                                   # ... and off again it is the other handle's
    got = _run(h, fl, steps)
    TL._same_run(got, want)
    look = h.rollout_lookahead()
    assert np.array_equal(look[0], want_look[0]) and np.array_equal(look[1], want_look[1])
    for getter in (h.rollout_tracks, h.rollout_lookahead_traffic):
        with pytest.raises(mpmpc.MpmpcError):
            getter()
    # every lead zero: every entry is the step-k disc, and the run is the flag-off run with that table
    zeros = np.zeros(c.n_wp)
    never.rollout_set_lookahead(zeros, 9)
    want0 = _run(never, fl, steps)
    h.rollout_set_lookahead(zeros, 9)
    h.rollout_set_lookahead_traffic(True)
    fl.init(h)
    for k in range(steps):
        h.rollout_step(1)
        who, tz = h.rollout_lookahead_traffic()
        slots = np.array([d[-4:] for d in h.rollout_obstacles()])
        assert np.array_equal(tz, np.repeat(slots[:, :, None, :], N, 2)), k
    assert h.rollout_tracks()["valid"].any() and (who >= 0).any()
    TL._same_run((h.rollout_state(), h.rollout_corridor()), want0)
    # without movers and with the flag off, no step looks ahead - rollout_lookahead refuses as it always did
    h.rollout_set_movers(None)
    h.rollout_set_lookahead_traffic(False)
    fl.init(h)
    h.rollout_step(1)
    with pytest.raises(mpmpc.MpmpcError):
        h.rollout_lookahead()
    h.rollout_set_lookahead_traffic(True)                                    # ... and on, such a step does: leads, no mover discs
    h.rollout_step(1)
    lead, hz = h.rollout_lookahead()
    assert lead.shape == (B, N) and hz.shape[0] == 0 and not lead.any()
    never.close()
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("track", ["sim", "real"])
def test_one_call_equals_single_steps_and_init_resets(track, car_twin):
    N, B, steps = SHAPES[track][:3]
    c, fl = TL.ctx(track), fleet(track, car_twin)
    su = Setup(fl.group, fl.rad, 4, fl.range_cells)
    h = _open(track, N, B, su, c.seg_default, MAX_LEAD)
    one = _run(h, fl, steps)
    extra_one = (h.rollout_tracks(), h.rollout_lookahead_traffic(), h.rollout_lookahead())
    fl.init(h)                                                               # rollout_init: no track is a step's of this rollout
    with pytest.raises(mpmpc.MpmpcError):
        h.rollout_tracks()
    for k in range(steps):
        h.rollout_step(1)
        if k == 0:                                                           # the first step: frozen discs for every car
            who, tz = h.rollout_lookahead_traffic()
            slots = np.array([d[-4:] for d in h.rollout_obstacles()])
            assert (who >= 0).any() and h.rollout_lookahead()[0].max() > 5
            assert np.array_equal(tz, np.repeat(slots[:, :, None, :], N, 2))
    single = (h.rollout_state(), h.rollout_corridor())
    extra = (h.rollout_tracks(), h.rollout_lookahead_traffic(), h.rollout_lookahead())
    h.close()
    TL._same_run(one, single)
    assert same_tracks(extra_one[0], extra[0])
    for a, b in zip(extra_one[1] + extra_one[2], extra[1] + extra[2]):
        assert np.array_equal(a, b)
    moved = np.any(extra[1][1] != extra[1][1][:, :, :1], (2, 3))
    print("%s: slots whose disc moves within the horizon at the last step: %d of %d occupied" % (track, moved.sum(), (extra[1][0] >= 0).sum()))
    assert moved.any()
    TM._enough_alive(one[0])


@pytest.mark.gpu
def test_perception_gates_the_neighbours(twin, car_twin):
    """a car anticipates exactly the neighbours it sees at the step: the lists K0c planned from are the true ones masked by
    rollout_perception()'s disc_known (a traffic slot: while seen); an unseen neighbour is absent in every column"""
    track, S = "sim", 4
    N, B, steps = SHAPES[track][:3]
    c, fl = TL.ctx(track), fleet(track, car_twin)
    su = Setup(fl.group, fl.rad, S, fl.range_cells)
    h = _open(track, N, B, su, c.seg_default, MAX_LEAD)
    h.rollout_set_perception(np.linspace(-np.pi / 2, np.pi / 2, 181), 0.3, 2)
    fl.init(h)
    seen = dict(unseen=0, seen=0)

    def gate(k, true):
        known = h.rollout_perception()["disc_known"]
        out = []
        for b in range(B):
            bits = np.array([(int(known[b]) >> q) & 1 for q in range(S)], bool)
            present = true[b][:, 2] > 0
            seen["unseen"] += int((present & ~bits).sum())
            seen["seen"] += int((present & bits).sum())
            out.append(np.where(bits[:, None], true[b], 0).astype(np.int32))
        return out
    compared, mattered, _ = _check_steps(h, c, twin, su, N, B, steps, c.seg_default, MAX_LEAD, gate=gate)
    h.close()
    print("perception: %d car-steps compared, %d changed by the traffic lookahead, neighbours seen / unseen %s" % (compared, mattered, seen))
    assert compared * 2 >= B * steps and seen["unseen"] > 0 and seen["seen"] > 0 and mattered >= 1


@pytest.mark.gpu
def test_movers_and_traffic_anticipated_together(twin, car_twin):
    """2 static discs, 2 movers along the path and 4 traffic slots per car: one K0c launch reads K0h's and K0ht's tables"""
    track = "sim"
    N, B, steps = SHAPES[track][:3]
    c, fl = TL.ctx(track), fleet(track, car_twin, extras=True)
    su = Setup(fl.group, fl.rad, 4, fl.range_cells, static=fl.static, rows=fl.rows)
    h = _open(track, N, B, su, c.seg_default, MAX_LEAD)
    fl.init(h)
    compared, mattered, _ = _check_steps(h, c, twin, su, N, B, steps, c.seg_default, MAX_LEAD)
    st = h.rollout_state()
    h.close()
    print("movers + traffic: %d car-steps compared, %d with rows the traffic lookahead changed; alive %s" %
          (compared, mattered, dict(zip(*np.unique(st["alive"], return_counts=True)))))
    assert compared * 2 >= B * steps and mattered >= 1


@pytest.mark.gpu
def test_refusals(car_twin):
    track = "sim"
    N, B, steps = SHAPES[track][:3]
    c, fl = TL.ctx(track), fleet(track, car_twin)
    su = Setup(fl.group, fl.rad, 4, fl.range_cells)
    h = _open(track, N, B, su, c.seg_default, MAX_LEAD)
    for getter in (h.rollout_tracks, h.rollout_lookahead_traffic):
        with pytest.raises(mpmpc.MpmpcError):
            getter()                                                         # before any rollout
    fl.init(h)
    with pytest.raises(mpmpc.MpmpcError):
        h.rollout_lookahead_traffic()                                        # no step yet
    h.rollout_step(2)
    assert h.rollout_tracks()["cells"].shape == (B, N + 1, 2) and h.rollout_lookahead_traffic()[1].shape == (B, 4, N, 3)
    buf = np.zeros(B * (N + 1) * 2, np.int32)
    assert h.lib.mpmpc_rollout_tracks(h._h, B - 1, _i(buf), None, None) == E_STATE           # wrong B
    assert h.lib.mpmpc_rollout_lookahead_traffic(h._h, B + 1, _i(buf), None) == E_STATE
    assert h.lib.mpmpc_rollout_tracks(h._h, B, None, None, None) == E_ARG
    su.apply(h)                                                              # a per-car setting anew: the last step's tables are no longer its
    for getter in (h.rollout_tracks, h.rollout_lookahead_traffic):
        with pytest.raises(mpmpc.MpmpcError):
            getter()
    h.rollout_step(1)
    who, tz = h.rollout_lookahead_traffic()
    slots = np.array([d[-4:] for d in h.rollout_obstacles()])
    assert np.array_equal(tz, np.repeat(slots[:, :, None, :], N, 2))         # ... and that step planned on frozen discs
    h.rollout_set_lookahead(c.seg_default, 3)                                # the lookahead anew: the getters refuse the last step's ...
    for getter in (h.rollout_tracks, h.rollout_lookahead_traffic):
        with pytest.raises(mpmpc.MpmpcError):
            getter()
    h.rollout_step(1)                                                        # ... but the tracks stay: the next step reads them
    who, tz = h.rollout_lookahead_traffic()
    slots = np.array([d[-4:] for d in h.rollout_obstacles()])
    assert h.rollout_lookahead()[0].max() == 3 and np.any(tz != np.repeat(slots[:, :, None, :], N, 2))
    assert h.rollout_tracks()["valid"].any()
    tr = scenarios.sim_track()
    h.set_path(tr.kappa, tr.v_ref, tr.ds_next)                               # the path set anew: every setting is void
    assert h.lib.mpmpc_rollout_step(h._h, B, 1) == E_STATE
    h.close()
    # the budget: 11 651 cars x 64 slots x 30 columns x 12 bytes is the first fleet over 256 MiB - whichever setter comes last refuses
    big = 11651
    h, _ = TT._handle(track, N, big)
    grp, rad = np.arange(big) // 1024, np.zeros(big, np.int32)
    h.rollout_set_lookahead(c.seg_default, MAX_LEAD)
    h.rollout_set_lookahead_traffic(True)
    with pytest.raises(mpmpc.MpmpcError, match="256 MiB"):
        h.rollout_set_traffic(grp, rad, 64, -1)
    h.rollout_set_traffic(grp, rad, 63, -1)                                  # ... and the setting before stays possible
    h.rollout_set_lookahead_traffic(False)
    h.rollout_set_traffic(grp, rad, 64, -1)
    with pytest.raises(mpmpc.MpmpcError, match="256 MiB"):
        h.rollout_set_lookahead_traffic(True)
    h.rollout_set_lookahead(None)
    h.rollout_set_lookahead_traffic(True)
    with pytest.raises(mpmpc.MpmpcError, match="256 MiB"):
        h.rollout_set_lookahead(c.seg_default, MAX_LEAD)
    h.rollout_set_traffic(grp[:-1], rad[:-1], 64, -1)                        # one car fewer fits
    h.rollout_set_lookahead(c.seg_default, MAX_LEAD)
    h.close()


@pytest.mark.gpu
def test_batch_mpc_rollout_takes_lookahead_traffic():
    import traffic
    from MPC import BatchMPC
    from scipy import sparse
    m, rp, car = T.build_world()
    Q, R, QN = sparse.diags([1.0, 0.0, 0.0]), sparse.diags([0.5, 0.0]), sparse.diags([1.0, 0.0, 0.0])
    ic = {'umin': np.array([0.0, -np.tan(0.66) / car.length]), 'umax': np.array([1.0, np.tan(0.66) / car.length])}
    sc = {'xmin': np.array([-np.inf] * 3), 'xmax': np.array([np.inf] * 3)}
    B, N = 8, 30
    bm = BatchMPC(car, N, Q, R, QN, sc, ic, 4.0, max_batch=B, corridor="device")
    starts = np.array([0, 10, 20, 30, 60, 70, 120, 160])
    cum = np.cumsum(rp.segment_lengths)
    poses = np.array([[rp.waypoints[w].x, rp.waypoints[w].y, rp.waypoints[w].psi] for w in starts])
    tf = traffic.Traffic([0, 0, 0, 0, 1, 1, -1, 2], 0.04, 2, range=2.0)
    plain = bm.rollout(cum[starts], poses, 6, traffic=tf, lookahead=LK.Lookahead(25))
    with pytest.raises(mpmpc.MpmpcError):
        bm.handle.rollout_tracks()                                            # that rollout did not anticipate traffic
    got = bm.rollout(cum[starts], poses, 6, traffic=tf, lookahead=LK.Lookahead(25, traffic=True))
    who, tz = bm.handle.rollout_lookahead_traffic()
    trk = bm.handle.rollout_tracks()
    assert who.shape == (B, 2) and tz.shape == (B, 2, N, 3) and trk["valid"].any()
    assert set(who[0].tolist()) <= {1, 2, 3, -1} and set(who[4].tolist()) <= {5, -1} and (who >= 0).any()
    assert who[6].tolist() == [-1, -1] and who[7].tolist() == [-1, -1]           # sees nobody; alone in its group
    wps = rp.waypoints
    z = bm.handle.download(B).z.reshape(B, -1)
    want = LK.plan_tracks(z, got["wp_id"], got["status"], got["alive"], [w.x for w in wps], [w.y for w in wps], [w.psi for w in wps],
                          m.origin, m.resolution, circular=rp.circular)
    assert same_tracks(trk, want)
    assert np.any(tz[:, :, :, :2] != tz[:, :, :1, :2])                        # a neighbour moves along the horizon
    assert not all(np.array_equal(got[k], plain[k]) for k in plain)
    again = bm.rollout(cum[starts], poses, 6, traffic=tf, lookahead=LK.Lookahead(25))      # a later rollout does not anticipate again
    assert all(np.array_equal(again[k], plain[k]) for k in plain)
    bm.close()
