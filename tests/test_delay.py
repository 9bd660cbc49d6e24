"""Actuation delay in the device rollout and its compensation (K3d / K3q, mpmpc_rollout_set_delay): a command issued at step k
reaches the wheels at step k + d; the controller predicts its pose through the c commands in flight and plans from there.

CPU: the host twin (tests/emul_delay, the same delay_core.hpp) against the product's restatement (delay.Delay), against the
emulation's localise / advance and the plant's twin (c = 0 and d = 0 change no bit), the register's order, exact compensation
(d = c: the prediction of step k is the state of step k + c, bit for bit), the argument checks, the Python surface.
GPU: zero delay against no delay, the register and exact compensation on the device (one path and two routes), one call
against many and a resumed run, the closed loop against the host loop of the project's host classes around Delay.apply,
compensation against none, the error codes, BatchMPC.rollout(delay=...)."""
import ctypes as C
import inspect
import types

import numpy as np
import pytest

import mpc_np as M
import mpmpc
import mpmpc_testlib as T
import scenarios
import twins
import delay_twin
from delay import DELAY_MAX, Delay, Path, current_waypoint
from plant import IDENTITY, Plant
from spatial_bicycle_models import TemporalState

E_ARG, E_STATE = -1, -3
TS, L_CAR = 0.05, 0.12
KEYS = ("s", "pose", "cc", "wp_id", "x0", "u", "status", "counter", "alive")
# test_plant.py's plant of the closed-loop tests
NOISY = dict(speed_gain=0.97, steer_gain=1.03, steer_offset=0.01, wheelbase_scale=1.03, speed_lag=0.8, steer_lag=0.8, steer_rate=0.3,
             speed_noise=0.02, steer_noise=0.01, position_noise=0.002, heading_noise=0.005)

_d = T._d


@pytest.fixture(scope="module")
def twin():
    """The CPU twin of K3d / K3q (tests/emul_delay)."""
    return delay_twin.delay()


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, float), np.ascontiguousarray(b, float)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _sim():
    g1 = np.load(M.GOLDEN + "/g1_path_sim_track.npz")
    g3 = np.load(M.GOLDEN + "/g3_corridor.npz")
    return g1, g3, np.cumsum(g1["segment_lengths"])


def _lap():
    """Sim_Track as a delay.Path"""
    g1, _, cum = _sim()
    return Path(cum, g1["x"], g1["y"], g1["psi"], g1["kappa"])


def _two_routes():
    """the lap (rows 0 .. 199, circular) and its open second half (rows 200 .. 299 = waypoints 100 .. 199), laid end to end"""
    g1, g3, cum = _sim()
    tr = scenarios.sim_track()
    own = []
    for lo, hi in ((0, 200), (100, 200)):
        own.append(dict(kappa=tr.kappa[lo:hi].copy(), v_ref=tr.v_ref[lo:hi].copy(), ds_next=tr.ds_next[lo:hi].copy(),
                        ub=np.ascontiguousarray(g3["ub_free"][lo:hi]), lb=np.ascontiguousarray(g3["lb_free"][lo:hi]),
                        x=g1["x"][lo:hi].copy(), y=g1["y"][lo:hi].copy(), psi=g1["psi"][lo:hi].copy(),
                        border_ub=g1["border_ub"][lo:hi].copy(), border_lb=g1["border_lb"][lo:hi].copy(), cum_lengths=cum[lo:hi].copy()))
    cat, first = mpmpc.concat_routes(own)
    return cat, first, np.array([1, 0], np.int32)


def _route_path(cat, first, route):
    route = np.asarray(route)
    return Path(cat["cum_lengths"], cat["x"], cat["y"], cat["psi"], cat["kappa"], first=first[route], n_wp=np.diff(first)[route])


def _twin_predict(twin, path, i, c, q, pose, s):
    """K3d of the twin for car i of `path` -> (wp, pred_pose, pred_s, now, now_wp); outputs start from sentinels"""
    first, n = path.car(i)
    pred_pose, pred_s, now, now_wp = np.full(3, 7.0), np.full(1, 7.0), np.full(3, 7.0), C.c_int(-7)
    q, pose = np.ascontiguousarray(q, float), np.ascontiguousarray(pose, float)
    wp = twin.dl_emu_predict(n, first, _d(path.cum), _d(path.x), _d(path.y), _d(path.psi), _d(path.kappa), int(c), _d(q), L_CAR, TS, _d(pose),
                             float(s), _d(pred_pose), _d(pred_s), _d(now), C.byref(now_wp))
    return wp, pred_pose, pred_s[0], now, now_wp.value


def _car_state(path, i, w, rng):
    """a car near waypoint w of its route: a small lateral / heading / arc offset, random commands in flight"""
    first, n = path.car(i)
    r = first + w
    pose = np.array([path.x[r] + rng.uniform(-0.02, 0.02), path.y[r] + rng.uniform(-0.02, 0.02), path.psi[r] + rng.uniform(-0.2, 0.2)])
    s = float(path.cum[r]) + rng.uniform(-0.01, 0.01) if w > 0 else float(path.cum[r]) + rng.uniform(0.0, 0.01)
    q = np.stack([rng.uniform(0.3, 1.0, DELAY_MAX), rng.uniform(-0.4, 0.4, DELAY_MAX)], 1)
    return pose, s, q


# ---------------------------------------------------------------------------------------------------- CPU: dl_predict
def _compare_predict(twin, path, i, c, q, pose, s):
    """the twin against Delay.predict for one car, to test_plant.py's tolerance of pl_drive against Plant.drive (1e-14)"""
    wp, pp, ps, now, now_wp = _twin_predict(twin, path, i, c, q, pose, s)
    B = 1 if path.first is None else path.first.size
    poses, ss, qs = np.tile(pose, (B, 1)), np.full(B, s), np.tile(q, (B, 1, 1))
    ref = Delay(0, assumed=c).predict(poses, ss, qs, path, L_CAR, TS)
    assert wp == ref["wp"][i]
    assert np.max(np.abs(pp - ref["pred_pose"][i])) <= 1e-14 and abs(ps - ref["pred_s"][i]) <= 1e-14
    if wp >= 0:
        assert now_wp == ref["now_wp"][i] and np.max(np.abs(now - ref["now"][i])) <= 1e-14
    return wp, pp, ps, now, now_wp


def test_predict_matches_the_numpy_restatement(twin):
    lap = _lap()
    rng = np.random.default_rng(101)
    moved = 0
    for case in range(180):      # c = 0 .. 8, twenty states each
        c = case % 9
        w = int(rng.integers(0, 185))
        pose, s, q = _car_state(lap, 0, w, rng)
        wp, pp, ps, now, now_wp = _compare_predict(twin, lap, 0, c, q, pose, s)
        assert wp >= 0 and now_wp == wp
        moved += int(current_waypoint(lap.cum, ps) != wp)
        if c > 0:
            assert ps > s and not _same_bits(pp, pose)
    assert moved >= 20      # a waypoint change inside the prediction


def test_predict_on_the_second_route_and_at_the_open_end(twin):
    cat, first, circ = _two_routes()
    route = np.array([0, 1])
    path = _route_path(cat, first, route)
    rng = np.random.default_rng(102)
    n1 = int(np.diff(first)[1])
    end = float(cat["cum_lengths"][first[1] + n1 - 1])
    for c in range(9):      # a car on the second route (first row 200): its own cum, its geometry rows
        for w in (0, 1, 40, 80):
            pose, s, q = _car_state(path, 1, w, rng)
            wp, pp, ps, now, now_wp = _compare_predict(twin, path, 1, c, q, pose, s)
            assert wp >= 0 and now_wp == 200 + wp and now[2] == cat["kappa"][200 + wp]
    # the prediction passes the open end: it stops there, pred_s is past the end
    pose, s, q = _car_state(path, 1, n1 - 2, rng)
    q[:, 0], q[:, 1] = 1.0, 0.1      # (one command in every slot: a larger c only adds steps)
    stopped = None
    for c in range(1, 9):
        wp, pp, ps, now, now_wp = _compare_predict(twin, path, 1, c, q, pose, s)
        if stopped is None and ps >= end:
            stopped = (c, pp.copy(), ps)
        elif stopped is not None:      # more assumed steps change nothing: the loop ended when s passed the end
            assert _same_bits(pp, stopped[1]) and ps == stopped[2]
    assert stopped is not None and 1 <= stopped[0] < 8
    # s already past the end: passed through, `now` not written
    for c in (0, 3, 8):
        wp, pp, ps, now, now_wp = _twin_predict(twin, path, 1, c, q, pose, end + 0.25)
        assert wp == -1 and _same_bits(pp, pose) and ps == end + 0.25 and np.all(now == 7.0) and now_wp == -7
        ref = Delay(0, assumed=c).predict(np.tile(pose, (2, 1)), np.full(2, end + 0.25), np.tile(q, (2, 1, 1)), path, L_CAR, TS)
        assert ref["wp"][1] == -1 and _same_bits(ref["pred_pose"][1], pose) and ref["pred_s"][1] == end + 0.25


def test_no_assumed_delay_is_the_emulations_localise(twin, emu):
    lap = _lap()
    rng = np.random.default_rng(103)
    for case in range(100):
        w = int(rng.integers(0, 200))
        pose, s, q = _car_state(lap, 0, w, rng)
        wp, pp, ps, now, now_wp = _twin_predict(twin, lap, 0, 0, q, pose, s)
        x0, alive = np.zeros(3), C.c_int(0)
        ref = emu.lib.emu_localise(C.c_int(200), C.c_int(10), C.c_int(1), _d(lap.cum), _d(lap.x), _d(lap.y), _d(lap.psi), C.c_double(s),
                                   _d(pose), _d(x0), C.byref(alive))
        assert wp == ref and now_wp == ref
        assert _same_bits(pp, pose) and ps == s      # pred is the input, bit for bit
        assert _same_bits(now[:2], x0[:2]) and now[2] == lap.kappa[ref]


# ----------------------------------------------------------------------------------------------------- CPU: dl_drive
def _drive_cases(n=300):
    """teacher-forced random states at N = 5, test_plant.py's way"""
    rng = np.random.default_rng(78)
    N, cases = 5, []
    for c in range(n):
        p = np.array(IDENTITY)
        p[0], p[1], p[2], p[3] = rng.uniform(0.8, 1.2), rng.uniform(0.8, 1.2), rng.uniform(-0.05, 0.05), rng.uniform(0.9, 1.1)
        p[4] = 1.0 if c % 2 == 0 else rng.uniform(0.05, 0.999)
        p[5] = 1.0 if (c // 2) % 2 == 0 else rng.uniform(0.05, 0.999)
        p[6] = (np.inf, 10.0, rng.uniform(0.005, 0.05))[c % 3]
        p[7:] = rng.uniform(0.0, 0.05, 4)
        cases.append(dict(p=p, status=(1, 2, -2, -3, -4)[c % 5], counter=int(rng.integers(0, N - 1)), z=rng.uniform(-1, 1, 5 * N + 3),
                          cc=rng.uniform(-0.6, 0.9, 2 * N), x0=np.array([rng.uniform(-0.1, 0.1), rng.uniform(-0.3, 0.3), 0.0]),
                          kappa=rng.uniform(-3, 3), pose=rng.uniform(-3, 3, 3), s=rng.uniform(0, 20),
                          act=np.array([rng.uniform(0, 1), rng.uniform(-0.5, 0.5)]), n5=rng.uniform(-1, 1, 5),
                          q=np.stack([rng.uniform(0, 1, DELAY_MAX), rng.uniform(-0.5, 0.5, DELAY_MAX)], 1)))
    return N, cases


def _twin_advance(twin, N, c, d, plant=False):
    cc, pose, u, q, act = c["cc"].copy(), c["pose"].copy(), np.zeros(2), c["q"].copy(), c["act"].copy()
    counter, s = C.c_int(c["counter"]), np.array([c["s"]])
    now = np.array([c["x0"][0], c["x0"][1], c["kappa"]])
    if plant:
        alive = twin.dl_emu_advance_plant(N, L_CAR, TS, c["status"], _d(c["z"]), _d(cc), C.byref(counter), _d(now), d, _d(q),
                                          _d(np.ascontiguousarray(c["p"])), _d(np.ascontiguousarray(c["n5"])), _d(act), _d(pose), _d(s), _d(u))
    else:
        alive = twin.dl_emu_advance(N, L_CAR, TS, c["status"], _d(c["z"]), _d(cc), C.byref(counter), _d(now), d, _d(q), _d(pose), _d(s), _d(u))
    return dict(alive=alive, cc=cc, pose=pose, u=u, counter=counter.value, s=s[0], q=q, act=act)


def test_no_delay_is_the_emulations_advance_and_the_plants_drive(twin, emu):
    N, cases = _drive_cases()
    pl = twins.plant()
    seen = set()
    for c in cases:
        for plant in (False, True):
            got = _twin_advance(twin, N, c, 0, plant)
            cc, pose, u, act = c["cc"].copy(), c["pose"].copy(), np.zeros(2), c["act"].copy()
            counter, s = C.c_int(c["counter"]), np.array([c["s"]])
            if plant:
                alive = pl.pl_emu_advance(N, L_CAR, TS, c["status"], _d(c["z"]), _d(cc), C.byref(counter), _d(c["x0"]), c["kappa"],
                                          _d(np.ascontiguousarray(c["p"])), _d(np.ascontiguousarray(c["n5"])), _d(act), _d(pose), _d(s), _d(u))
            else:
                sc = C.c_double(c["s"])
                alive = emu.lib.emu_advance(C.c_int(N), C.c_double(L_CAR), C.c_double(TS), C.c_int(c["status"]), _d(c["z"]), _d(cc),
                                            C.byref(counter), _d(c["x0"]), C.c_double(c["kappa"]), _d(pose), C.byref(sc), _d(u))
                s[0] = sc.value
            assert got["alive"] == alive and got["counter"] == counter.value
            for k, v in (("cc", cc), ("pose", pose), ("u", u), ("act", act)):
                assert _same_bits(got[k], v), (k, plant)
            assert got["s"] == s[0]
            usable = c["status"] in (1, 2, -2)
            if not alive:      # the N - 1 ending leaves the register untouched
                assert not usable and c["counter"] == N - 2 and _same_bits(got["q"], c["q"])
            else:
                assert _same_bits(got["q"][0], got["u"]) and _same_bits(got["q"][1:], c["q"][:-1])
            seen.add((usable, bool(alive), plant))
    assert seen == {(True, True, False), (True, True, True), (False, True, False), (False, True, True), (False, False, False),
                    (False, False, True)}


def test_register_order(twin, emu):
    """The command of driven step j is executed at step j + d, the first d executions are queue0[d - 1] .. queue0[0], and on a
    fallback step the queued command is the fallback entry.  What was executed is read off the pose: the emulation's advance,
    made to drive the expected command, must give the same bits."""
    N, steps = 5, 14
    rng = np.random.default_rng(79)
    for d in range(DELAY_MAX + 1):
        q0 = np.stack([rng.uniform(0.1, 1, DELAY_MAX), rng.uniform(-0.5, 0.5, DELAY_MAX)], 1)
        st = dict(q=q0.copy(), pose=rng.uniform(-1, 1, 3), s=1.0, counter=0, cc=rng.uniform(0.1, 0.9, 2 * N))
        issued = []
        for j in range(steps):
            fallback = j in (4, 5, 9)
            case = dict(status=-3 if fallback else 1, counter=st["counter"], z=rng.uniform(-1, 1, 5 * N + 3), cc=st["cc"], pose=st["pose"],
                        s=st["s"], q=st["q"], x0=np.array([rng.uniform(-0.1, 0.1), rng.uniform(-0.3, 0.3), 0.0]), kappa=rng.uniform(-3, 3),
                        act=np.zeros(2))
            got = _twin_advance(twin, N, case, d)
            assert got["alive"] == 1
            if fallback:      # the fallback entry is commanded and queued
                assert _same_bits(got["u"], st["cc"][2 * (st["counter"] + 1):2 * (st["counter"] + 1) + 2]) and got["counter"] == st["counter"] + 1
            else:
                assert got["u"][0] == case["z"][3 * (N + 1)] and got["counter"] == 0
            issued.append(got["u"].copy())
            assert _same_bits(got["q"][0], got["u"]) and _same_bits(got["q"][1:], st["q"][:-1])
            want = issued[j - d] if j >= d else q0[d - 1 - j]
            # the emulation drives `want`: a fallback step at counter 0 reads plan entry 1
            cc = np.zeros(2 * N)
            cc[2:4] = want
            pose, u, counter, s = st["pose"].copy(), np.zeros(2), C.c_int(0), C.c_double(st["s"])
            assert emu.lib.emu_advance(C.c_int(N), C.c_double(L_CAR), C.c_double(TS), C.c_int(-3), _d(case["z"]), _d(cc), C.byref(counter),
                                       _d(case["x0"]), C.c_double(case["kappa"]), _d(pose), C.byref(s), _d(u)) == 1
            assert _same_bits(u, want) and _same_bits(got["pose"], pose) and got["s"] == s.value, (d, j)
            st = dict(q=got["q"], pose=got["pose"], s=got["s"], counter=got["counter"], cc=got["cc"])


@pytest.mark.parametrize("d", [1, 3, 8])
def test_exact_compensation_through_the_twin(twin, d):
    """d = c, 12 steps of arbitrary commands: the prediction of step k is the state at the beginning of step k + c, bit for bit"""
    lap = _lap()
    N, steps = 5, 12
    rng = np.random.default_rng(80 + d)
    for start in (3, 57, 140):
        pose, s, q = _car_state(lap, 0, start, rng)
        states, preds, cc, counter = [], [], rng.uniform(0.1, 0.9, 2 * N), 0
        for k in range(steps):
            states.append((pose.copy(), s))
            wp, pp, ps, now, now_wp = _twin_predict(twin, lap, 0, d, q, pose, s)
            assert wp >= 0
            preds.append((pp, ps))
            z = rng.uniform(-1, 1, 5 * N + 3)
            z[3 * (N + 1)::2][:N] = rng.uniform(0.2, 1.0, N)      # forward speeds
            status = -3 if k in (5, 6) else 1
            cc2, pose2, u, q2 = cc.copy(), pose.copy(), np.zeros(2), q.copy()
            cnt, s2 = C.c_int(counter), np.array([s])
            assert twin.dl_emu_advance(N, L_CAR, TS, status, _d(z), _d(cc2), C.byref(cnt), _d(now), d, _d(q2), _d(pose2), _d(s2), _d(u)) == 1
            cc, pose, s, q, counter = cc2, pose2, float(s2[0]), q2, cnt.value
        states.append((pose.copy(), s))
        for k in range(steps + 1 - d):
            assert _same_bits(preds[k][0], states[k + d][0]) and preds[k][1] == states[k + d][1], (start, k)
        assert not _same_bits(states[0][0], states[d][0])      # (the car moved)


# ------------------------------------------------------------------------------------------ CPU: checks and surface
def test_argument_checks(twin):
    ip = C.POINTER(C.c_int32)

    def check(B, mb, delay, assumed=None, queue0=None):
        dd = np.ascontiguousarray(delay, np.int32)
        aa = None if assumed is None else np.ascontiguousarray(assumed, np.int32)
        return twin.dl_emu_check(B, mb, dd.ctypes.data_as(ip), None if aa is None else aa.ctypes.data_as(ip),
                                 _d(None if queue0 is None else np.ascontiguousarray(queue0, float)))
    B = 3
    assert twin.dl_emu_max() == DELAY_MAX == 8
    assert check(B, 8, [0, 8, 3]) == 0 and check(B, 8, [0, 8, 3], [8, 0, 5]) == 0
    assert check(B, 8, [0, 8, 3], None, np.ones((B, 8, 2))) == 0
    for car in range(B):      # row by row
        for bad in (-1, 9, 2 ** 31 - 1, -2 ** 31):
            d = [1, 2, 3]
            d[car] = bad
            assert check(B, 8, d) == E_ARG and check(B, 8, [1, 2, 3], d) == E_ARG
        for good in (0, 8):
            d = [1, 2, 3]
            d[car] = good
            assert check(B, 8, d) == 0 and check(B, 8, [1, 2, 3], d) == 0
        for bad in (np.nan, np.inf, -np.inf):
            for slot in (0, 7):
                for ch in (0, 1):
                    q = np.zeros((B, 8, 2))
                    q[car, slot, ch] = bad
                    assert check(B, 8, [1, 2, 3], None, q) == E_ARG
    assert check(0, 8, [1, 2, 3]) == E_ARG and check(9, 8, [1] * 9) == E_ARG and check(8, 8, [1] * 8) == 0
    # Delay.arrays: scalars and per-car values
    d, a, q = Delay(3).arrays(4)
    assert d.tolist() == [3] * 4 and a.tolist() == [3] * 4 and q is None and d.dtype == np.int32
    d, a, q = Delay([1, 2, 3], assumed=0, queue0=np.ones((8, 2))).arrays(3)
    assert d.tolist() == [1, 2, 3] and a.tolist() == [0, 0, 0] and q.shape == (3, 8, 2)
    for bad in (dict(steps=[1, 2]), dict(steps=9), dict(steps=-1), dict(steps=1.5), dict(steps=1, assumed=9),
                dict(steps=1, queue0=np.zeros((2, 8, 2)))):
        with pytest.raises(ValueError):
            Delay(**bad).arrays(3)
    one = Delay([1, 2, 3], assumed=[3, 2, 1], queue0=np.arange(48.0).reshape(3, 8, 2)).car(2)
    assert one.arrays(1)[0].tolist() == [3] and one.arrays(1)[1].tolist() == [1] and one.arrays(1)[2][0, 0].tolist() == [32.0, 33.0]


def test_python_surface():
    from MPC import BatchMPC
    assert "delay" in inspect.signature(BatchMPC.rollout).parameters
    for name in ("rollout_set_delay", "rollout_delay"):
        assert hasattr(mpmpc.Handle, name)
    assert mpmpc.Handle.DELAY_FIELDS == ("queue", "pred_pose", "pred_s", "now")
    for name in ("mpmpc_rollout_set_delay", "mpmpc_rollout_delay"):
        assert name in mpmpc.EXPORTS
    header = open(T.ROOT + "/include/mpmpc.h").read()
    assert "#define MPMPC_DELAY_MAX 8" in header and "int mpmpc_rollout_set_delay(" in header and "int mpmpc_rollout_delay(" in header


def test_batchmpc_refuses_delay_with_lookahead():
    """ValueError before any device call: the stand-in's handle fails on every use"""
    from MPC import BatchMPC

    class NoDevice:
        def __getattr__(self, name):
            raise AssertionError("device call: " + name)
    bm = BatchMPC.__new__(BatchMPC)
    bm._path, bm.corridor_cols, bm.handle = types.SimpleNamespace(), 30, NoDevice()
    with pytest.raises(ValueError, match="delay and lookahead"):
        bm.rollout(np.zeros(2), np.zeros((2, 3)), 1, delay=Delay(3), lookahead=types.SimpleNamespace(max_lead=2, traffic=False))


# ------------------------------------------------------------------------------------------------------------ GPU
def _handle(N, B, warm=None):
    """Sim_Track, the free grid's corridor table"""
    g1, g3, cum = _sim()
    tr = scenarios.sim_track()
    h = mpmpc.Handle(T.stock_config(N, max_batch=B))
    h.set_path(tr.kappa, tr.v_ref, tr.ds_next)
    h.set_corridor(g3["ub_free"], g3["lb_free"])
    h.set_path_geometry(g1["x"], g1["y"], g1["psi"], g1["border_ub"], g1["border_lb"])
    if warm is not None:
        h.rollout_warm_start(warm)
    return h


def _starts(B, seed, last=200):
    g1, _, cum = _sim()
    w = np.random.default_rng(seed).integers(0, last, B)
    return w, cum[w], np.stack([g1["x"][w], g1["y"][w], g1["psi"][w]], axis=1)


def _equal_states(a, b):
    for k in KEYS:
        same = np.array_equal(a[k], b[k]) if a[k].dtype.kind == "i" else _same_bits(a[k], b[k])
        assert same, k


def _code(err):
    return int(str(err.value).split("mpmpc error ")[1].split(":")[0])


def _in_flight(B, v=0.6, delta=0.0):
    q = np.zeros((B, DELAY_MAX, 2))
    q[:, :, 0], q[:, :, 1] = v, delta
    return q


@pytest.mark.gpu
@pytest.mark.parametrize("plant", [False, True])
def test_zero_delay_changes_nothing(plant):
    """N = 10, B = 300: in K3q a block of 256 threads ends inside a car.  d = c = 0 against a handle without the setting, and
    the same under test_plant.py's noisy plant against a plant-only handle."""
    N, B, steps = 10, 300, 25
    _, _, cum = _sim()
    w, s0, poses = _starts(B, 21)
    pl = Plant(seed=99, **NOISY)
    out = []
    for delayed in (False, True):
        h = _handle(N, B)
        if plant:
            h.rollout_set_plant(pl.params(B), pl.seed)
        if delayed:
            h.rollout_set_delay(np.zeros(B, np.int32), queue0=_in_flight(B))      # (in flight, never executed)
        h.rollout_init(TS, cum, s0, poses)
        h.rollout_step(steps)
        out.append((h.rollout_state(), h.rollout_plant() if plant else None, h.rollout_delay() if delayed else None))
        h.close()
    (want, want_pl, _), (got, got_pl, dl) = out
    _equal_states(got, want)
    if plant:
        for k in mpmpc.Handle.PLANT_FIELDS:
            assert np.array_equal(got_pl[k], want_pl[k]), k
    alive = got["alive"] == 1
    assert alive.sum() > B // 2
    assert _same_bits(dl["queue"][alive, 0], got["u"][alive])
    if not plant:      # the prediction is the input: the pose the last step started from is not kept, its x0 is
        assert _same_bits(dl["now"][alive, :2], got["x0"][alive, :2])


@pytest.mark.gpu
def test_register_on_the_device():
    """d = car index mod 9, c = 0, a deterministic plant: the actuator state after step k is Plant.drive's recursion on the u
    recorded at step k - d (queue0 before that), bit for bit, and the register holds the last 8 u."""
    N, B, steps = 10, 300, 12
    _, _, cum = _sim()
    w, s0, poses = _starts(B, 22, last=160)
    d = (np.arange(B) % 9).astype(np.int32)
    rng = np.random.default_rng(23)
    q0 = np.stack([rng.uniform(0.2, 0.8, (B, DELAY_MAX)), rng.uniform(-0.2, 0.2, (B, DELAY_MAX))], 2)
    plant = Plant(speed_gain=0.9, steer_lag=0.5)
    h = _handle(N, B)
    h.rollout_set_plant(plant.params(B))
    h.rollout_init(TS, cum, s0, poses)
    h.rollout_set_delay(d, np.zeros(B, np.int32), q0)
    queue, act = q0.copy(), np.zeros((B, 2))
    driven_steps = np.zeros(B, int)
    for k in range(steps):
        h.rollout_step(1)
        st, pl, dl = h.rollout_state(), h.rollout_plant(), h.rollout_delay()
        driven = st["alive"] == 1
        ex = np.where((d > 0)[:, None], queue[np.arange(B), np.maximum(d - 1, 0)], st["u"])
        new_act = plant.drive(k, ex, np.zeros((B, 3)), np.zeros(B), act, np.zeros((B, 2)), np.zeros(B), L_CAR, TS)[2]
        act = np.where(driven[:, None], new_act, act)
        queue = np.where(driven[:, None, None], np.concatenate([st["u"][:, None, :], queue[:, :-1]], 1), queue)
        driven_steps += driven
        assert _same_bits(pl["act"], act), k
        assert _same_bits(dl["queue"], queue), k
    h.close()
    assert np.sum(driven_steps == steps) > B // 2
    full = driven_steps == steps      # every delay occurs among the cars driven throughout; the first d executions were queue0's
    assert set(d[full].tolist()) == set(range(9))


def _compensation_run(h, B, d, cum, s0, poses, steps, q0):
    h.rollout_init(TS, cum, s0, poses)
    h.rollout_set_delay(d, d, q0)
    states, preds = [], []
    for k in range(steps):
        st = h.rollout_state()
        states.append((st["pose"], st["s"]))
        h.rollout_step(1)
        dl = h.rollout_delay()
        preds.append((dl["pred_pose"], dl["pred_s"]))
    st = h.rollout_state()
    states.append((st["pose"], st["s"]))
    through = st["alive"] == 1
    checked = 0
    for k in range(steps):
        for c in range(DELAY_MAX + 1):
            cars = through & (d == c)
            if k + c <= steps and cars.any():
                assert _same_bits(preds[k][0][cars], states[k + c][0][cars]), (k, c)
                assert _same_bits(preds[k][1][cars], states[k + c][1][cars]), (k, c)
                checked += int(cars.sum())
    return st, through, checked


@pytest.mark.gpu
def test_exact_compensation_on_the_device():
    """d = c = car index mod 9, no plant: pred_pose / pred_s of step k are pose / s found at step k + c, bit for bit"""
    N, B, steps = 10, 300, 20
    _, _, cum = _sim()
    w, s0, poses = _starts(B, 24, last=150)
    d = (np.arange(B) % 9).astype(np.int32)
    h = _handle(N, B)
    st, through, checked = _compensation_run(h, B, d, cum, s0, poses, steps, _in_flight(B))
    h.close()
    assert through.sum() > B // 2 and set(d[through].tolist()) == set(range(9)) and checked > 2000
    assert np.all(np.abs(st["pose"][through] - poses[through]).max(axis=1) > 0.1)      # (they drove)


@pytest.mark.gpu
def test_exact_compensation_on_two_routes():
    """16 cars, half of them on the second route (first row 200 of the tables)"""
    N, B, steps = 10, 16, 14
    cat, first, circ = _two_routes()
    route = (np.arange(B) % 2).astype(np.int32)
    wp = np.where(route == 0, np.arange(B) * 11 % 180, np.arange(B) * 5 % 60).astype(int)
    g = first[route] + wp
    s0, poses = cat["cum_lengths"][g], np.stack([cat["x"][g], cat["y"][g], cat["psi"][g]], 1)
    d = (np.arange(B) // 2 % 9).astype(np.int32)
    h = mpmpc.Handle(T.stock_config(N, max_batch=B, circular=False))
    h.set_path(cat["kappa"], cat["v_ref"], cat["ds_next"])
    h.set_corridor(cat["ub"], cat["lb"])
    h.set_routes(first, circ)
    h.set_path_geometry(cat["x"], cat["y"], cat["psi"], cat["border_ub"], cat["border_lb"])
    h.set_car_routes(route)
    st, through, checked = _compensation_run(h, B, d, cat["cum_lengths"], s0, poses, steps, _in_flight(B))
    dl = h.rollout_delay()
    h.close()
    assert through[route == 1].sum() >= 6 and through[route == 0].sum() >= 6 and checked > 100
    # `now` belongs to the car's own route: kappa of a row of the second route
    second = through & (route == 1)
    assert np.all(np.isin(dl["now"][second, 2], cat["kappa"][200:]))


@pytest.mark.gpu
def test_one_call_equals_many_and_a_resumed_run():
    N, B, steps, at = 10, 70, 25, 10
    _, _, cum = _sim()
    w, s0, poses = _starts(B, 25, last=160)
    plant = Plant(seed=4242, car0=5, **NOISY)
    d = (np.arange(B) % 4).astype(np.int32)
    c = np.where(np.arange(B) % 8 < 4, d, np.maximum(d - 1, 0)).astype(np.int32)      # exact and under-estimated
    h = _handle(N, B, warm=False)
    h.rollout_set_plant(plant.params(B), plant.seed, plant.car0)
    h.rollout_init(TS, cum, s0, poses)
    h.rollout_set_delay(d, c, _in_flight(B))
    h.rollout_step(steps)
    want, want_pl, want_dl = h.rollout_state(), h.rollout_plant(), h.rollout_delay()
    h.rollout_init(TS, cum, s0, poses)      # (d and c stay, the registers are zeroed: the commands in flight are set again)
    h.rollout_set_delay(d, c, _in_flight(B))
    for t in range(steps):
        if t == at:
            saved, saved_pl, saved_dl = h.rollout_state(), h.rollout_plant(), h.rollout_delay()
        h.rollout_step(1)
    got, got_pl, got_dl = h.rollout_state(), h.rollout_plant(), h.rollout_delay()
    _equal_states(got, want)
    for k in mpmpc.Handle.PLANT_FIELDS:
        assert np.array_equal(got_pl[k], want_pl[k]), k
    for k in mpmpc.Handle.DELAY_FIELDS:
        assert _same_bits(got_dl[k], want_dl[k]), k
    # resumed from the save
    h.rollout_init(TS, cum, saved["s"], saved["pose"], saved["cc"])
    h.rollout_set_counters(saved["counter"])
    h.rollout_set_plant(plant.params(B), plant.seed, plant.car0, step0=-at, act0=saved_pl["act"])
    h.rollout_set_delay(d, c, saved_dl["queue"])
    h.rollout_step(steps - at)
    res, res_pl, res_dl = h.rollout_state(), h.rollout_plant(), h.rollout_delay()
    h.close()
    # a resumed run starts every car alive: the cars that were running at the save are compared (cars do not interact; some of
    # those that under-estimate their delay under this plant have ended by then, and some end later - in both runs alike)
    on = saved["alive"] == 1
    assert on.sum() > B // 2 and (c < d)[on].any() and (want["alive"] == 1)[on].sum() > B // 2
    _equal_states({k: res[k][on] for k in KEYS}, {k: want[k][on] for k in KEYS})
    assert _same_bits(res_pl["act"][on], want_pl["act"][on]) and _same_bits(res_pl["meas"][on], want_pl["meas"][on])
    for k in mpmpc.Handle.DELAY_FIELDS:
        assert _same_bits(res_dl[k][on], want_dl[k][on]), k
    assert not _same_bits(saved_dl["queue"], _in_flight(B))


def _host_loop(N, starts, delay, steps):
    """the reference's loop with the project's host classes, one car at a time, around Delay.apply"""
    g1, _, cum = _sim()
    lap = _lap()
    rows, statuses = [], []
    for i, w in enumerate(starts):
        m, rp, car = T.build_world(obstacles=False)
        mpc = T.make_mpc(car, N)
        one = delay.car(i)
        st = dict(pose=np.array([[rp.waypoints[w].x, rp.waypoints[w].y, rp.waypoints[w].psi]]), s=np.array([float(cum[w])]), queue=one.queue(1))

        def control(pred_pose, pred_s):
            car.s = float(pred_s[0])
            car.temporal_state = TemporalState(*pred_pose[0])
            u = mpc.get_control()
            statuses.append(mpc.last_status)
            return u
        for k in range(steps):
            st = one.apply(k, st["pose"], st["s"], st["queue"], control, lap, car.length, car.Ts)
        rows.append(np.concatenate([st["s"], st["pose"][0], st["pred_pose"][0], st["u"][0], st["executed"][0]]))
    return np.array(rows), statuses


CLOSED_LOOP = {"a": ([0, 12, 37, 88, 120, 150, 171], [3, 1, 2, 5, 3, 1, 2], None),      # d = c
               "b": ([0, 12, 37, 120, 150, 171], 1, 0)}                                 # d = 1, no compensation


@pytest.mark.gpu
@pytest.mark.parametrize("N", [10, 30])
@pytest.mark.parametrize("case", ["a", "b"])
def test_closed_loop_matches_the_host_loop(case, N):
    """(a) d = c per car, (b) d = 1 without compensation; bounds s, pose, pred_pose 1e-8 and u, executed 1e-6 (test_plant.py's).
    Measured on an MI355X (printed below): at most 1.4e-14 on s, pose and pred_pose and 4.2e-14 on u and
    executed, both at (a), N = 30."""
    g1, _, cum = _sim()
    steps = 25
    starts, d, c = CLOSED_LOOP[case]
    starts = np.array(starts)
    B = starts.size
    delay = Delay(d, assumed=c, queue0=_in_flight(B))
    host, statuses = _host_loop(N, starts, delay, steps)
    assert all(v == 1 for v in statuses), statuses      # the comparison must not cross a verdict boundary
    h = _handle(N, B)
    poses = np.stack([g1["x"][starts], g1["y"][starts], g1["psi"][starts]], axis=1)
    h.rollout_init(TS, cum, cum[starts], poses)
    h.rollout_set_delay(*delay.arrays(B))
    h.rollout_step(steps)
    st, dl = h.rollout_state(), h.rollout_delay()
    h.close()
    dd = delay.arrays(B)[0]
    executed = np.where((dd > 0)[:, None], dl["queue"][np.arange(B), dd], st["u"])      # what left the register in the last step
    figures = dict(s=np.max(np.abs(st["s"] - host[:, 0])), pose=np.max(np.abs(st["pose"] - host[:, 1:4])),
                   pred_pose=np.max(np.abs(dl["pred_pose"] - host[:, 4:7])), u=np.max(np.abs(st["u"] - host[:, 7:9])),
                   executed=np.max(np.abs(executed - host[:, 9:11])))
    print("delay closed loop (%s) N=%d:" % (case, N), figures)
    assert np.all(st["alive"] == 1)
    assert figures["s"] <= 1e-8 and figures["pose"] <= 1e-8 and figures["pred_pose"] <= 1e-8
    assert figures["u"] <= 1e-6 and figures["executed"] <= 1e-6


@pytest.mark.gpu
def test_compensation_helps():
    """d = 3 on every car, an identity plant for ey_max: the fleet that assumes 3 stays feasible and tracks better, car by car,
    than the fleet that assumes 0"""
    N, steps = 10, 25
    g1, _, cum = _sim()
    starts = np.array(CLOSED_LOOP["a"][0])
    B = starts.size
    poses = np.stack([g1["x"][starts], g1["y"][starts], g1["psi"][starts]], axis=1)
    out = {}
    for c in (3, 0):
        h = _handle(N, B)
        h.rollout_set_plant(Plant().params(B))
        h.rollout_init(TS, cum, cum[starts], poses)
        h.rollout_set_delay(*Delay(3, assumed=c, queue0=_in_flight(B)).arrays(B))
        h.rollout_step(steps)
        out[c] = (h.rollout_state(), h.rollout_plant())
        h.close()
    (st3, pl3), (st0, pl0) = out[3], out[0]
    print("ey_max compensated %s\nuncompensated %s, alive %s" % (pl3["ey_max"], pl0["ey_max"], st0["alive"]))
    assert np.all(st3["alive"] == 1) and np.all(st3["counter"] == 0)
    assert np.all(pl3["ey_max"] < pl0["ey_max"])


@pytest.mark.gpu
def test_state_and_argument_errors():
    N, B = 10, 8
    g1, _, cum = _sim()
    w, s0, poses = _starts(B, 26, last=160)
    d = (np.arange(B) % 4).astype(np.int32)
    h = _handle(N, B, warm=False)
    h.rollout_init(TS, cum, s0, poses)
    with pytest.raises(mpmpc.MpmpcError) as e:
        h.rollout_delay()      # no delay
    assert _code(e) == E_STATE
    h.rollout_set_delay(d, d, _in_flight(B))
    with pytest.raises(mpmpc.MpmpcError) as e:
        h.rollout_delay()      # no step under it yet
    assert _code(e) == E_STATE
    h.rollout_step(3)
    h.rollout_step(3)
    want, want_dl = h.rollout_state(), h.rollout_delay()
    # a refused call leaves the running setting's next step unchanged
    h.rollout_init(TS, cum, s0, poses)
    h.rollout_set_delay(d, d, _in_flight(B))
    h.rollout_step(3)
    for bad in (-1, 9):
        x = d.copy()
        x[B - 1] = bad
        for args in ((x, d), (d, x)):
            with pytest.raises(mpmpc.MpmpcError) as e:
                h.rollout_set_delay(*args)
            assert _code(e) == E_ARG
    for bad in (np.nan, np.inf):
        q = _in_flight(B)
        q[B - 1, 7, 1] = bad
        with pytest.raises(mpmpc.MpmpcError) as e:
            h.rollout_set_delay(d, d, q)
        assert _code(e) == E_ARG
    with pytest.raises(mpmpc.MpmpcError) as e:
        h.rollout_set_delay(np.zeros(B + 1, np.int32))      # more than max_batch
    assert _code(e) == E_ARG
    h.rollout_step(3)
    got, got_dl = h.rollout_state(), h.rollout_delay()
    _equal_states(got, want)
    for k in mpmpc.Handle.DELAY_FIELDS:
        assert _same_bits(got_dl[k], want_dl[k]), k
    # a lookahead in force
    tr = scenarios.sim_track()
    h.rollout_set_lookahead(tr.ds_next / tr.v_ref, 2)
    with pytest.raises(mpmpc.MpmpcError) as e:
        h.rollout_step(1)
    assert _code(e) == E_STATE
    h.rollout_set_lookahead(None)
    h.rollout_step(1)
    # a step of another B
    h.rollout_init(TS, cum, s0[:5], poses[:5])
    with pytest.raises(mpmpc.MpmpcError) as e:
        h.rollout_step(1)
    assert _code(e) == E_STATE
    h.rollout_set_delay(None)
    h.rollout_step(1)      # without a delay: any B the rollout holds
    with pytest.raises(mpmpc.MpmpcError) as e:
        h.rollout_delay()
    assert _code(e) == E_STATE
    h.close()


@pytest.mark.gpu
def test_batchmpc_rollout_takes_a_delay():
    """BatchMPC.rollout(..., delay=Delay(3)) returns "delay"; a following rollout without it is bit-equal to a controller that
    never had one"""
    from MPC import BatchMPC
    from scipy import sparse
    _, g3, cum = _sim()
    m, rp, car = T.build_world(obstacles=False)
    Q, R, QN = sparse.diags([1.0, 0.0, 0.0]), sparse.diags([0.5, 0.0]), sparse.diags([1.0, 0.0, 0.0])
    ic = {'umin': np.array([0.0, -np.tan(0.66) / car.length]), 'umax': np.array([1.0, np.tan(0.66) / car.length])}
    sc = {'xmin': np.array([-np.inf] * 3), 'xmax': np.array([np.inf] * 3)}
    B, N, steps = 8, 10, 12
    w, s0, poses = _starts(B, 27, last=160)
    fresh = BatchMPC(car, N, Q, R, QN, sc, ic, 4.0, max_batch=B, corridor=(g3["ub_free"], g3["lb_free"]))
    plain = fresh.rollout(s0, poses, steps)
    assert "delay" not in plain
    bm = BatchMPC(car, N, Q, R, QN, sc, ic, 4.0, max_batch=B, corridor=(g3["ub_free"], g3["lb_free"]))
    out = bm.rollout(s0, poses, steps, delay=Delay(3, queue0=_in_flight(B)))
    dl = out.pop("delay")
    assert set(dl) == set(mpmpc.Handle.DELAY_FIELDS) and dl["queue"].shape == (B, 8, 2)
    assert np.all(out["alive"] == 1) and _same_bits(dl["queue"][:, 0], out["u"])
    assert np.all(np.abs(out["pose"] - plain["pose"]).max(axis=1) > 0)
    assert bm.rollout(s0, poses, 0, delay=Delay(3))["delay"] is None
    again = bm.rollout(s0, poses, steps)      # off again
    _equal_states(again, plain)
    with pytest.raises(mpmpc.MpmpcError):
        bm.handle.rollout_delay()
