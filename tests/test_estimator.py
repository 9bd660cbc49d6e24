"""Pose estimator in the device rollout (K3e, mpmpc_rollout_set_estimator): per car a 3-state extended Kalman filter on the world
pose in the controller's nominal model, with a measurement schedule; the controller localises on the estimate.

CPU: the host twin (tests/emul_estimator, the same estimator_core.hpp) against the product's restatement
(estimator.Estimator.update) and against a joint-form Kalman update, exactness when there is nothing to estimate (through
ro_drive and through the delay's twin), the schedule, the covariance over a long run, the filter against the raw measurement,
the argument checks, the Python surface.
GPU: set-and-cleared against never set, exactness on the device (one path and two routes, with and without a delay), K3e
against the twin step by step, one call against many and a resumed run, the closed loop against the host loop around
Estimator.apply, the estimator against none, the error codes, BatchMPC.rollout(estimator=...)."""
import ctypes as C
import inspect
import math
import types

import numpy as np
import pytest

import mpmpc
import mpmpc_testlib as T
import delay_twin
import estimator_twin
import test_delay as TD      # (its Sim_Track handles, starts and closed-loop cases)
from delay import DELAY_MAX, Delay
from estimator import Estimator, fresh, wrap
from plant import Plant
from spatial_bicycle_models import TemporalState

E_ARG, E_STATE = -1, -3
TS, L_CAR = TD.TS, TD.L_CAR
KEYS = TD.KEYS
_d, _same_bits, _sim, _code = T._d, TD._same_bits, TD._sim, TD._code
# the open-loop drive of the filter tests: v 0.8, delta = 0.3 sin(0.1 k), noise amplitudes 0.03 m and 0.05 rad
A_XY, A_PSI = 0.03, 0.05


@pytest.fixture(scope="module")
def twin():
    """The CPU twin of K3e (tests/emul_estimator)."""
    return estimator_twin.estimator()


class TwinCar:
    """one car's filter state around es_emu_step"""

    def __init__(self, twin, est, car=0):
        self.twin, self.e, self.car = twin, est, car
        self.p = np.ascontiguousarray(est.params(car + 1)[car])
        self.est, self.cov, self.st = np.zeros(3), np.zeros(6), np.zeros(4)
        self.primed, self.used, self.steps = C.c_int(0), C.c_int(0), C.c_int(0)

    def step(self, k, z, pose, cmd):
        z, pose, cmd = (np.ascontiguousarray(a, float) for a in (z, pose, cmd))
        return self.twin.es_emu_step(_d(self.p), self.e.seed & (2 ** 64 - 1), (self.e.car0 + self.car) & 0xFFFFFFFF, k - self.e.step0, L_CAR, TS,
                                     _d(z), _d(pose), _d(cmd), _d(self.est), _d(self.cov), C.byref(self.primed), _d(self.st),
                                     C.byref(self.used), C.byref(self.steps))

    def state(self):
        return dict(est=self.est[None].copy(), cov=self.cov[None].copy(), primed=np.array([self.primed.value], np.int32),
                    err2_max=self.st[0:1].copy(), err2_sum=self.st[1:2].copy(), meas2_sum=self.st[2:3].copy(), head2_sum=self.st[3:4].copy(),
                    used=np.array([self.used.value], np.int32), steps=np.array([self.steps.value], np.int32))


def _drive(twin, pose, v, delta):
    """the nominal model's step (ro_drive itself) -> the new pose"""
    pose, s = np.array(pose, float), np.zeros(1)
    twin.es_emu_drive(L_CAR, TS, v, delta, _d(np.zeros(3)), 0.0, _d(pose), _d(s))
    return pose


def _command(k):
    return 0.8, 0.3 * math.sin(0.1 * k)


def _open_loop(twin, steps, plant):
    """-> (true poses [steps, 3], measured poses [steps, 3], commands [steps, 2]): the open-loop drive, pose k measured at step k"""
    pose, poses, cmds = np.array([0.3, -0.2, 0.4]), [], []
    for k in range(steps):
        poses.append(pose.copy())
        cmds.append(_command(k))
        pose = _drive(twin, pose, *cmds[-1])
    poses = np.array(poses)
    meas = np.array([plant.measure(k, poses[k])[0] for k in range(steps)])
    return poses, meas, np.array(cmds)


# ------------------------------------------------------------------------------------------- CPU: the twin against numpy
def test_single_steps_match_the_numpy_restatement(twin):
    """seeded states, every branch: un-primed, time update alone (unscheduled, dropped), time and measurement update; 1e-14 as
    test_plant.py's pl_drive against Plant.drive"""
    rng = np.random.default_rng(301)
    seen = set()
    for case in range(400):
        e = Estimator(rng.uniform(0, 1e-4), rng.uniform(0, 1e-4), rng.uniform(1e-5, 1e-3), rng.uniform(1e-5, 1e-3), rng.uniform(0, 1e-2),
                      rng.uniform(0, 1e-2), period=(1, 3, 8)[case % 3], drop=(0.0, 0.3)[case // 3 % 2], seed=int(rng.integers(0, 2 ** 63)),
                      car0=int(rng.integers(-5, 50)), step0=int(rng.integers(-20, 20)))
        car = TwinCar(twin, e)
        k = int(rng.integers(-30, 60))
        pose = np.array([rng.uniform(-3, 3), rng.uniform(-3, 3), rng.uniform(-7, 7)])
        z = pose + np.array([rng.uniform(-0.03, 0.03), rng.uniform(-0.03, 0.03), rng.uniform(-0.05, 0.05) + (2 * np.pi if case % 7 == 0 else 0.0)])
        cmd = np.array([rng.uniform(0, 1), rng.uniform(-0.6, 0.6)])
        if case % 5:      # primed, with a valid covariance A A^T
            a = rng.uniform(-0.05, 0.05, (3, 3))
            P = a @ a.T
            car.est[:] = pose + rng.uniform(-0.02, 0.02, 3)
            car.cov[:] = P[np.triu_indices(3)]
            car.primed.value = 1
            car.st[:] = rng.uniform(0, 1, 4)
            car.used.value, car.steps.value = 3, 7
        before = car.state()
        took = car.step(k, z, pose, cmd)
        ref = e.update(k, z[None], pose[None], cmd[None], before, L_CAR, TS)
        got = car.state()
        assert took == int(ref["took"][0]) and took == int(e.available(k, 1)[0] or not before["primed"][0])
        for key in ("est", "cov") + tuple(mpmpc.Handle.ESTIMATOR_FIELDS[2:6]):
            assert np.max(np.abs(got[key] - ref[key])) <= 1e-14, (case, key)
        for key in ("primed", "used", "steps"):
            assert np.array_equal(got[key], ref[key]), (case, key)
        assert got["primed"][0] == 1 and got["steps"][0] == before["steps"][0] + 1
        seen.add((int(before["primed"][0]), took))
    assert seen == {(0, 1), (1, 0), (1, 1)}


def test_sequential_updates_equal_the_joint_form(twin):
    """200 steps of the open-loop drive: the twin against a filter of its own with K = P (P + R)^-1 (numpy.linalg) and the
    same time update in matrix form.  est to 1e-12, cov to 1e-12 of its largest entry; a numpy restatement of the law measured
    6e-15 on est."""
    steps = 200
    plant = Plant(position_noise=A_XY, heading_noise=A_PSI, seed=11)
    e = Estimator.matched(plant, q_xy=1e-6, q_psi=1e-6)
    poses, meas, cmds = _open_loop(twin, steps, plant)
    p = e.params(1)[0]
    Q, R = np.diag([p[0], p[0], p[1]]), np.diag([p[2], p[2], p[3]])
    car = TwinCar(twin, e)
    x, P = None, None
    worst = [0.0, 0.0]
    for k in range(steps):
        car.step(k, meas[k], poses[k], cmds[k - 1] if k else np.zeros(2))
        if x is None:
            x, P = meas[k].copy(), np.diag([p[4], p[4], p[5]])
        else:
            v, delta = cmds[k - 1]
            F = np.eye(3)
            F[0, 2], F[1, 2] = -v * math.sin(x[2]) * TS, v * math.cos(x[2]) * TS
            x = x + np.array([v * math.cos(x[2]) * TS, v * math.sin(x[2]) * TS, v / L_CAR * math.tan(delta) * TS])
            P = F @ P @ F.T + Q
            nu = meas[k] - x
            nu[2] = wrap(meas[k][2], x[2])
            K = P @ np.linalg.inv(P + R)
            x = x + K @ nu
            P = (np.eye(3) - K) @ P
        worst[0] = max(worst[0], np.max(np.abs(car.est - x)))
        worst[1] = max(worst[1], np.max(np.abs(car.cov - P[np.triu_indices(3)])) / np.max(np.abs(P)))
    print("sequential against joint: est %.2e, cov (relative) %.2e" % tuple(worst))
    assert worst[0] <= 1e-12 and worst[1] <= 1e-12
    assert car.used.value == steps


# ---------------------------------------------------------------------------------- CPU: nothing to estimate, nothing changes
def _any_estimator(rng, case):
    return Estimator(rng.uniform(0, 1e-3), rng.uniform(0, 1e-3), rng.uniform(1e-6, 1e-2), rng.uniform(1e-6, 1e-2), rng.uniform(0, 1e-2),
                     rng.uniform(0, 1e-2), period=(1, 3, 8)[case % 3], drop=(0.0, 0.3, 0.9)[case % 3], seed=case)


def test_exact_through_ro_drive(twin):
    """no noise, no delay: est has the bits of the pose on every step, for any q, r, period and drop"""
    rng = np.random.default_rng(302)
    for case in range(6):
        car = TwinCar(twin, _any_estimator(rng, case))
        pose, cmd = rng.uniform(-2, 2, 3), np.zeros(2)
        for k in range(40):
            car.step(k, pose, pose, cmd)
            assert _same_bits(car.est, pose), (case, k)
            cmd = np.array([rng.uniform(0.1, 1.0), rng.uniform(-0.6, 0.6)])
            pose = _drive(twin, pose, *cmd)
        assert car.st[0] == 0.0 and car.st[1] == 0.0 and car.st[2] == 0.0 and car.st[3] == 0.0 and car.steps.value == 40
        assert car.used.value == 40 if case % 3 == 0 else 0 < car.used.value < 40      # (period 1 and no drop: every step)


@pytest.mark.parametrize("d", [1, 3, 7])
def test_exact_through_the_delayed_drive(twin, d):
    """no noise, d = c: the filter reads entry c of the register as K3q left it and est has the bits of the pose on every step"""
    dl = delay_twin.delay()
    N = 5
    rng = np.random.default_rng(303 + d)
    for case in range(3):
        car = TwinCar(twin, _any_estimator(rng, case))
        pose, s = rng.uniform(-2, 2, 3), np.array([1.0])
        q = np.stack([rng.uniform(0.1, 1, DELAY_MAX), rng.uniform(-0.5, 0.5, DELAY_MAX)], 1)
        cc, counter = rng.uniform(0.1, 0.9, 2 * N), C.c_int(0)
        for k in range(30):
            car.step(k, pose, pose, q[d])
            assert _same_bits(car.est, pose), (d, case, k)
            z = rng.uniform(-1, 1, 5 * N + 3)
            z[3 * (N + 1)] = rng.uniform(0.2, 1.0)
            now, u = np.array([rng.uniform(-0.1, 0.1), rng.uniform(-0.3, 0.3), rng.uniform(-3, 3)]), np.zeros(2)
            status = -3 if k in (9, 10) else 1      # (two fallback steps: the fallback entry is queued and later executed)
            assert dl.dl_emu_advance(N, L_CAR, TS, status, _d(z), _d(cc), C.byref(counter), _d(now), d, _d(q), _d(pose), _d(s), _d(u)) == 1
        assert car.st[0] == 0.0 and car.st[3] == 0.0


# ------------------------------------------------------------------------------------------------------ CPU: the schedule
def test_schedule(twin):
    n = 0
    for period in (1, 3, 8):
        for drop in (0.0, 0.3):
            for step0 in (0, 7, -2 ** 40):
                e = Estimator(0, 0, 1, 1, period=period, drop=drop, seed=0xFEDCBA9876543210, car0=3, step0=step0)
                p = e.params(9)
                for k in list(range(-25, 40)) + [2 ** 33, -2 ** 35 + 1]:
                    ref = e.available(k, 9)
                    got = [twin.es_emu_available(_d(np.ascontiguousarray(p[i])), e.seed, 3 + i, k - step0) for i in range(9)]
                    assert got == ref.astype(int).tolist(), (period, drop, step0, k)
                    if drop == 0.0:
                        assert np.all(ref == ((k - step0) % period == 0))
                    n += int(ref.sum())
    assert n > 1000
    # the dropout rate over 4 000 scheduled steps of one car: 0.3 within four standard deviations
    e = Estimator(0, 0, 1, 1, period=1, drop=0.3, seed=5)
    rate = 1.0 - np.mean([e.available(k, 1)[0] for k in range(4000)])
    assert abs(rate - 0.3) < 4 * math.sqrt(0.3 * 0.7 / 4000)
    # period 3, nothing dropped, 30 steps: ten measurements
    car = TwinCar(twin, Estimator(1e-6, 1e-6, 1e-4, 1e-4, period=3))
    for k in range(30):
        car.step(k, np.zeros(3), np.zeros(3), np.zeros(2))
    assert car.used.value == 10 and car.steps.value == 30
    # a car that is not primed takes its measurement on a step that is not scheduled
    e = Estimator(1e-6, 1e-6, 1e-4, 1e-4, p0_xy=0.5, p0_psi=0.25, period=3, step0=-1)
    car = TwinCar(twin, e)
    z = np.array([1.0, 2.0, 3.0])
    assert e.available(0).tolist() == [False] and e.available(1).tolist() == [False] and e.available(2).tolist() == [True]
    assert Estimator(0, 0, 1, 1, period=[1, 2, 3]).available(2).tolist() == [True, True, False]
    assert not e.available(0, 1)[0] and car.step(0, z, np.zeros(3), np.zeros(2)) == 1
    assert _same_bits(car.est, z) and car.cov.tolist() == [0.5, 0.0, 0.0, 0.5, 0.0, 0.25] and car.used.value == 1
    assert car.step(1, z, np.zeros(3), np.zeros(2)) == 0 and car.step(2, z, np.zeros(3), np.zeros(2)) == 1      # j = 2, 3


def test_covariance_stays_a_covariance(twin):
    """2 000 steps with dropouts and a measurement every third step: finite, diagonal >= 0 (the lower triangle is not stored: the
    matrix is symmetric by construction), and the matrix the six entries stand for stays positive semi-definite to rounding"""
    plant = Plant(position_noise=A_XY, heading_noise=A_PSI, seed=12)
    e = Estimator.matched(plant, q_xy=1e-6, q_psi=1e-6, period=3, drop=0.3, seed=9)
    car = TwinCar(twin, e)
    pose, cmd = np.array([0.3, -0.2, 0.4]), np.zeros(2)
    lowest = np.inf
    for k in range(2000):
        car.step(k, plant.measure(k, pose)[0], pose, cmd)
        assert np.all(np.isfinite(car.cov)) and np.all(np.isfinite(car.est))
        assert car.cov[0] >= 0 and car.cov[3] >= 0 and car.cov[5] >= 0
        P = np.zeros((3, 3))
        P[np.triu_indices(3)] = car.cov
        P = P + np.triu(P, 1).T
        lowest = min(lowest, np.linalg.eigvalsh(P)[0] / np.max(np.abs(P)))
        cmd = np.array(_command(k))
        pose = _drive(twin, pose, *cmd)
    assert lowest > -1e-12
    assert 300 < car.used.value < 600 and car.steps.value == 2000


def test_the_filter_filters(twin):
    """the open-loop drive, Estimator.matched, q 1e-6: the position error of the estimate is at most half the measurement's
    (root of the summed squares), over 8 seeds, every step and every third; a numpy restatement gave 0.16 - 0.35"""
    steps = 200
    for period in (1, 3):
        ratios = []
        for seed in range(8):
            plant = Plant(position_noise=A_XY, heading_noise=A_PSI, seed=100 + seed)
            e = Estimator.matched(plant, q_xy=1e-6, q_psi=1e-6, period=period)
            poses, meas, cmds = _open_loop(twin, steps, plant)
            car = TwinCar(twin, e)
            for k in range(steps):
                car.step(k, meas[k], poses[k], cmds[k - 1] if k else np.zeros(2))
            ratios.append(math.sqrt(car.st[1] / car.st[2]))
            assert abs(car.st[2] / steps - 2 * A_XY ** 2 / 6) < 0.3 * 2 * A_XY ** 2 / 6      # (the measurement's variance is the plant's)
        print("period %d: sqrt(err2_sum / meas2_sum) = %s" % (period, np.round(ratios, 3).tolist()))
        assert max(ratios) <= 0.5


# ------------------------------------------------------------------------------------------ CPU: checks and surface
def test_argument_checks(twin):
    def check(B, mb, params, est0=None, cov0=None):
        a = [None if v is None else np.ascontiguousarray(v, float) for v in (params, est0, cov0)]
        return twin.es_emu_check(B, mb, _d(a[0]), _d(a[1]), _d(a[2]))
    B = 3
    assert twin.es_emu_params() == 8 == len(mpmpc.Handle.ESTIMATOR_FIELDS)
    good = Estimator(0.0, 0.0, 1e-4, 1e-4, p0_xy=0.0, p0_psi=0.0, period=4, drop=0.99).params(B)
    assert check(B, 8, good) == 0 and check(B, 8, good, np.ones((B, 3)), np.ones((B, 6))) == 0
    assert check(B, 8, good, np.ones((B, 3)), None) == E_ARG and check(B, 8, good, None, np.ones((B, 6))) == E_ARG
    for car in range(B):      # row by row
        for col, bads in ((0, (-1e-9, np.nan, np.inf)), (1, (-1e-9, np.nan, np.inf)), (2, (0.0, -1.0, np.nan, np.inf)),
                          (3, (0.0, -1.0, np.nan, np.inf)), (4, (-1e-9, np.nan, np.inf)), (5, (-1e-9, np.nan, np.inf)),
                          (6, (0.0, 0.5, 1.5, -1.0, np.nan, np.inf, 2.0 ** 31)), (7, (-0.1, 1.0, 1.5, np.nan))):
            for bad in bads:
                p = good.copy()
                p[car, col] = bad
                assert check(B, 8, p) == E_ARG, (car, col, bad)
        for arr, shape in (("est0", (B, 3)), ("cov0", (B, 6))):
            for bad in (np.nan, np.inf, -np.inf):
                e0, c0 = np.ones((B, 3)), np.ones((B, 6))
                (e0 if arr == "est0" else c0)[car, shape[1] - 1] = bad
                assert check(B, 8, good, e0, c0) == E_ARG
    assert check(0, 8, good) == E_ARG and check(9, 8, np.tile(good[:1], (9, 1))) == E_ARG and check(8, 8, np.tile(good[:1], (8, 1))) == 0
    # Estimator.params: scalars and per-car values, p0 defaults to r
    p = Estimator(1e-6, 2e-6, [1e-4, 2e-4, 3e-4], 4e-4, period=[1, 2, 3], drop=0.1).params(3)
    assert p.shape == (3, 8) and p[:, 2].tolist() == [1e-4, 2e-4, 3e-4] and p[:, 4].tolist() == p[:, 2].tolist() and p[:, 5].tolist() == [4e-4] * 3
    assert p[:, 6].tolist() == [1.0, 2.0, 3.0] and p[:, 7].tolist() == [0.1] * 3 and p[:, 0].tolist() == [1e-6] * 3
    for bad in (dict(r_xy=[1, 2]), dict(period=1.5), dict(period=0), dict(q_xy=np.zeros((3, 1)))):
        kw = dict(q_xy=0, q_psi=0, r_xy=1, r_psi=1)
        kw.update(bad)
        with pytest.raises(ValueError):
            Estimator(**kw).params(3)
    one = Estimator(0, 0, [1.0, 2.0, 3.0], 1, period=[1, 2, 3], seed=7, car0=10, step0=-4).car(2)
    assert one.params(1)[0, 2] == 3.0 and one.params(1)[0, 6] == 3.0 and (one.seed, one.car0, one.step0) == (7, 12, -4)
    # matched: r = A^2 / 6, the variance of the plant's triangular noise (checked against its draws)
    plant = Plant(position_noise=[0.03, 0.06], heading_noise=0.05, seed=3)
    m = Estimator.matched(plant, period=2, drop=0.25, seed=8).params(2)
    assert np.allclose(m[:, 2], [0.03 ** 2 / 6, 0.06 ** 2 / 6], rtol=1e-15) and np.allclose(m[:, 3], 0.05 ** 2 / 6, rtol=1e-15)
    assert m[:, 6].tolist() == [2.0, 2.0] and m[:, 7].tolist() == [0.25, 0.25]
    draws = plant.noise(2, 4000)[:, 0, 2:4]
    assert abs(np.mean(draws ** 2) * 0.03 ** 2 / m[0, 2] - 1.0) < 0.05
    with pytest.raises(ValueError):
        Estimator.matched(Plant(position_noise=0.03))


def test_python_surface():
    from MPC import BatchMPC
    assert "estimator" in inspect.signature(BatchMPC.rollout).parameters
    for name in ("rollout_set_estimator", "rollout_estimator"):
        assert hasattr(mpmpc.Handle, name)
    assert mpmpc.Handle.ESTIMATOR_FIELDS == ("est", "cov", "err2_max", "err2_sum", "meas2_sum", "head2_sum", "used", "steps")
    for name in ("mpmpc_rollout_set_estimator", "mpmpc_rollout_estimator"):
        assert name in mpmpc.EXPORTS
    header = open(T.ROOT + "/include/mpmpc.h").read()
    assert "#define MPMPC_ESTIMATOR_PARAMS 8" in header and "int mpmpc_rollout_set_estimator(" in header
    assert "int mpmpc_rollout_estimator(" in header
    assert set(fresh(2)) == set(mpmpc.Handle.ESTIMATOR_FIELDS) | {"primed"}


def test_batchmpc_refuses_bad_combinations():
    """ValueError before any device call: the stand-in's handle fails on every use"""
    from MPC import BatchMPC

    class NoDevice:
        def __getattr__(self, name):
            raise AssertionError("device call: " + name)
    bm = BatchMPC.__new__(BatchMPC)
    bm._path, bm.corridor_cols, bm.handle = types.SimpleNamespace(), 30, NoDevice()
    e = Estimator(1e-6, 1e-6, 1e-4, 1e-4)
    with pytest.raises(ValueError, match="assumed delay of 8"):
        bm.rollout(np.zeros(2), np.zeros((2, 3)), 1, estimator=e, delay=Delay(8))
    with pytest.raises(ValueError, match="assumed delay of 8"):
        bm.rollout(np.zeros(2), np.zeros((2, 3)), 1, estimator=e, delay=Delay(2, assumed=[1, 8]))
    with pytest.raises(ValueError, match="delay and lookahead"):
        bm.rollout(np.zeros(2), np.zeros((2, 3)), 1, estimator=e, delay=Delay(3), lookahead=types.SimpleNamespace(max_lead=2, traffic=False))
    with pytest.raises(AssertionError, match="device call"):      # (an assumed delay below 8 passes the argument checks)
        bm.rollout(np.zeros(2), np.zeros((2, 3)), 1, estimator=e, delay=Delay(8, assumed=7))


# ------------------------------------------------------------------------------------------------------------ GPU
NOISY = dict(TD.NOISY, position_noise=A_XY, heading_noise=A_PSI)      # test_plant.py's plant with the filter tests' pose noise
_handle, _starts, _equal_states, _in_flight = TD._handle, TD._starts, TD._equal_states, TD._in_flight


def _set(h, e, B, **kw):
    h.rollout_set_estimator(e.params(B), e.seed, e.car0, kw.pop("step0", e.step0), **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("plant", [False, True])
def test_off_changes_nothing(plant):
    """the estimator set and cleared (before the rollout starts, and again between its steps) against a handle that never had
    one: the same bits, with and without a plant"""
    N, B, steps = 10, 64, 20
    _, _, cum = _sim()
    w, s0, poses = _starts(B, 31)
    pl = Plant(seed=99, **NOISY)
    e = Estimator.matched(pl, period=2, drop=0.2, seed=5)
    out = []
    for touched in (False, True):
        h = _handle(N, B)
        if plant:
            h.rollout_set_plant(pl.params(B), pl.seed)
        if touched:
            _set(h, e, B)
            h.rollout_set_estimator(None)
        h.rollout_init(TS, cum, s0, poses)
        h.rollout_step(steps // 2)
        if touched:
            _set(h, e, B)
            h.rollout_set_estimator(None)
            with pytest.raises(mpmpc.MpmpcError):
                h.rollout_estimator()
        h.rollout_step(steps - steps // 2)
        out.append((h.rollout_state(), h.rollout_plant() if plant else None))
        h.close()
    (want, want_pl), (got, got_pl) = out
    _equal_states(got, want)
    if plant:
        for k in mpmpc.Handle.PLANT_FIELDS:
            assert np.array_equal(got_pl[k], want_pl[k]), k
    assert (got["alive"] == 1).sum() > B // 2


def _exact_run(h, B, cum, s0, poses, steps, plant, d, e):
    """-> (state, plant fields, delay fields, the number of (car, step) pairs whose est had the bits of the pose)"""
    if plant is not None:
        h.rollout_set_plant(plant.params(B))
    h.rollout_init(TS, cum, s0, poses)
    if d is not None:
        h.rollout_set_delay(d, d, _in_flight(B))
    if e is not None:
        _set(h, e, B)
    checked = 0
    for k in range(steps):
        before = h.rollout_state()
        h.rollout_step(1)
        if e is not None:
            es = h.rollout_estimator()
            on = before["alive"] == 1
            assert _same_bits(es["est"][on], before["pose"][on]), k
            assert np.all(es["steps"][on] == k + 1) and np.all(es["err2_max"] == 0.0) and np.all(es["head2_sum"] == 0.0)
            assert np.all(es["meas2_sum"] == 0.0)
            checked += int(on.sum())
    return h.rollout_state(), h.rollout_plant() if plant is not None else None, h.rollout_delay() if d is not None else None, checked


@pytest.mark.gpu
@pytest.mark.parametrize("delayed", [False, True])
@pytest.mark.parametrize("plant", [False, True])
def test_exact_on_the_device(plant, delayed):
    """an identity plant (or none) without noise, an estimator with a period and dropouts, no delay or d = c = 2: state, plant
    and delay fields are those of the run without the estimator, and est has the bits of the pose the step found"""
    N, B, steps = 10, 64, 16
    _, _, cum = _sim()
    w, s0, poses = _starts(B, 32, last=160)
    e = Estimator(1e-5, 2e-5, 3e-4, 4e-4, p0_xy=1e-3, p0_psi=2e-3, period=3, drop=0.3, seed=77, car0=4)
    pl = Plant() if plant else None
    d = np.full(B, 2, np.int32) if delayed else None
    out = []
    for est in (None, e):
        h = _handle(N, B)
        out.append(_exact_run(h, B, cum, s0, poses, steps, pl, d, est))
        if est is not None:
            es = h.rollout_estimator()
        h.close()
    (want, want_pl, want_dl, _), (got, got_pl, got_dl, checked) = out
    _equal_states(got, want)
    if plant:
        for k in mpmpc.Handle.PLANT_FIELDS:
            assert np.array_equal(got_pl[k], want_pl[k]), k
    if delayed:
        for k in mpmpc.Handle.DELAY_FIELDS:
            assert _same_bits(got_dl[k], want_dl[k]), k
    on = got["alive"] == 1
    assert on.sum() > B // 2 and checked > steps * B // 2
    assert np.all(es["used"][on] < steps) and np.all(es["used"][on] >= 1) and np.all(es["cov"][on][:, [0, 3, 5]] > 0)
    assert np.all(np.abs(got["pose"][on] - poses[on]).max(axis=1) > 0.1)      # (they drove)


@pytest.mark.gpu
@pytest.mark.parametrize("delayed", [False, True])
def test_exact_on_two_routes(delayed):
    """16 cars, half of them on the second route; d = c = 2 on every car"""
    N, B, steps = 10, 16, 14
    cat, first, circ = TD._two_routes()
    route = (np.arange(B) % 2).astype(np.int32)
    wp = np.where(route == 0, np.arange(B) * 11 % 180, np.arange(B) * 5 % 60).astype(int)
    g = first[route] + wp
    s0, poses = cat["cum_lengths"][g], np.stack([cat["x"][g], cat["y"][g], cat["psi"][g]], 1)
    e = Estimator(1e-5, 2e-5, 3e-4, 4e-4, period=2, drop=0.3, seed=78)
    d = np.full(B, 2, np.int32) if delayed else None
    out = []
    for est in (None, e):
        h = mpmpc.Handle(T.stock_config(N, max_batch=B, circular=False))
        h.set_path(cat["kappa"], cat["v_ref"], cat["ds_next"])
        h.set_corridor(cat["ub"], cat["lb"])
        h.set_routes(first, circ)
        h.set_path_geometry(cat["x"], cat["y"], cat["psi"], cat["border_ub"], cat["border_lb"])
        h.set_car_routes(route)
        out.append(_exact_run(h, B, cat["cum_lengths"], s0, poses, steps, Plant(), d, est))
        h.close()
    (want, want_pl, want_dl, _), (got, got_pl, got_dl, checked) = out
    _equal_states(got, want)
    for k in mpmpc.Handle.PLANT_FIELDS:
        assert np.array_equal(got_pl[k], want_pl[k]), k
    if delayed:
        for k in mpmpc.Handle.DELAY_FIELDS:
            assert _same_bits(got_dl[k], want_dl[k]), k
    on = got["alive"] == 1
    assert on[route == 1].sum() >= 5 and on[route == 0].sum() >= 5 and checked > 100


@pytest.mark.gpu
@pytest.mark.parametrize("delayed", [False, True])
def test_k3e_matches_the_twin_step_by_step(twin, delayed):
    """A noisy plant, one step per call; the twin is fed the device's own measured pose, command (u, or entry c of the register)
    and previous est / cov.  used and steps are equal; est and cov stay within the one-step bound: 1e-14 for the arithmetic both
    sides round alike, plus what the device's cos / sin / tan may differ from the host's by - 4 ulp of a result of magnitude at
    most 1 (cos, sin) or tan(0.66) < 1 - through the time update's coefficients: Ts v (positions), Ts v / L (heading), and, for
    the covariance (entries below 1), twice a = Ts v sin, b = Ts v cos.  Measured on an MI355X (printed below):
    at most 2.2e-16 on est and 1.4e-20 on cov."""
    N, B, steps = 10, 64, 20
    _, _, cum = _sim()
    w, s0, poses = _starts(B, 33, last=160)
    pl = Plant(seed=7, car0=2, **NOISY)
    e = Estimator.matched(pl, period=[1 + i % 3 for i in range(B)], drop=0.25, seed=21, car0=9, step0=-3)
    c = (np.arange(B) % 4).astype(np.int32)
    h = _handle(N, B)
    h.rollout_set_plant(pl.params(B), pl.seed, pl.car0)
    h.rollout_init(TS, cum, s0, poses)
    if delayed:
        h.rollout_set_delay(c, c, _in_flight(B))
    _set(h, e, B)
    prev = fresh(B)
    u_prev, q_prev = np.zeros((B, 2)), _in_flight(B)
    worst = dict(est=0.0, cov=0.0)
    cars = [TwinCar(twin, e.car(i)) for i in range(B)]
    taken = np.zeros(B, int)
    ulp4 = 4 * 2.0 ** -52
    for k in range(steps):
        before = h.rollout_state()
        h.rollout_step(1)
        st, es, meas = h.rollout_state(), h.rollout_estimator(), h.rollout_plant()["meas"]
        on = before["alive"] == 1
        for i in np.flatnonzero(on):
            car = cars[i]
            car.est[:], car.cov[:], car.primed.value = prev["est"][i], prev["cov"][i], int(prev["primed"][i])
            car.st[:] = [prev[f][i] for f in ("err2_max", "err2_sum", "meas2_sum", "head2_sum")]
            car.used.value, car.steps.value = int(prev["used"][i]), int(prev["steps"][i])
            cmd = q_prev[i, c[i]] if delayed else u_prev[i]
            taken[i] += car.step(k, meas[i], before["pose"][i], cmd)
            assert car.used.value == es["used"][i] and car.steps.value == es["steps"][i] == k + 1, (k, i)
            v = abs(cmd[0])
            tol = 1e-14 + ulp4 * TS * v * (1.0 + 1.0 / L_CAR)
            de, dc = np.max(np.abs(car.est - es["est"][i])), np.max(np.abs(car.cov - es["cov"][i]))
            worst["est"], worst["cov"] = max(worst["est"], de), max(worst["cov"], dc)
            assert de <= tol and dc <= 1e-14 + 2 * ulp4 * TS * v, (k, i, de, dc)
            for f, col in (("err2_max", 0), ("err2_sum", 1), ("meas2_sum", 2), ("head2_sum", 3)):
                assert abs(car.st[col] - es[f][i]) <= 1e-14, (k, i, f)
        off = ~on      # a car that is not running keeps what it had
        assert _same_bits(es["est"][off], prev["est"][off]) and np.array_equal(es["steps"][off], prev["steps"][off])
        prev = dict(es, primed=np.where(on, 1, prev["primed"]))
        u_prev = st["u"]
        if delayed:
            q_prev = h.rollout_delay()["queue"]
    h.close()
    print("K3e against the twin, delayed=%s: est %.2e, cov %.2e" % (delayed, worst["est"], worst["cov"]))
    on = st["alive"] == 1
    assert on.sum() > B // 2
    assert np.array_equal(es["used"], taken) and np.all(taken[on] > 1) and (taken[on] < steps).sum() > on.sum() // 2
    avail = np.array([e.available(k, B) for k in range(steps)])      # the schedule and the dropouts are the numpy restatement's
    assert np.array_equal(taken[on], 1 + avail[1:, on].sum(axis=0))


@pytest.mark.gpu
def test_one_call_equals_many_and_a_resumed_run():
    """a noisy plant, per-car delays (d = c and c < d) and the estimator; the resumed run takes est0 / cov0, step0 = -at, the
    plant's act0 and the saved register (which holds the command of the last step)"""
    N, B, steps, at = 10, 64, 24, 10
    _, _, cum = _sim()
    w, s0, poses = _starts(B, 34, last=160)
    plant = Plant(seed=4242, car0=5, **NOISY)
    e = Estimator.matched(plant, period=2, drop=0.2, seed=17, car0=3)
    d = (np.arange(B) % 4).astype(np.int32)
    c = np.where(np.arange(B) % 8 < 4, d, np.maximum(d - 1, 0)).astype(np.int32)
    h = _handle(N, B, warm=False)
    h.rollout_set_plant(plant.params(B), plant.seed, plant.car0)

    def start():
        h.rollout_init(TS, cum, s0, poses)
        h.rollout_set_delay(d, c, _in_flight(B))
    start()
    _set(h, e, B)
    h.rollout_step(steps)
    want, want_pl, want_dl, want_es = h.rollout_state(), h.rollout_plant(), h.rollout_delay(), h.rollout_estimator()
    start()      # (rollout_init un-primes the cars and zeroes the statistics; the parameters stay)
    for t in range(steps):
        if t == at:
            saved, saved_pl, saved_dl, saved_es = h.rollout_state(), h.rollout_plant(), h.rollout_delay(), h.rollout_estimator()
        h.rollout_step(1)
    got, got_pl, got_dl, got_es = h.rollout_state(), h.rollout_plant(), h.rollout_delay(), h.rollout_estimator()
    _equal_states(got, want)
    for k in mpmpc.Handle.PLANT_FIELDS:
        assert np.array_equal(got_pl[k], want_pl[k]), k
    for k in mpmpc.Handle.DELAY_FIELDS:
        assert _same_bits(got_dl[k], want_dl[k]), k
    for k in mpmpc.Handle.ESTIMATOR_FIELDS:
        assert np.array_equal(got_es[k], want_es[k]) if got_es[k].dtype.kind == "i" else _same_bits(got_es[k], want_es[k]), k
    # resumed from the save
    h.rollout_init(TS, cum, saved["s"], saved["pose"], saved["cc"])
    h.rollout_set_counters(saved["counter"])
    h.rollout_set_plant(plant.params(B), plant.seed, plant.car0, step0=-at, act0=saved_pl["act"])
    h.rollout_set_delay(d, c, saved_dl["queue"])
    _set(h, e, B, step0=-at, est0=saved_es["est"], cov0=saved_es["cov"])
    h.rollout_step(steps - at)
    res, res_pl, res_dl, res_es = h.rollout_state(), h.rollout_plant(), h.rollout_delay(), h.rollout_estimator()
    h.close()
    on = saved["alive"] == 1      # (a resumed run starts every car alive: the cars that were running at the save are compared)
    assert on.sum() > B // 4 and (want["alive"] == 1)[on].sum() > B // 4
    _equal_states({k: res[k][on] for k in KEYS}, {k: want[k][on] for k in KEYS})
    assert _same_bits(res_pl["act"][on], want_pl["act"][on]) and _same_bits(res_pl["meas"][on], want_pl["meas"][on])
    for k in mpmpc.Handle.DELAY_FIELDS:
        assert _same_bits(res_dl[k][on], want_dl[k][on]), k
    assert _same_bits(res_es["est"][on], want_es["est"][on]) and _same_bits(res_es["cov"][on], want_es["cov"][on])
    still = on & (want["alive"] == 1)      # the statistics start over with the resumed run
    assert np.all(res_es["steps"][still] == steps - at) and np.all(want_es["steps"][still] == steps)
    assert not _same_bits(want_es["est"], want_pl["meas"])


def _host_loop(N, starts, plant, est, delay, steps):
    """the reference's loop with the project's host classes, one car at a time, around Estimator.apply"""
    g1, _, cum = _sim()
    lap = TD._lap()
    rows, statuses = [], []
    for i, w in enumerate(starts):
        m, rp, car = T.build_world(obstacles=False)
        mpc = T.make_mpc(car, N)
        one_p, one_e = plant.car(i), est.car(i)
        one_d = None if delay is None else delay.car(i)
        st = dict(pose=np.array([[rp.waypoints[w].x, rp.waypoints[w].y, rp.waypoints[w].psi]]), s=np.array([float(cum[w])]),
                  act=np.zeros((1, 2)), queue=None if one_d is None else one_d.queue(1), state=fresh(1), u=np.zeros((1, 2)))

        def control(pose_in, s_in=None):
            car.s = float(st["s"][0]) if s_in is None else float(s_in[0])
            car.temporal_state = TemporalState(*pose_in[0])
            u = mpc.get_control()
            statuses.append(mpc.last_status)
            if s_in is not None:
                return u
            return u, [[car.spatial_state.e_y, car.spatial_state.e_psi]], [car.current_waypoint.kappa]
        for k in range(steps):
            st = one_e.apply(k, st["pose"], st["s"], st["state"], st["u"], control, car.length, car.Ts, plant=one_p, act=st["act"],
                             delay=one_d, queue=st["queue"], path=lap)
        ss = st["state"]
        rows.append(np.concatenate([st["s"], st["pose"][0], st["est"][0], st["u"][0], ss["cov"][0],
                                    [ss["err2_sum"][0], ss["meas2_sum"][0], float(ss["used"][0])]]))
    return np.array(rows), statuses


@pytest.mark.gpu
@pytest.mark.parametrize("N", [10, 30])
@pytest.mark.parametrize("case", ["none", "a"])
def test_closed_loop_matches_the_host_loop(case, N):
    """test_delay.py's CLOSED_LOOP starts under a noisy plant: (none) no delay, test_plant.py's plant (gains, offset, wheelbase,
    lags, rate limit, command noise) with the filter tests' pose noise of 3 cm and 0.05 rad; (a) d = c per car, that pose noise
    alone - under a delay the mismatched plant makes the host controller infeasible on some steps, which the assertion on the
    statuses rules out.  Bounds s, pose, est 1e-8 and u 1e-6 (test_plant.py's).  Measured on an MI355X (printed below; DESIGN.md,
    K3e): at most 4.4e-15 on s, pose and est and 4.5e-14 on u, both at (none), N = 30."""
    g1, _, cum = _sim()
    steps = 25
    starts, d, _ = TD.CLOSED_LOOP["a"]
    starts = np.array(starts)
    B = starts.size
    plant = Plant(seed=12345, **(dict(position_noise=A_XY, heading_noise=A_PSI) if case == "a" else NOISY))
    est = Estimator.matched(plant, period=2, drop=0.2, seed=6)
    delay = Delay(d, queue0=_in_flight(B)) if case == "a" else None
    host, statuses = _host_loop(N, starts, plant, est, delay, steps)
    assert all(v == 1 for v in statuses), statuses      # the comparison must not cross a verdict boundary
    h = _handle(N, B)
    h.rollout_set_plant(plant.params(B), plant.seed)
    poses = np.stack([g1["x"][starts], g1["y"][starts], g1["psi"][starts]], axis=1)
    h.rollout_init(TS, cum, cum[starts], poses)
    if delay is not None:
        h.rollout_set_delay(*delay.arrays(B))
    _set(h, est, B)
    h.rollout_step(steps)
    st, es = h.rollout_state(), h.rollout_estimator()
    h.close()
    figures = dict(s=np.max(np.abs(st["s"] - host[:, 0])), pose=np.max(np.abs(st["pose"] - host[:, 1:4])),
                   est=np.max(np.abs(es["est"] - host[:, 4:7])), u=np.max(np.abs(st["u"] - host[:, 7:9])),
                   cov=np.max(np.abs(es["cov"] - host[:, 9:15])), err2_sum=np.max(np.abs(es["err2_sum"] - host[:, 15])))
    print("estimator closed loop (%s) N=%d:" % (case, N), figures)
    assert np.all(st["alive"] == 1) and np.array_equal(es["used"], host[:, 17].astype(int)) and np.all(es["steps"] == steps)
    assert figures["s"] <= 1e-8 and figures["pose"] <= 1e-8 and figures["est"] <= 1e-8 and figures["u"] <= 1e-6
    assert figures["cov"] <= 1e-8 and figures["err2_sum"] <= 1e-8


HELPS = dict(N=10, B=64, steps=40, seed=35, plant_seed=555)


def _helps_inputs():
    B = HELPS["B"]
    w, s0, poses = _starts(B, HELPS["seed"], last=150)
    plant = Plant(seed=HELPS["plant_seed"], position_noise=A_XY, heading_noise=A_PSI)      # the noise alone: 3 cm, 0.05 rad
    return w, s0, poses, plant, Estimator.matched(plant)


@pytest.mark.gpu
def test_the_estimator_helps():
    """64 cars, 40 steps, the same plant (pose noise of 3 cm and 0.05 rad, nothing else) and seeds with Estimator.matched and
    without: the fleet's summed squared lateral error is lower with the estimator and every car's estimate is closer to the
    true position than its measurements were (err2_sum < meas2_sum).  No ratio is fixed.  That these inputs satisfy both
    inequalities was checked beforehand with the host loop on the CPU emulation (profiles/estimator/README.md: 0.705 against
    0.891 m^2, worst err2_sum / meas2_sum 0.26).  Measured on an MI355X (printed below): ey_sq 0.705 against 0.891 m^2, every car
    driven on all 40 steps in both fleets, sqrt(err2_sum / meas2_sum) 0.22 .. 0.51."""
    N, B, steps = HELPS["N"], HELPS["B"], HELPS["steps"]
    _, _, cum = _sim()
    w, s0, poses, plant, est = _helps_inputs()
    out = {}
    for name, e in (("with", est), ("without", None)):
        h = _handle(N, B)
        h.rollout_set_plant(plant.params(B), plant.seed)
        h.rollout_init(TS, cum, s0, poses)
        if e is not None:
            _set(h, e, B)
        h.rollout_step(steps)
        out[name] = (h.rollout_state(), h.rollout_plant(), h.rollout_estimator() if e is not None else None)
        h.close()
    (st1, pl1, es), (st0, pl0, _) = out["with"], out["without"]
    print("summed ey_sq with %.4e, without %.4e; alive with %d, without %d; sqrt(err2_sum / meas2_sum) %.3f .. %.3f" %
          (pl1["ey_sq"].sum(), pl0["ey_sq"].sum(), (st1["alive"] == 1).sum(), (st0["alive"] == 1).sum(),
           np.sqrt(es["err2_sum"] / es["meas2_sum"]).min(), np.sqrt(es["err2_sum"] / es["meas2_sum"]).max()))
    assert np.all(pl1["steps"] == steps) and np.all(pl0["steps"] == steps)      # every car was driven on every step, in both fleets
    assert pl1["ey_sq"].sum() < pl0["ey_sq"].sum()
    assert np.all(es["err2_sum"] < es["meas2_sum"]) and np.all(es["used"] == steps)


@pytest.mark.gpu
def test_state_and_argument_errors():
    N, B = 10, 8
    g1, _, cum = _sim()
    w, s0, poses = _starts(B, 36, last=160)
    e = Estimator(1e-6, 1e-6, 1e-4, 1e-4, period=2, drop=0.1, seed=3)
    good = e.params(B)
    h = _handle(N, B, warm=False)
    h.rollout_init(TS, cum, s0, poses)
    with pytest.raises(mpmpc.MpmpcError) as err:
        h.rollout_estimator()      # no estimator
    assert _code(err) == E_STATE
    _set(h, e, B)
    with pytest.raises(mpmpc.MpmpcError) as err:
        h.rollout_estimator()      # no step under it yet
    assert _code(err) == E_STATE
    h.rollout_step(3)
    h.rollout_step(3)
    want, want_es = h.rollout_state(), h.rollout_estimator()
    # a refused call leaves the running setting's next step unchanged
    h.rollout_init(TS, cum, s0, poses)
    h.rollout_step(3)
    for col, bad in ((0, np.nan), (1, -1.0), (2, 0.0), (3, -1e-3), (2, np.inf), (4, np.nan), (6, 0.0), (6, 2.5), (7, 1.0), (7, -0.5)):
        p = good.copy()
        p[B - 1, col] = bad
        with pytest.raises(mpmpc.MpmpcError) as err:
            h.rollout_set_estimator(p)
        assert _code(err) == E_ARG, (col, bad)
    for kw in (dict(est0=np.zeros((B, 3))), dict(cov0=np.zeros((B, 6)))):      # one without the other
        with pytest.raises(mpmpc.MpmpcError) as err:
            h.rollout_set_estimator(good, **kw)
        assert _code(err) == E_ARG
    e0 = np.zeros((B, 3))
    e0[B - 1, 2] = np.nan
    with pytest.raises(mpmpc.MpmpcError) as err:
        h.rollout_set_estimator(good, est0=e0, cov0=np.zeros((B, 6)))
    assert _code(err) == E_ARG
    with pytest.raises(mpmpc.MpmpcError) as err:
        h.rollout_set_estimator(np.tile(good[:1], (B + 1, 1)))      # more than max_batch
    assert _code(err) == E_ARG
    h.rollout_step(3)
    got, got_es = h.rollout_state(), h.rollout_estimator()
    _equal_states(got, want)
    for k in mpmpc.Handle.ESTIMATOR_FIELDS:
        assert np.array_equal(got_es[k], want_es[k]), k
    # an assumed delay of 8: refused with both settings named, and the step runs once either is changed
    h.rollout_set_delay(np.full(B, 8, np.int32))
    with pytest.raises(mpmpc.MpmpcError) as err:
        h.rollout_step(1)
    assert _code(err) == E_STATE and "mpmpc_rollout_set_estimator" in str(err.value) and "mpmpc_rollout_set_delay" in str(err.value)
    a = np.full(B, 7, np.int32)
    a[B - 1] = 8
    h.rollout_set_delay(np.full(B, 8, np.int32), a)
    with pytest.raises(mpmpc.MpmpcError) as err:
        h.rollout_step(1)
    assert _code(err) == E_STATE
    h.rollout_set_delay(np.full(B, 8, np.int32), np.full(B, 7, np.int32))
    h.rollout_step(1)
    h.rollout_set_delay(None)
    h.rollout_step(1)
    # a step of another B
    h.rollout_init(TS, cum, s0[:5], poses[:5])
    with pytest.raises(mpmpc.MpmpcError) as err:
        h.rollout_step(1)
    assert _code(err) == E_STATE
    h.rollout_set_estimator(None)
    h.rollout_step(1)      # without an estimator: any B the rollout holds
    with pytest.raises(mpmpc.MpmpcError) as err:
        h.rollout_estimator()
    assert _code(err) == E_STATE
    h.close()


@pytest.mark.gpu
def test_batchmpc_rollout_takes_an_estimator():
    """BatchMPC.rollout(..., estimator=...) returns "estimator"; with plant, delay, audit and record their outputs stay in place;
    a following rollout without it is bit-equal to a controller that never had one"""
    from MPC import BatchMPC
    from footprint import Footprint
    from scipy import sparse
    m, rp, car = T.build_world(obstacles=False)
    Q, R, QN = sparse.diags([1.0, 0.0, 0.0]), sparse.diags([0.5, 0.0]), sparse.diags([1.0, 0.0, 0.0])
    ic = {'umin': np.array([0.0, -np.tan(0.66) / car.length]), 'umax': np.array([1.0, np.tan(0.66) / car.length])}
    sc = {'xmin': np.array([-np.inf] * 3), 'xmax': np.array([np.inf] * 3)}
    B, N, steps = 8, 10, 12
    w, s0, poses = _starts(B, 37, last=160)
    plant = Plant(seed=8, position_noise=A_XY, heading_noise=A_PSI)
    est = Estimator.matched(plant, period=2)

    def make():
        return BatchMPC(car, N, Q, R, QN, sc, ic, 4.0, max_batch=B, corridor="device")
    fresh_bm = make()
    plain = fresh_bm.rollout(s0, poses, steps)
    fresh_bm.close()
    assert "estimator" not in plain
    bm = make()
    out = bm.rollout(s0, poses, steps, estimator=est)      # the estimator alone: it filters the true pose
    es = out.pop("estimator")
    assert set(es) == set(mpmpc.Handle.ESTIMATOR_FIELDS) and es["est"].shape == (B, 3) and es["cov"].shape == (B, 6)
    assert np.all(es["steps"] == steps) and np.all(es["used"] == steps // 2) and np.all(es["meas2_sum"] == 0.0)
    _equal_states(out, plain)      # (nothing to estimate: the rollout without it)
    out = bm.rollout(s0, poses, steps, estimator=est, plant=plant, delay=Delay(2, queue0=_in_flight(B)), audit=Footprint(0.12, 0.06),
                     record=True)
    assert set(out["estimator"]) == set(mpmpc.Handle.ESTIMATOR_FIELDS)
    assert set(out["plant"]) == set(mpmpc.Handle.PLANT_FIELDS) and set(out["delay"]) == set(mpmpc.Handle.DELAY_FIELDS)
    assert set(out["audit"]) >= set(mpmpc.Handle.AUDIT_FIELDS) and out["trace"]["pose"].shape[:2] == (steps, B)
    on = out["alive"] == 1
    assert on.sum() >= B // 2 and np.all(out["estimator"]["err2_sum"][on] < out["estimator"]["meas2_sum"][on])
    assert not _same_bits(out["estimator"]["est"][on], out["plant"]["meas"][on])
    assert bm.rollout(s0, poses, 0, estimator=est)["estimator"] is None
    again = bm.rollout(s0, poses, steps)      # off again
    _equal_states(again, plain)
    with pytest.raises(mpmpc.MpmpcError):
        bm.handle.rollout_estimator()
    bm.close()
