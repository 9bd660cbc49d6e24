"""Plant models in the device rollout (K3n / K3p, mpmpc_rollout_set_plant): per-car mismatch, actuator lag and reproducible
noise; the true pose and the pose the controller localises on separate.

CPU: the host twin (tests/emul_plant, the same plant_core.hpp) against Philox4x32-10's known answers, against a restatement of
the draws written here from the header's text and against the product's numpy (plant.Plant); pl_drive / pl_measure against
Plant.drive / Plant.measure and - the command, the counter, the ending, an identity plant - against emu_advance; the argument
checks.  GPU: mpmpc_plant_noise, an identity plant against no plant, one call against many and a resumed run, the closed loop
against the host loop of the project's host classes around Plant.apply, the consumers of the true pose, the error codes."""
import ctypes as C
import math

import numpy as np
import pytest

import mpc_np as M
import mpmpc
import mpmpc_testlib as T
import scenarios
import twins
from plant import IDENTITY, NAMES, Plant
from spatial_bicycle_models import TemporalState, t2s_batch

lp, up = C.POINTER(C.c_int64), C.POINTER(C.c_uint32)
E_ARG, E_STATE = -1, -3
TS, L_CAR = 0.05, 0.12
KEYS = ("s", "pose", "cc", "wp_id", "x0", "u", "status", "counter", "alive")
# the plant of the closed-loop tests
NOISY = dict(speed_gain=0.97, steer_gain=1.03, steer_offset=0.01, wheelbase_scale=1.03, speed_lag=0.8, steer_lag=0.8, steer_rate=0.3,
             speed_noise=0.02, steer_noise=0.01, position_noise=0.002, heading_noise=0.005)


_d = T._d


@pytest.fixture(scope="module")
def twin():
    """The CPU twin of K3n / K3p (tests/emul_plant)."""
    return twins.plant()


# ------------------------------------------------------------------------- the draws, restated from the header's text
def _philox(ctr, key):
    """Philox4x32-10 on python ints: ctr 4 words, key 2 words -> 4 words"""
    c, k = list(ctr), list(key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


def _variate(w):
    return float((w >> 16) + (w & 0xFFFF) - 65535) * 2.0 ** -16


def _draws(seed, car0, B, js):
    """[len(js), B, 5] = n_v, n_delta, n_x, n_y, n_psi"""
    out = np.zeros((len(js), B, 5))
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    for t, j in enumerate(js):
        ju = int(j) & 0xFFFFFFFFFFFFFFFF
        for i in range(B):
            head = [(car0 + i) & 0xFFFFFFFF, ju & 0xFFFFFFFF, ju >> 32]
            out[t, i, :4] = [_variate(w) for w in _philox(head + [0], key)]
            out[t, i, 4] = _variate(_philox(head + [1], key)[0])
    return out


def _twin_draws(twin, seed, car0, B, js):
    j = np.ascontiguousarray([int(v) for v in js], np.int64)
    out = np.full((j.size, B, 5), 7.0)
    twin.pl_emu_noise(seed, car0, B, j.size, j.ctypes.data_as(lp), _d(out))
    return out


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, float), np.ascontiguousarray(b, float)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def test_philox_known_answers(twin):
    import plant
    for ctr, key, want in KAT:
        assert tuple(_philox(ctr, key)) == want
        c, k, out = np.array(ctr, np.uint32), np.array(key, np.uint32), np.zeros(4, np.uint32)
        twin.pl_emu_philox(k.ctypes.data_as(up), c.ctypes.data_as(up), out.ctypes.data_as(up))
        assert tuple(int(v) for v in out) == want
        assert tuple(int(v) for v in plant.philox4x32(np.array(ctr, np.uint64), np.array(key, np.uint64))) == want


DRAW_CASES = [(0, 0), (12345, 0), ((1 << 32) + 5, 0), (0xDEADBEEFCAFEF00D, 0), (12345, 1000), ((1 << 40) + 9, 4000000000)]


@pytest.mark.parametrize("seed,car0", DRAW_CASES)
def test_draws_agree_bit_for_bit(twin, seed, car0):
    js = list(range(-3, 4)) + [2 ** 32 - 1, 2 ** 32]
    want = _draws(seed, car0, 5, js)
    assert _same_bits(_twin_draws(twin, seed, car0 - (1 << 32) if car0 >= 1 << 31 else car0, 5, js), want)
    assert _same_bits(Plant(seed=seed, car0=car0).noise(5, js), want)
    step0 = 17      # step indices k with a step0: j = k - step0
    assert _same_bits(Plant(seed=seed, car0=car0, step0=step0).noise(5, [j + step0 for j in js]), want)
    assert len({tuple(r) for r in want.reshape(-1, 5)}) == want.size // 5      # (no two (car, step) rows alike)


def test_a_draw_does_not_depend_on_the_batch(twin):
    seed, js = 987654321, [-2, 0, 5]
    fleet = _twin_draws(twin, seed, 3, 300, js)
    assert _same_bits(fleet, Plant(seed=seed, car0=3).noise(300, js))
    for i in (0, 1, 63, 64, 255, 256, 299):
        assert _same_bits(fleet[:, i:i + 1], _twin_draws(twin, seed, 3 + i, 1, js))
        assert _same_bits(fleet[:, i:i + 1], _draws(seed, 3 + i, 1, js))
    assert _same_bits(Plant(seed=seed).noise(4, 3), Plant(seed=seed).noise(4, [0, 1, 2]))      # an int: steps 0 .. n - 1


def test_draw_statistics(twin):
    t = _twin_draws(twin, 2024, 0, 1000, range(20)).reshape(-1)      # 10^5 draws
    assert t.size == 100000
    assert abs(t.mean()) < 0.01 and abs(t.std() * math.sqrt(6.0) - 1.0) < 0.01      # (standard error of the mean: 0.0013)
    assert np.max(np.abs(t)) <= 65535.0 / 65536.0
    assert np.array_equal(t * 65536.0, np.round(t * 65536.0))      # integers over 2^16


# ------------------------------------------------------------------------------------------ pl_drive / pl_measure
def _drive_cases():
    """teacher-forced random states at N = 5: (params [11], status, counter, z, cc, x0, kappa, pose, s, act, k) per case"""
    rng = np.random.default_rng(77)
    N, cases = 5, []
    for c in range(600):
        p = np.array(IDENTITY)
        p[0], p[1], p[2], p[3] = rng.uniform(0.8, 1.2), rng.uniform(0.8, 1.2), rng.uniform(-0.05, 0.05), rng.uniform(0.9, 1.1)
        p[4] = 1.0 if c % 2 == 0 else rng.uniform(0.05, 0.999)
        p[5] = 1.0 if (c // 2) % 2 == 0 else rng.uniform(0.05, 0.999)
        p[6] = (np.inf, 10.0, rng.uniform(0.005, 0.05))[c % 3]
        p[7:] = rng.uniform(0.0, 0.05, 4)
        status = 1 if c % 5 < 3 else -3
        counter = int(rng.integers(0, N - 1))      # 0 .. N - 2: a fallback step at N - 2 ends the run
        cases.append(dict(p=p, status=status, counter=counter, z=rng.uniform(-1, 1, 5 * N + 3), cc=rng.uniform(-0.6, 0.9, 2 * N),
                          x0=np.array([rng.uniform(-0.1, 0.1), rng.uniform(-0.3, 0.3), 0.0]), kappa=rng.uniform(-3, 3),
                          pose=rng.uniform(-3, 3, 3), s=rng.uniform(0, 20), act=np.array([rng.uniform(0, 1), rng.uniform(-0.5, 0.5)]),
                          k=int(rng.integers(-5, 1000)), seed=int(rng.integers(0, 2 ** 63)), car=int(rng.integers(0, 5000))))
    return N, cases


def _twin_advance(twin, N, c, p, n5):
    cc, pose, act, u = c["cc"].copy(), c["pose"].copy(), c["act"].copy(), np.zeros(2)
    counter, s = C.c_int(c["counter"]), np.array([c["s"]])
    alive = twin.pl_emu_advance(N, L_CAR, TS, c["status"], _d(c["z"]), _d(cc), C.byref(counter), _d(c["x0"]), c["kappa"],
                                _d(np.ascontiguousarray(p)), _d(np.ascontiguousarray(n5)), _d(act), _d(pose), _d(s), _d(u))
    return dict(alive=alive, cc=cc, pose=pose, act=act, u=u, counter=counter.value, s=s[0])


def _emu_advance(emu, N, c):
    cc, pose, u = c["cc"].copy(), c["pose"].copy(), np.zeros(2)
    counter, s = C.c_int(c["counter"]), C.c_double(c["s"])
    alive = emu.lib.emu_advance(C.c_int(N), C.c_double(L_CAR), C.c_double(TS), C.c_int(c["status"]), _d(c["z"]), _d(cc), C.byref(counter),
                                _d(c["x0"]), C.c_double(c["kappa"]), _d(pose), C.byref(s), _d(u))
    return dict(alive=alive, cc=cc, pose=pose, u=u, counter=counter.value, s=s.value)


def test_drive_and_measure_match_plant_apply(twin, emu):
    N, cases = _drive_cases()
    seen = set()
    for c in cases:
        pl = Plant(*c["p"], seed=c["seed"], car0=c["car"])
        n5 = pl.noise(1, [c["k"]])[0, 0]
        got, ref = _twin_advance(twin, N, c, c["p"], n5), _emu_advance(emu, N, c)
        # the command, the counter, the plan and the N - 1 ending are emu_advance's
        assert got["alive"] == ref["alive"] and got["counter"] == ref["counter"]
        assert _same_bits(got["u"], ref["u"]) and _same_bits(got["cc"], ref["cc"])
        fallback = c["status"] != 1
        if fallback:
            assert _same_bits(got["u"], c["cc"][2 * (c["counter"] + 1):2 * (c["counter"] + 1) + 2])
        meas = np.zeros(3)
        twin.pl_emu_measure(_d(np.ascontiguousarray(c["p"])), _d(np.ascontiguousarray(n5)), _d(c["pose"]), _d(meas))
        assert _same_bits(meas, pl.measure(c["k"], c["pose"])[0])
        if not got["alive"]:      # the run ends: nothing of the plant moves
            assert fallback and c["counter"] == N - 2
            assert _same_bits(got["pose"], c["pose"]) and got["s"] == c["s"] and _same_bits(got["act"], c["act"])
            seen.add("ended")
            continue
        pose, s, act = pl.drive(c["k"], got["u"], c["pose"], c["s"], c["act"], c["x0"], c["kappa"], L_CAR, TS)
        assert _same_bits(got["act"], act[0])
        assert np.max(np.abs(got["pose"] - pose[0])) <= 1e-14 and abs(got["s"] - s[0]) <= 1e-14
        # which way every select went
        v_t = c["p"][0] * got["u"][0] + c["p"][7] * n5[0]
        d_t = (c["p"][1] * got["u"][1] + c["p"][2]) + c["p"][8] * n5[1]
        d_new = d_t if c["p"][5] == 1.0 else c["act"][1] + c["p"][5] * (d_t - c["act"][1])
        binding = abs(d_new - c["act"][1]) > c["p"][6]
        if binding:
            assert abs(abs(got["act"][1] - c["act"][1]) - c["p"][6]) <= 1e-15
        if c["p"][4] == 1.0:
            assert got["act"][0] == v_t
        seen.add(("fallback" if fallback else "solved", "counter %d" % c["counter"] if fallback else "", c["p"][4] == 1.0,
                  c["p"][5] == 1.0, "inf" if np.isinf(c["p"][6]) else ("binds" if binding else "slack")))
    assert "ended" in seen
    for fb in [("solved", "")] + [("fallback", "counter %d" % q) for q in range(N - 2)]:
        for key in ("av", "ad"):
            for one in (True, False):
                assert any(t[:2] == fb and t[2 if key == "av" else 3] == one for t in seen if t != "ended"), (fb, key, one)
        for rate in ("inf", "binds", "slack"):
            assert any(t[:2] == fb and t[4] == rate for t in seen if t != "ended"), (fb, rate)


def test_identity_plant_is_emu_advance(twin, emu):
    N, cases = _drive_cases()
    ident = np.array(IDENTITY)
    for c in cases:
        n5 = Plant(seed=c["seed"], car0=c["car"]).noise(1, [c["k"]])[0, 0]      # (drawn, and multiplied by zero)
        got, ref = _twin_advance(twin, N, c, ident, n5), _emu_advance(emu, N, c)
        assert got["alive"] == ref["alive"] and got["counter"] == ref["counter"]
        for k in ("u", "cc", "pose"):
            assert _same_bits(got[k], ref[k]), k
        assert got["s"] == ref["s"]
        if got["alive"]:
            assert _same_bits(got["act"], got["u"])      # executed = commanded
        meas = np.zeros(3)
        twin.pl_emu_measure(_d(ident), _d(np.ascontiguousarray(n5)), _d(c["pose"]), _d(meas))
        assert _same_bits(meas, c["pose"])


def test_statistics_accumulate_in_step_order(twin):
    rng = np.random.default_rng(5)
    ey_max, ey_sq, steps = np.zeros(1), np.zeros(1), C.c_int(0)
    want_max, want_sq = 0.0, 0.0
    for _ in range(50):
        x, y, wx, wy, a = (float(v) for v in rng.uniform(-2, 2, 5))
        twin.pl_emu_stats(x, y, wx, wy, math.cos(a), math.sin(a), _d(ey_max), _d(ey_sq), C.byref(steps))
        e = math.cos(a) * (y - wy) - math.sin(a) * (x - wx)
        want_max, want_sq = max(want_max, abs(e)), want_sq + e * e
    assert ey_max[0] == want_max and ey_sq[0] == want_sq and steps.value == 50


# the parameter table: (column, values that must be refused, values that must pass)
NAN, INF = float("nan"), float("inf")
TABLE = [(0, [NAN, INF, -INF], [0.0, -1.0, 3.0]), (1, [NAN, INF, -INF], [0.0, -1.0, 3.0]), (2, [NAN, INF, -INF], [-0.5, 0.5]),
         (3, [NAN, 0.0, -1.0, INF], [0.5, 2.0]), (4, [NAN, 0.0, -0.1, 1.0000001, INF], [1.0, 1e-6]),
         (5, [NAN, 0.0, -0.1, 1.0000001, INF], [1.0, 1e-6]), (6, [NAN, 0.0, -1.0, -INF], [INF, 1e-9]),
         (7, [NAN, -1e-9, INF], [0.0, 2.0]), (8, [NAN, -1e-9, INF], [0.0, 2.0]), (9, [NAN, -1e-9, INF], [0.0, 2.0]),
         (10, [NAN, -1e-9, INF], [0.0, 2.0])]


def _check(twin, B, max_batch, params, act0=None):
    p = np.ascontiguousarray(params, float)
    return twin.pl_emu_check(B, max_batch, _d(p), _d(None if act0 is None else np.ascontiguousarray(act0, float)))


def test_argument_checks(twin):
    B = 3
    ident = np.tile(np.array(IDENTITY), (B, 1))
    assert len(TABLE) == len(NAMES) == ident.shape[1] == 11
    assert _check(twin, B, 8, ident) == 0
    assert np.array_equal(Plant().params(B), ident)
    for col, bad, good in TABLE:
        for car in (0, B - 1):
            for v in bad:
                p = ident.copy()
                p[car, col] = v
                assert _check(twin, B, 8, p) == E_ARG, (NAMES[col], v)
            for v in good:
                p = ident.copy()
                p[car, col] = v
                assert _check(twin, B, 8, p) == 0, (NAMES[col], v)
    assert _check(twin, 0, 8, ident) == E_ARG and _check(twin, 9, 8, np.tile(np.array(IDENTITY), (9, 1))) == E_ARG
    assert _check(twin, B, 8, ident, np.zeros((B, 2))) == 0
    for v in (NAN, INF):
        a = np.zeros((B, 2))
        a[1, 1] = v
        assert _check(twin, B, 8, ident, a) == E_ARG
    # per-car values and scalars in Plant.params
    p = Plant(speed_gain=[0.9, 1.0, 1.1], steer_rate=0.2).params(3)
    assert p[:, 0].tolist() == [0.9, 1.0, 1.1] and p[:, 6].tolist() == [0.2] * 3
    with pytest.raises(ValueError):
        Plant(speed_gain=[0.9, 1.0]).params(3)
    one = Plant(speed_gain=[0.9, 1.0, 1.1], seed=4, car0=10).car(2)
    assert one.params(1)[0, 0] == 1.1 and one.car0 == 12 and one.seed == 4


def test_python_surface():
    from MPC import BatchMPC
    import inspect
    assert "plant" in inspect.signature(BatchMPC.rollout).parameters
    for name in ("rollout_set_plant", "rollout_plant"):
        assert hasattr(mpmpc.Handle, name)
    assert hasattr(mpmpc, "plant_noise")
    for name in ("mpmpc_rollout_set_plant", "mpmpc_rollout_plant", "mpmpc_plant_noise"):
        assert name in mpmpc.EXPORTS


# ------------------------------------------------------------------------------------------------------------ GPU
def _sim():
    g1 = np.load(M.GOLDEN + "/g1_path_sim_track.npz")
    g3 = np.load(M.GOLDEN + "/g3_corridor.npz")
    return g1, g3, np.cumsum(g1["segment_lengths"])


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
    """cars on waypoints below `last` (a car near the end of the lap finishes it within 25 steps: alive = 0)"""
    g1, _, cum = _sim()
    w = np.random.default_rng(seed).integers(0, last, B)
    return w, cum[w], np.stack([g1["x"][w], g1["y"][w], g1["psi"][w]], axis=1)


def _equal_states(a, b):
    for k in KEYS:
        same = np.array_equal(a[k], b[k]) if a[k].dtype.kind == "i" else _same_bits(a[k], b[k])
        assert same, k


def _code(err):
    return int(str(err.value).split("mpmpc error ")[1].split(":")[0])


@pytest.mark.gpu
def test_plant_noise_on_the_device():
    seed, car0, B, n, j0 = (1 << 35) + 77, 40, 300, 3, -1      # (300 cars: more than one block of 256 threads)
    got = mpmpc.plant_noise(seed, car0, B, j0, n)
    assert _same_bits(got, _draws(seed, car0, B, [j0 + t for t in range(n)]))
    assert _same_bits(got, Plant(seed=seed, car0=car0, step0=1).noise(B, n))      # steps 0 .. 2 at step0 = 1: j = -1 .. 1


@pytest.mark.gpu
def test_identity_plant_changes_nothing():
    """N = 10, B = 300: in K3p a block of 256 threads ends inside a car.  An identity plant (with a seed: the variates are drawn
    and multiplied by zero) against a handle without a plant, and the accumulators against numpy over single-step snapshots."""
    N, B, steps = 10, 300, 25
    g1, _, cum = _sim()
    w, s0, poses = _starts(B, 11)
    ref = _handle(N, B)
    ref.rollout_init(TS, cum, s0, poses)
    ref.rollout_step(steps)
    want = ref.rollout_state()
    ref.close()
    h = _handle(N, B)
    h.rollout_set_plant(Plant(seed=99).params(B), seed=99)
    h.rollout_init(TS, cum, s0, poses)
    cosw, sinw = np.array([math.cos(a) for a in g1["psi"]]), np.array([math.sin(a) for a in g1["psi"]])
    ey_max, ey_sq, n_driven = np.zeros(B), np.zeros(B), np.zeros(B, np.int32)
    before = poses
    for _ in range(steps):
        h.rollout_step(1)
        st = h.rollout_state()
        wp = st["wp_id"]
        e = cosw[wp] * (before[:, 1] - g1["y"][wp]) - sinw[wp] * (before[:, 0] - g1["x"][wp])
        driven = st["alive"] == 1
        ey_max = np.where(driven, np.maximum(ey_max, np.abs(e)), ey_max)
        ey_sq = np.where(driven, ey_sq + e * e, ey_sq)
        n_driven += driven
        before = st["pose"]
    got, pl = h.rollout_state(), h.rollout_plant()
    h.close()
    _equal_states(got, want)
    assert _same_bits(pl["ey_max"], ey_max) and _same_bits(pl["ey_sq"], ey_sq) and np.array_equal(pl["steps"], n_driven)
    assert np.sum(n_driven == steps) > B // 2 and np.all(ey_max[n_driven > 1] > 0)      # (some cars end early: they stop counting)
    alive = got["alive"] == 1
    assert _same_bits(pl["act"][alive], got["u"][alive])      # executed = commanded


@pytest.mark.gpu
def test_one_call_equals_many_and_a_resumed_run():
    N, B, steps, at = 10, 70, 25, 10
    _, _, cum = _sim()
    w, s0, poses = _starts(B, 12, last=160)
    plant = Plant(seed=4242, car0=5, **NOISY)
    h = _handle(N, B, warm=False)
    h.rollout_set_plant(plant.params(B), plant.seed, plant.car0)
    h.rollout_init(TS, cum, s0, poses)
    h.rollout_step(steps)
    want, want_pl = h.rollout_state(), h.rollout_plant()
    assert np.all(want["alive"] == 1)      # (a resumed run starts every car alive)
    # 25 calls of one step, saved at step 10
    h.rollout_init(TS, cum, s0, poses)      # (the plant in force stays; its actuators and accumulators start over)
    for t in range(steps):
        if t == at:
            saved, saved_pl = h.rollout_state(), h.rollout_plant()
        h.rollout_step(1)
    got, got_pl = h.rollout_state(), h.rollout_plant()
    _equal_states(got, want)
    for k in mpmpc.Handle.PLANT_FIELDS:
        assert np.array_equal(got_pl[k], want_pl[k]), k
    assert np.all(want_pl["steps"] == steps)
    # resumed from the save: k restarts at 0, the noise continues at j = 10
    h.rollout_init(TS, cum, saved["s"], saved["pose"], saved["cc"])
    h.rollout_set_counters(saved["counter"])
    h.rollout_set_plant(plant.params(B), plant.seed, plant.car0, step0=-at, act0=saved_pl["act"])
    h.rollout_step(steps - at)
    res, res_pl = h.rollout_state(), h.rollout_plant()
    h.close()
    _equal_states(res, want)
    assert _same_bits(res_pl["act"], want_pl["act"]) and _same_bits(res_pl["meas"], want_pl["meas"])
    assert np.all(res_pl["steps"] == steps - at)
    # and the noise mattered: the measured pose is not the true one
    assert np.all(np.abs(want_pl["meas"] - saved["pose"]).max(axis=1) > 0)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [10, 30])
def test_closed_loop_matches_the_host_loop(N):
    """Every car against the reference's loop run with the project's host classes, one car at a time, with Plant.apply around
    get_control and the plant step."""
    g1, g3, cum = _sim()
    steps, seed = 25, 12345
    starts = np.array([0, 12, 37, 88, 120, 150, 171])
    B = starts.size
    plant = Plant(seed=seed, **NOISY)
    host, statuses = [], []
    for i, w in enumerate(starts):
        m, rp, car = T.build_world(obstacles=False)
        mpc = T.make_mpc(car, N)
        one = plant.car(i)
        st = dict(pose=np.array([[rp.waypoints[w].x, rp.waypoints[w].y, rp.waypoints[w].psi]]), s=np.array([float(cum[w])]),
                  act=np.zeros((1, 2)))

        def control(meas):
            car.s = float(st["s"][0])
            car.temporal_state = TemporalState(*meas[0])
            u = mpc.get_control()
            statuses.append(mpc.last_status)
            return u, [[car.spatial_state.e_y, car.spatial_state.e_psi]], [car.current_waypoint.kappa]
        for k in range(steps):
            st = one.apply(k, st["pose"], st["s"], st["act"], control, car.length, car.Ts)
        host.append(np.concatenate([st["s"], st["pose"][0], st["meas"][0], st["u"][0], st["act"][0]]))
    host = np.array(host)
    assert all(v == 1 for v in statuses), statuses      # the comparison must not cross a verdict boundary
    h = _handle(N, B)
    h.rollout_set_plant(plant.params(B), plant.seed)
    poses = np.stack([g1["x"][starts], g1["y"][starts], g1["psi"][starts]], axis=1)
    h.rollout_init(TS, cum, cum[starts], poses)
    h.rollout_step(steps)
    st, pl = h.rollout_state(), h.rollout_plant()
    h.close()
    figures = dict(s=np.max(np.abs(st["s"] - host[:, 0])), pose=np.max(np.abs(st["pose"] - host[:, 1:4])),
                   meas=np.max(np.abs(pl["meas"] - host[:, 4:7])), u=np.max(np.abs(st["u"] - host[:, 7:9])),
                   act=np.max(np.abs(pl["act"] - host[:, 9:11])))
    print("plant closed loop N=%d:" % N, figures)
    assert np.all(st["alive"] == 1)
    assert figures["s"] <= 1e-8 and figures["pose"] <= 1e-8 and figures["meas"] <= 1e-8
    assert figures["u"] <= 1e-6 and figures["act"] <= 1e-6
    assert np.all(pl["steps"] == steps)


@pytest.mark.gpu
def test_consumers_keep_the_true_pose():
    """The lidar scan and the audit judge the true car; K3a localises on the measured pose."""
    N, B = 10, 8
    g1, g3, cum = _sim()
    h0, w0 = g1["grid_shape"]
    grid = np.ascontiguousarray(np.unpackbits(g1["grid_free"])[:h0 * w0].reshape(h0, w0).astype(np.int8))
    origin, res = tuple(float(v) for v in g1["origin"]), float(g1["resolution"][0])
    sm = float(g3["safety_margin"][0])
    tr = scenarios.sim_track()
    h = mpmpc.Handle(T.stock_config(N, max_batch=B))
    h.set_path(tr.kappa, tr.v_ref, tr.ds_next)
    h.set_map(grid, origin, res)
    h.set_path_geometry(g1["x"], g1["y"], g1["psi"], g1["border_ub"], g1["border_lb"])
    h.build_corridor(N, 2 * sm, sm, want_tables=False)
    w, s0, poses = _starts(B, 13, last=160)
    ang = np.linspace(-1.5, 1.5, 31)
    length, width, reach = 0.12, 0.06, 0.2
    h.rollout_set_audit(1, length, width, reach)
    h.rollout_set_plant(Plant(position_noise=0.01).params(B), seed=7)
    h.rollout_init(TS, cum, s0, poses)
    before = h.rollout_state()["pose"]
    assert _same_bits(before, poses)
    for k in range(2):      # the issue's one step, and one more whose start the plant has already moved
        h.rollout_step(1)
        st, pl, aud = h.rollout_state(), h.rollout_plant(), h.rollout_audit()
        assert np.all(st["alive"] == 1)
        assert np.array_equal(h.rollout_scan(ang, 0.3), mpmpc.lidar_scan(grid, origin, res, st["pose"], ang, 0.3))
        contact, clearance = mpmpc.footprint_audit(grid, origin, res, before, length, width, reach)      # the step's own pose
        assert np.array_equal(aud["last_contact"], contact) and _same_bits(aud["last_clearance"], clearance)
        wp = st["wp_id"]
        x0 = t2s_batch(pl["meas"][:, 0], pl["meas"][:, 1], pl["meas"][:, 2], g1["x"][wp], g1["y"][wp], g1["psi"][wp])
        assert np.max(np.abs(st["x0"] - x0)) <= 1e-13
        noise = Plant(position_noise=0.01, seed=7).noise(B, [k])[0]
        assert _same_bits(pl["meas"], np.stack([before[:, 0] + 0.01 * noise[:, 2], before[:, 1] + 0.01 * noise[:, 3], before[:, 2]], 1))
        assert np.all(np.abs(pl["meas"][:, :2] - before[:, :2]).max(axis=1) > 0)      # measured, not true
        before = st["pose"]
    h.close()


@pytest.mark.gpu
def test_state_and_argument_errors():
    N, B = 10, 8
    _, _, cum = _sim()
    w, s0, poses = _starts(B, 14, last=160)
    plant = Plant(seed=3, **NOISY)
    h = _handle(N, B, warm=False)
    h.rollout_init(TS, cum, s0, poses)
    with pytest.raises(mpmpc.MpmpcError) as e:
        h.rollout_plant()      # no plant
    assert _code(e) == E_STATE
    h.rollout_set_plant(plant.params(B), plant.seed)
    with pytest.raises(mpmpc.MpmpcError) as e:
        h.rollout_plant()      # no step under it yet
    assert _code(e) == E_STATE
    h.rollout_step(3)
    h.rollout_step(3)
    want, want_pl = h.rollout_state(), h.rollout_plant()
    # a refused call leaves the running setting's next step unchanged
    h.rollout_init(TS, cum, s0, poses)
    h.rollout_step(3)
    for col, bad, _ in TABLE:
        p = plant.params(B)
        p[B - 1, col] = bad[0]
        with pytest.raises(mpmpc.MpmpcError) as e:
            h.rollout_set_plant(p, seed=1, step0=5)
        assert _code(e) == E_ARG, NAMES[col]
    with pytest.raises(mpmpc.MpmpcError) as e:
        h.rollout_set_plant(plant.params(B), act0=np.full((B, 2), np.nan))
    assert _code(e) == E_ARG
    with pytest.raises(mpmpc.MpmpcError) as e:
        h.rollout_set_plant(plant.params(B + 1))      # more than max_batch
    assert _code(e) == E_ARG
    h.rollout_step(3)
    got, got_pl = h.rollout_state(), h.rollout_plant()
    _equal_states(got, want)
    for k in mpmpc.Handle.PLANT_FIELDS:
        assert np.array_equal(got_pl[k], want_pl[k]), k
    # a step of another B
    h.rollout_init(TS, cum, s0[:5], poses[:5])
    with pytest.raises(mpmpc.MpmpcError) as e:
        h.rollout_step(1)
    assert _code(e) == E_STATE
    h.rollout_set_plant(None)
    h.rollout_step(1)      # without a plant: any B the rollout holds
    with pytest.raises(mpmpc.MpmpcError) as e:
        h.rollout_plant()
    assert _code(e) == E_STATE
    h.close()


@pytest.mark.gpu
def test_batchmpc_rollout_takes_a_plant():
    """BatchMPC.rollout(..., plant=...) on a corridor table (no corridor='device'): an identity plant is the rollout without
    one, a noisy one returns its state under "plant", and the setting goes off again with the next call without one."""
    from MPC import BatchMPC
    from scipy import sparse
    _, g3, cum = _sim()
    m, rp, car = T.build_world(obstacles=False)
    Q, R, QN = sparse.diags([1.0, 0.0, 0.0]), sparse.diags([0.5, 0.0]), sparse.diags([1.0, 0.0, 0.0])
    ic = {'umin': np.array([0.0, -np.tan(0.66) / car.length]), 'umax': np.array([1.0, np.tan(0.66) / car.length])}
    sc = {'xmin': np.array([-np.inf] * 3), 'xmax': np.array([np.inf] * 3)}
    B, N, steps = 8, 10, 12
    bm = BatchMPC(car, N, Q, R, QN, sc, ic, 4.0, max_batch=B, corridor=(g3["ub_free"], g3["lb_free"]))
    w, s0, poses = _starts(B, 15, last=160)
    plain = bm.rollout(s0, poses, steps)
    assert "plant" not in plain
    same = bm.rollout(s0, poses, steps, plant=Plant(seed=8))
    pl = same.pop("plant")
    _equal_states(same, plain)
    assert np.all(pl["steps"] == steps) and _same_bits(pl["act"], plain["u"])
    noisy = bm.rollout(s0, poses, steps, plant=Plant(seed=8, **NOISY))
    assert np.all(noisy["alive"] == 1) and np.all(noisy["plant"]["steps"] == steps)
    assert np.all(np.abs(noisy["pose"] - plain["pose"]).max(axis=1) > 0)
    assert bm.rollout(s0, poses, 0, plant=Plant(seed=8, **NOISY))["plant"] is None
    again = bm.rollout(s0, poses, steps)      # off again
    _equal_states(again, plain)
    with pytest.raises(mpmpc.MpmpcError):
        bm.handle.rollout_plant()
