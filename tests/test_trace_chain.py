"""The pose chain in the trace (MPMPC_REC_PLANT .. MPMPC_REC_SCAN of mpmpc_rollout_record, mpmpc_rollout_trace_chain): what the
plant, the delay, the estimator and the localiser left in their own buffers at the end of every recorded step, written behind
the record by a third recorder kernel.  The law is one sentence - every value is the one the matching getter would return if
it were called right after that step - plus the masks of include/mpmpc.h, restated here ONCE with numpy (expected_chain) and
used by both halves.

CPU: the header, the exports and the constants; ro_chain_layout over every subset of the bits; ro_record_chain on the host
(tests/emul_chain) against expected_chain on random sources.  GPU: one rollout_step(8) that records against eight
rollout_step(1) with every getter downloaded in between, bit for bit, on seven fleets; recording changes neither the state
nor the old fields; the recorded chain explains the step's own wp_id and x0 (and no other candidate does); refusals and
lifetime; the new kernel's resources."""
import ctypes as C
import functools
import itertools
import os
import re

import numpy as np
import pytest

import mpc_np as M
import mpmpc
import chain_twin
import twins
import test_delay as TD          # (Sim_Track's path, the in-flight register, _same_bits, _code)
import test_estimator as TE      # (the noisy plant's values, the estimator's setter)
import test_localiser as TLc     # (the fleets on the device's map, the lidar stand-in, the localiser's setter)
import test_pose_chain as TP     # (SEP, T2S_TOL and _sep: the pose chain's own separation rule)
from delay import current_waypoint, t2s
from estimator import Estimator
from localiser import Localiser
from plant import Plant

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_STATE = -1, -3
PLANT, DELAY, EST, FIX, SCAN = 8, 16, 32, 64, 128
BITS = (PLANT, DELAY, EST, FIX, SCAN)
GROUPS = {PLANT: ("act", "meas"), DELAY: ("queue", "pred_pose", "pred_s", "now"), EST: ("est", "cov", "used"),
          FIX: ("fix", "prior", "cand", "score", "hits"), SCAN: ("ranges",)}
FEATURE = {PLANT: "plant", DELAY: "delay", EST: "estimator", FIX: "localiser", SCAN: "localiser"}      # the feature a group belongs to
FIELDS = chain_twin.FIELDS
INTS = chain_twin.INTS
OUTLIVES = ("act", "queue", "used")      # state that outlives a step: recorded for every car, as it stands
EMPTY = dict(used=-1, cand=-2, score=-2, hits=-2)      # (doubles: NaN)
OLD = ("s", "pose", "wp_id", "x0", "u", "status", "counter", "alive", "plan", "pred_x", "pred_y", "ub", "lb")
TS, L_CAR = TD.TS, TD.L_CAR
_same_bits, _code = TD._same_bits, TD._code
_d, _i = chain_twin.T._d, chain_twin.T._i


def _shape(f, n_beams):
    return dict(act=(2,), meas=(3,), queue=(8, 2), pred_pose=(3,), pred_s=(), now=(3,), est=(3,), cov=(6,), used=(), fix=(3,), prior=(3,),
                cand=(), score=(), hits=(), ranges=(n_beams,))[f]


def _eq(a, b):
    """bit-equal, NaN in the same places"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and (np.array_equal(a, b, equal_nan=True) if a.dtype.kind == "f" else np.array_equal(a, b))


# --------------------------------------------------------------------------------------------------------- the masks
def expected_chain(fields, on, a_in, src, n_beams=0):
    """include/mpmpc.h's masks with numpy.  fields: the bits recorded;  on: {feature: in force at the step};  a_in [B]: alive
    before the step;  src: {field: what the getter returns after the step} (of the features that are on);  n_beams: of a
    recorded scan -> {field: [B, ...]}"""
    a_in = np.asarray(a_in)
    B, ran = a_in.size, np.asarray(a_in) == 1
    out = {}
    for bit in BITS:
        if not fields & bit:
            continue
        for f in GROUPS[bit]:
            if not on[FEATURE[bit]]:
                mask = np.zeros(B, bool)
            elif f in OUTLIVES:
                mask = np.ones(B, bool)
            elif f == "ranges":
                mask = ran & (np.asarray(src["hits"]) >= 0)
            else:
                mask = ran
            v = np.asarray(src[f]) if on[FEATURE[bit]] else np.zeros((B,) + _shape(f, n_beams))
            empty = EMPTY.get(f, np.nan)
            out[f] = np.where(mask.reshape((B,) + (1,) * (v.ndim - 1)), v, empty).astype(np.int32 if f in INTS else np.float64)
    return out


# ------------------------------------------------------------------------------------------------------------ CPU
@pytest.fixture(scope="module")
def twin():
    """The CPU twin of the chain kernel (tests/emul_chain)."""
    return chain_twin.chain()


def _layout(twin, B, fields, n_beams):
    out = (C.c_longlong * len(chain_twin.LAYOUT))()
    twin.chain_emu_layout(B, fields, n_beams, out)
    return dict(zip(chain_twin.LAYOUT, out))


def test_abi_declares_the_chain(built_library):
    raw = open(os.path.join(ROOT, "include", "mpmpc.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for macro, val in (("MPMPC_REC_PLANT", 8), ("MPMPC_REC_DELAY", 16), ("MPMPC_REC_EST", 32), ("MPMPC_REC_FIX", 64), ("MPMPC_REC_SCAN", 128)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, val), text), macro
    assert (mpmpc.REC_PLANT, mpmpc.REC_DELAY, mpmpc.REC_EST, mpmpc.REC_FIX, mpmpc.REC_SCAN) == BITS
    assert re.search(r"\bint\s+mpmpc_rollout_trace_chain\s*\(", text)
    lib = mpmpc.load_library(built_library)
    assert "mpmpc_rollout_trace_chain" in mpmpc.EXPORTS and hasattr(lib, "mpmpc_rollout_trace_chain")
    lib.mpmpc_rollout_trace_chain.argtypes = [C.c_void_p] + [C.c_int32] * 3 + [C.c_void_p] * 15
    assert lib.mpmpc_rollout_trace_chain(None, 1, 0, 0, *([None] * 15)) == E_ARG and b"handle is NULL" in lib.mpmpc_last_error()
    assert "the fix in the trace" not in raw      # (no longer out of scope)


def test_layout_of_every_subset(twin):
    """all 32 subsets of the new bits: every selected field 256-aligned, disjoint, inside `bytes`, in the getter's order; the
    others -1; the chain begins where the old record ends, and the old record's size is what it was for its 8 subsets"""
    trace = twins.trace()
    N = 10
    per_car = lambda f, n: int(np.prod(_shape(f, n), dtype=int)) * (4 if f in INTS else 8)
    for B, n_beams in itertools.product((1, 3, 64, 1000), (1, 30, 2048)):
        pad = lambda b: (b * B + 255) // 256 * 256
        old = {fields: trace.trace_emu_record_bytes(N, B, fields) for fields in range(8)}
        for fields in range(8):      # the old record, restated: 88 bytes of basic fields per car in 8 blocks, then the optional ones
            want = sum(pad(b) for b in (8, 24, 24, 16, 4, 4, 4, 4)) + (pad(16 * N) if fields & 1 else 0) + \
                (2 * pad(8 * (N - 2)) if fields & 2 else 0) + (2 * pad(8 * N) if fields & 4 else 0)
            assert old[fields] == want and want % 256 == 0, (B, fields)
        for sub in range(32):
            fields = sub << 3
            lay = _layout(twin, B, fields, n_beams)
            at, entries = 0, 0
            for bit in BITS:
                for f in GROUPS[bit]:
                    if not fields & bit:
                        assert lay[f] == -1, (B, n_beams, fields, f)
                        continue
                    assert lay[f] == at and lay[f] % 256 == 0, (B, n_beams, fields, f)      # (in order and back to back: disjoint)
                    at += pad(per_car(f, n_beams))
                    entries += int(np.prod(_shape(f, n_beams), dtype=int))
            assert lay["bytes"] == at and lay["bytes"] % 256 == 0 and lay["entries"] == entries, (B, n_beams, fields)
            assert lay["n_beams"] == (n_beams if fields & SCAN else 0)
            for low in range(8):      # a record of (low | fields): the old part unchanged, the chain from its end, both 256-aligned
                assert trace.trace_emu_record_bytes(N, B, (low | fields) & 7) == old[low]
                assert (old[low] + at) % 256 == 0


def _random_sources(rng, B, n_beams):
    src = {f: (rng.integers(-1, 50, (B,) + _shape(f, n_beams)).astype(np.int32) if f in INTS else rng.normal(size=(B,) + _shape(f, n_beams)))
           for f in FIELDS}
    src["hits"] = rng.choice(np.array([-1, 0, 5], np.int32), B)
    return src


def _twin_record(twin, fields, on, a_in, src, n_beams):
    B = a_in.size
    have = [f for bit in BITS if fields & bit for f in GROUPS[bit]]
    out = {f: (np.full((B,) + _shape(f, n_beams), 77, np.int32) if f in INTS else np.full((B,) + _shape(f, n_beams), 77.0)) for f in have}
    group_on = {f: on[FEATURE[bit]] for bit in BITS for f in GROUPS[bit]}
    keep = {f: np.ascontiguousarray(src[f], np.int32 if f in INTS else np.float64) for f in FIELDS}
    ins = [(_i(keep[f]) if f in INTS else _d(keep[f])) if group_on[f] else None for f in FIELDS]
    outs = [(_i(out[f]) if f in INTS else _d(out[f])) if f in out else None for f in FIELDS]
    a = np.ascontiguousarray(a_in, np.int32)
    assert twin.chain_emu_record(B, fields, n_beams, _i(a), *ins, *outs) == 0
    return out


def test_twin_masks_every_subset(twin):
    """64 cars, a_in and a from every kind of ending, random feature flags and sources: the twin's record equals expected_chain
    bit for bit for every subset of the bits (with every combination of flags for the full set); an entry the code does not
    write would show as the twin's 0x5a fill"""
    rng = np.random.default_rng(17)
    B, n_beams = 64, 7
    kinds = np.array([1, 0, -1, -2, -3, -5], np.int32)
    flag_sets = [dict(zip(("plant", "delay", "estimator", "localiser"), bits)) for bits in itertools.product((False, True), repeat=4)]
    seen = set()
    for sub in range(32):
        fields = sub << 3
        for on in (flag_sets if sub == 31 else [flag_sets[i] for i in rng.integers(0, 16, 3)]):
            a_in = rng.choice(kinds, B)
            a_in[:6] = kinds      # (every kind occurs)
            src = _random_sources(rng, B, n_beams)
            got = _twin_record(twin, fields, on, a_in, src, n_beams)
            want = expected_chain(fields, on, a_in, src, n_beams)
            assert sorted(got) == sorted(want)
            for f in want:
                assert _eq(got[f], want[f]), (fields, on, f)
            seen.add((fields, tuple(on.values())))
    assert len({s[0] for s in seen}) == 32 and len({s[1] for s in seen if s[0] == 31 << 3}) == 16
    # what the masks mean, once by hand: everything on, car 0 running with a scan, car 1 running without one, car 2 ended before
    on = flag_sets[-1]
    a_in = np.array([1, 1, -2], np.int32)
    src = _random_sources(rng, 3, n_beams)
    src["hits"] = np.array([5, -1, 5], np.int32)
    got = _twin_record(twin, 31 << 3, on, a_in, src, n_beams)
    assert _same_bits(got["act"], src["act"]) and _same_bits(got["queue"], src["queue"]) and np.array_equal(got["used"], src["used"])
    assert _same_bits(got["meas"][:2], src["meas"][:2]) and np.all(np.isnan(got["meas"][2])) and np.all(np.isnan(got["est"][2]))
    assert list(got["hits"]) == [5, -1, -2] and list(got["cand"][:2]) == list(src["cand"][:2]) and got["cand"][2] == -2
    assert _same_bits(got["ranges"][0], src["ranges"][0]) and np.all(np.isnan(got["ranges"][1:]))
    off = _twin_record(twin, 31 << 3, flag_sets[0], a_in, src, n_beams)
    assert all(np.all(off[f] == EMPTY[f]) if f in INTS else np.all(np.isnan(off[f])) for f in off)


# ------------------------------------------------------------------------------------------------------------ GPU
N, B, STEPS = 10, 12, 8
SEED = 7      # (of the plant's noise: test 6's condition on the candidates' separation holds with it)
ON_OFF = ("plant", "delay", "estimator", "localiser")
FLEETS = {      # name -> (features on, case of test_localiser._step_setup, bits recorded beside the chain's four)
    "plant": (("plant",), "plain", 0),
    "plant_delay": (("plant", "delay"), "plain", 0),
    "plant_estimator_delay": (("plant", "estimator", "delay"), "plain", 0),
    "localiser_estimator_plant": (("localiser", "estimator", "plant"), "plain", SCAN),
    "all": (ON_OFF, "plain", SCAN),
    "two_routes": (ON_OFF, "two_routes", SCAN),
    "none": ((), "plain", 0),
}
GETTER = dict(plant="rollout_plant", delay="rollout_delay", estimator="rollout_estimator", localiser="rollout_localiser")


def _settings():
    """the issue's shapes: 30 beams of 1 m, W = T = 1; 3 cm / 0.05 rad of pose noise, a lag and a gain; d = 2 with c = 1 on half the
    cars (c = d on the others), the commands in flight steering, so that a prediction differs from what it starts from in
    position AND heading from the first step on"""
    plant = Plant(speed_gain=0.97, speed_lag=0.8, position_noise=0.03, heading_noise=0.05, seed=SEED, car0=2)
    loc = Localiser(TLc._lidar(30, rng=1.0), D=6, step_cells=1, window=1, headings=1, step_psi=0.01, min_hits=5, sigma_r=0.004, period=2, seed=3,
                    car0=1)
    est = Estimator.matched(plant, period=[1 + i % 3 for i in range(B)], drop=0.25, seed=21, car0=9, step0=-3)
    d, c = np.full(B, 2, np.int32), (1 + np.arange(B) % 2).astype(np.int32)
    return plant, loc, est, (d, c, TD._in_flight(B, 0.6, 0.1))


def _start(name, record=None):
    """-> a handle of the fleet at step 0, its features set in one order whoever asks; record: rollout_record's keywords"""
    feats, case, _ = FLEETS[name]
    plant, loc, est, delay = _settings()
    h, cum, s0, poses = TLc._step_setup(case, B, N)
    if case == "two_routes":      # cars 1 and 3 start 3 and 5 waypoints in front of where the open second route ends them
        cat, first, _ = TD._two_routes()
        s0, poses = s0.copy(), poses.copy()
        for car, w in ((1, 87), (3, 85)):
            g = first[1] + w
            s0[car], poses[car] = cat["cum_lengths"][g], (cat["x"][g] + 0.00113, cat["y"][g] - 0.00071, cat["psi"][g])
    if "plant" in feats:
        h.rollout_set_plant(plant.params(B), plant.seed, plant.car0)
    if "localiser" in feats:      # (in force before rollout_record: a recorded scan takes its n_beams)
        TLc._set(h, loc, B)
    if record is not None:
        h.rollout_record(STEPS, B=B, **record)
    h.rollout_init(TS, cum, s0, poses)
    if "delay" in feats:
        h.rollout_set_delay(*delay)
    if "estimator" in feats:
        TE._set(h, est, B)
    if "localiser" in feats:
        TLc._set(h, loc, B)
    return h


def _record_kw(name, chain=True):
    scan = bool(FLEETS[name][2] & SCAN)
    return dict(plan=True, prediction=True, rows=True, **(dict(chain=True, scan=scan) if chain else {}))


@functools.lru_cache(None)
def _runs(name):
    """The fleet three times: A records everything and takes its 8 steps in one call; B takes them one per call, unrecorded,
    with rollout_state and every getter of a feature in force downloaded after each; D records the old fields only.
    -> dict(trace, state: A's;  before, after, got: B's per step;  final: B's last state;  old: D's trace and state)"""
    feats = FLEETS[name][0]
    a = _start(name, _record_kw(name))
    try:
        a.rollout_step(STEPS)
        out = dict(trace=a.rollout_trace(), state=a.rollout_state())
    finally:
        a.close()
    b = _start(name)
    try:
        out.update(before=[], after=[], got=[])
        for k in range(STEPS):
            out["before"].append(b.rollout_state())
            b.rollout_step(1)
            out["after"].append(b.rollout_state())
            got = {}
            for f in feats:
                got.update(getattr(b, GETTER[f])())
            out["got"].append(got)
        out["final"] = out["after"][-1]
    finally:
        b.close()
    d = _start(name, _record_kw(name, chain=False))
    try:
        d.rollout_step(STEPS)
        out["old"] = dict(trace=d.rollout_trace(), state=d.rollout_state())
    finally:
        d.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(FLEETS))
def test_one_call_equals_many_and_the_getters(name):
    """record k of the one-call run against the getters downloaded after step k of the one-step-per-call run: bit-equal where
    the masks say "recorded", empty exactly where they say "empty" (expected_chain states both), the masks from the second
    run's alive before the step"""
    feats, _, extra = FLEETS[name]
    fields = PLANT | DELAY | EST | FIX | extra
    r = _runs(name)
    trace = r["trace"]
    want_keys = set(OLD) | {f for bit in BITS if fields & bit for f in GROUPS[bit]}
    assert set(trace) == want_keys and all(trace[f].shape[:2] == (STEPS, B) for f in trace)
    on = {f: f in feats for f in ON_OFF}
    filled = {f: 0 for f in FIELDS}
    for k in range(STEPS):
        assert np.array_equal(trace["alive"][k], r["after"][k]["alive"]), k      # (the two runs are the same run)
        want = expected_chain(fields, on, r["before"][k]["alive"], r["got"][k], 30)
        for f, v in want.items():
            assert _eq(trace[f][k], v), (name, k, f)
            filled[f] += int(np.sum(v != EMPTY[f]) if f in INTS else np.sum(~np.isnan(v)))
    for bit in BITS:      # every group of a feature in force was compared on values, every other group is empty throughout
        for f in GROUPS[bit]:
            if fields & bit:
                assert (filled[f] > 0) == on[FEATURE[bit]], (name, f, filled[f])
    if name == "two_routes":      # a car reaches the open end of the second route before the last step: its later records are empty
        ended = [(i, k) for i in range(B) for k in range(STEPS - 1) if trace["alive"][k, i] == -2 and (k == 0 or trace["alive"][k - 1, i] == 1)]
        assert ended, trace["alive"]
        for i, k in ended:
            for f in ("meas", "pred_pose", "pred_s", "now", "est", "cov", "fix", "prior", "ranges"):
                assert np.all(np.isnan(trace[f][k + 1:, i])), (i, k, f)
            assert np.all(trace["hits"][k + 1:, i] == -2) and np.all(trace["cand"][k + 1:, i] == -2) and np.all(trace["score"][k + 1:, i] == -2)
            assert _same_bits(trace["act"][k + 1:, i], np.broadcast_to(trace["act"][k, i], (STEPS - 1 - k, 2)))      # (state: it stands)
            assert np.all(trace["used"][k + 1:, i] == trace["used"][k, i]) and trace["used"][k, i] >= 1
    if name == "none":
        assert all(np.all(np.isnan(trace[f])) for f in ("act", "meas", "queue", "pred_pose", "pred_s", "now", "est", "cov", "fix", "prior"))
        assert np.all(trace["used"] == -1) and all(np.all(trace[f] == -2) for f in ("cand", "score", "hits"))
    if fields & SCAN:      # a scheduled step of a running, primed car holds a scan; period 2: every other record holds none
        assert np.all(trace["hits"][1::2][trace["alive"][0::2][:STEPS // 2] == 1] == -1)
        assert np.any(trace["hits"][2::2] >= 0) and np.all(np.isnan(trace["ranges"][1::2]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(FLEETS))
def test_recording_perturbs_nothing(name):
    """the final state of the run that recorded the chain is the unrecorded run's, and the old fields of its trace are those of
    a trace recorded with the old bits alone - bit for bit"""
    r = _runs(name)
    for f in TD.KEYS:
        assert _eq(r["state"][f], r["final"][f]), (name, f)
        assert _eq(r["old"]["state"][f], r["final"][f]), (name, f)
    assert sorted(r["old"]["trace"]) == sorted(OLD)
    for f in OLD:
        assert _eq(r["trace"][f], r["old"]["trace"][f]), (name, f)


@pytest.mark.gpu
def test_the_chain_is_the_steps_own():
    """The multi-step form of test_pose_chain's K3a row, on the fleet with everything on.  K3a localises on pred_pose at
    pred_s; so for every record with a waypoint, wp_id is delay.current_waypoint of the RECORDED pred_s and x0 is delay.t2s of the
    RECORDED pred_pose at that waypoint to T2S_TOL - the record's chain is the one its own step used.  Negative control: on the
    records whose other candidates (est, fix, meas, the true pose) all lie more than SEP from pred_pose in position and
    heading - at least 90 % of them, asserted - the t2s of every other candidate misses x0 by more than T2S_TOL."""
    tr = _runs("all")["trace"]
    lap = TD._lap()
    others = ("est", "fix", "meas", "pose")
    checked = apart = 0
    worst, nearest_miss = 0.0, np.inf
    for k, i in itertools.product(range(STEPS), range(B)):
        w = int(tr["wp_id"][k, i])
        if w < 0:
            continue
        checked += 1
        assert w == current_waypoint(lap.cum, float(tr["pred_s"][k, i])), (k, i)
        at = lambda pose: np.array(t2s(tuple(float(v) for v in pose), lap.x[w], lap.y[w], lap.psi[w]))[:2]
        d = float(np.max(np.abs(at(tr["pred_pose"][k, i]) - tr["x0"][k, i, :2])))
        worst = max(worst, d)
        assert d <= TP.T2S_TOL, (k, i, d)
        if not all(TP._sep(tr["pred_pose"][k, i], tr[c][k, i]) > TP.SEP for c in others):
            continue
        apart += 1
        for c in others:
            miss = float(np.max(np.abs(at(tr[c][k, i]) - tr["x0"][k, i, :2])))
            nearest_miss = min(nearest_miss, miss)
            assert miss > TP.T2S_TOL, (k, i, c, miss)
    print("chain of the step: %d records, %d with every other candidate apart; worst |t2s(pred_pose) - x0| %.2e, nearest miss of another "
          "candidate %.2e" % (checked, apart, worst, nearest_miss))
    assert checked > STEPS * B // 2 and apart >= 0.9 * checked, (checked, apart)


def _refused(call, code, word=""):
    with pytest.raises(mpmpc.MpmpcError) as err:
        call()
    assert _code(err) == code and word in str(err.value), str(err.value)


@pytest.mark.gpu
def test_refusals_and_lifetime():
    plant, loc, est, delay = _settings()
    loc31 = Localiser(TLc._lidar(31, rng=1.0), D=6, step_cells=1, window=1, headings=1, step_psi=0.01, min_hits=5)
    h, cum, s0, poses = TLc._step_setup("plain", B, N)
    try:
        # unknown bits; a scan without a localiser
        assert h.lib.mpmpc_rollout_record(h._h, B, 4, 256, 1) == E_ARG and h.lib.mpmpc_rollout_record(h._h, B, 4, 255 + 512, 1) == E_ARG
        _refused(lambda: h.rollout_record(4, scan=True, B=B), E_STATE, "MPMPC_REC_SCAN needs a localiser")
        # a trace without the estimator's bit
        h.rollout_set_plant(plant.params(B), plant.seed, plant.car0)
        TLc._set(h, loc, B)
        h.rollout_record(4, plant=True, fix=True, scan=True, B=B)
        h.rollout_init(TS, cum, s0, poses)
        TLc._set(h, loc, B)
        h.rollout_step(2)
        assert sorted(h.rollout_trace()) == sorted(OLD[:8] + ("act", "meas", "fix", "prior", "cand", "score", "hits", "ranges"))
        _refused(lambda: h.rollout_trace(fields=["est"]), E_STATE, "did not select")
        _refused(lambda: h.rollout_trace(fields=["queue", "act"]), E_STATE, "did not select")
        # records beyond those held
        _refused(lambda: h.rollout_trace(first=1, count=2, fields=["act"]), E_STATE, "held")
        assert h.rollout_trace(first=1, count=1, fields=["act"])["act"].shape == (1, B, 2)
        # a localiser with another n_beams while the scan is recorded: refused before anything is launched
        state, trace = h.rollout_state(), h.rollout_trace()
        TLc._set(h, loc31, B)
        _refused(lambda: h.rollout_step(1), E_STATE, "beams")
        now = h.rollout_state()
        assert all(_eq(now[f], state[f]) for f in TD.KEYS) and h.rollout_recorded() == (2, 2)
        assert all(_eq(v, trace[f]) for f, v in h.rollout_trace().items())
        # the plant switched off between two calls: meas (and act) empty from then on, filled before
        TLc._set(h, loc, B)
        h.rollout_set_plant(None)
        h.rollout_step(2)
        t = h.rollout_trace()
        running = t["alive"] == 1
        assert running[:2].any() and np.all(np.isfinite(t["meas"][:2][running[:2]])) and np.all(np.isfinite(t["act"][:2]))
        assert np.all(np.isnan(t["meas"][2:])) and np.all(np.isnan(t["act"][2:])) and np.all(np.isfinite(t["fix"][2:][running[2:]]))
        # a full trace refuses the step, as before
        _refused(lambda: h.rollout_step(1), E_STATE, "the trace is full")
        assert h.rollout_recorded() == (4, 4)
        # the chain stays readable after a solve has invalidated the rollout
        g = np.load(M.GOLDEN + "/g6_closed_loop_N%d.npz" % N)
        h.solve(g["wp_id"][:2].astype(np.int32), g["x0"][:2], g["cc_prev"][:2], g["lb"][:2], g["ub"][:2])
        _refused(lambda: h.rollout_step(1), E_STATE, "rollout_init")
        assert all(_eq(v, t[f]) for f, v in h.rollout_trace().items())
    finally:
        h.close()
    # stride 3: record r is step 3 r
    every = dict(chain=True, scan=True)
    out = []
    for stride in (1, 3):
        feats = FLEETS["all"][0]
        h = _start("all", dict(every, stride=stride))
        try:
            h.rollout_step(STEPS - 1)
            assert h.rollout_recorded() == ((STEPS - 1 + stride - 1) // stride, STEPS - 1)
            out.append(h.rollout_trace())
        finally:
            h.close()
    assert out[1]["act"].shape[0] == 3 and all(_eq(out[1][f], out[0][f][::3]) for f in out[0])
    assert np.any(out[1]["hits"] >= 0) and np.all(np.isfinite(out[1]["queue"]))


def test_the_chain_kernel_needs_no_scratch(built_library):
    """the new kernel's row of profiles/kernel_resources.py (the helper tests/test_abi.py uses): no scratch, no LDS, no AGPRs"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "profiles"))
    import kernel_resources
    rows = [r for r in kernel_resources.kernel_table() if "mpmpc_record_chain_kernel" in r["name"]]
    assert len(rows) == 1, [r["name"] for r in rows]
    print("mpmpc_record_chain_kernel: %s" % rows[0])
    assert rows[0]["scratch"] == 0 and rows[0]["lds"] == 0 and rows[0]["agpr"] == 0


def test_batchmpc_refuses_a_scan_without_a_localiser():
    """ValueError before any device call: the stand-in's handle fails on every use"""
    import types
    from MPC import BatchMPC

    class NoDevice:
        def __getattr__(self, name):
            raise AssertionError("device call: " + name)
    bm = BatchMPC.__new__(BatchMPC)
    bm._path, bm.corridor_cols, bm.handle = types.SimpleNamespace(), 30, NoDevice()
    with pytest.raises(ValueError, match="needs a localiser"):
        bm.rollout(np.zeros(2), np.zeros((2, 3)), 1, record=dict(chain=True, scan=True))
    with pytest.raises(AssertionError, match="device call"):      # (without the scan the argument checks pass)
        bm.rollout(np.zeros(2), np.zeros((2, 3)), 1, record=dict(chain=True))


@pytest.mark.gpu
def test_batchmpc_records_the_chain():
    """BatchMPC.rollout(record=dict(chain=True, scan=True)) with a plant, an estimator and a localiser: the trace holds the
    chain's keys, its last record is what the getters of the same call return, and a following unrecorded rollout is bit-equal
    to a controller that never recorded"""
    from MPC import BatchMPC
    from lidar_model import LidarModel
    from scipy import sparse
    import mpmpc_testlib as T
    m, rp, car = T.build_world(obstacles=False)
    Q, R, QN = sparse.diags([1.0, 0.0, 0.0]), sparse.diags([0.5, 0.0]), sparse.diags([1.0, 0.0, 0.0])
    ic = {'umin': np.array([0.0, -np.tan(0.66) / car.length]), 'umax': np.array([1.0, np.tan(0.66) / car.length])}
    sc = {'xmin': np.array([-np.inf] * 3), 'xmax': np.array([np.inf] * 3)}
    Bm, steps = 8, 6
    w, s0, poses = TD._starts(Bm, 48, last=160)
    plant = Plant(speed_gain=0.97, speed_lag=0.8, position_noise=0.03, heading_noise=0.05, seed=SEED)
    est = Estimator.matched(plant, seed=5)
    lidar = LidarModel(270, 0.8, 3.0)
    loc = Localiser(lidar, 6, 1, 1, 1, 0.01, min_hits=5, sigma_r=0.002, seed=4)

    def make():
        return BatchMPC(car, N, Q, R, QN, sc, ic, 4.0, max_batch=Bm, corridor="device")
    bm = make()
    try:
        with pytest.raises(ValueError, match="needs a localiser"):
            bm.rollout(s0, poses, steps, plant=plant, record=dict(scan=True))
        out = bm.rollout(s0, poses, steps, plant=plant, estimator=est, localiser=loc, record=dict(chain=True, scan=True))
        tr = out["trace"]
        assert set(tr) == set(OLD[:8]) | set(FIELDS) and tr["ranges"].shape == (steps, Bm, loc.angles.size)
        on = dict(plant=True, delay=False, estimator=True, localiser=True)
        got = {**out["plant"], **out["estimator"], **out["localiser"]}      # (the statistics' names collide; no chain field's does)
        want = expected_chain(PLANT | DELAY | EST | FIX | SCAN, on, tr["alive"][-2], got, loc.angles.size)
        assert (tr["alive"][-2] == 1).any() and all(_eq(tr[f][-1], v) for f, v in want.items())
        again = bm.rollout(s0, poses, steps, plant=plant, estimator=est, localiser=loc)
        assert "trace" not in again and all(_eq(again[f], out[f]) for f in TD.KEYS)
    finally:
        bm.close()
