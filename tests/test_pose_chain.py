"""The pose chain of a rollout step: which stage reads which pose (csrc/mpmpc_rollout_step.hpp: measured_pose, localise_pose and
the pointer choices of enqueue_delay_predict / enqueue_localise; DESIGN.md section 4, "A rollout step", rows 4 to 5).  Four
features stand between the car's true pose and the pose the controller plans on - K3n's measurement (plant), K3l's fix
(localiser), K3e's estimate (estimator), K3d's prediction (delay) - and the highest one that is on feeds the next.  Every
buffer holds a plausible pose a few millimetres from the right one, so a swapped pointer is silent in every per-feature test.

The law is written ONCE here, as a table (SOURCES), not copied from the C++.  One function, compose, runs the existing twins
(Plant.measure, tests/emul_localiser, tests/emul_estimator, tests/emul_delay, delay.current_waypoint + t2s) on the source the
table names, for any of the 16 combinations of (plant, localiser, estimator, delay).

CPU: the separations of the candidate sources in an open loop of the twins alone (the condition that makes the GPU half mean
something, asserted); the step verifier of the GPU half against a stand-in fleet made of the twins - it passes on the table's
wiring and fails on every single swapped source.  GPU: one step per call on three fleets, the device's own intermediate
outputs fed back to compose so that nothing accumulates; every stage within its one-step bound on the right source and - the
negative control - outside it on every other candidate that lies more than SEP away; the consumers of the true pose (lidar,
audit, traffic, the plant's statistics); and which refusal of plan_step wins when two apply."""
import collections
import itertools

import numpy as np
import pytest

import mpmpc
import delay_twin
import estimator_twin
import localiser_twin
import scenarios
import twins
import test_delay as TD          # (its Sim_Track handles, paths, starts and K3d's twin call)
import test_estimator as TE      # (TwinCar around es_emu_step, the noisy plant)
import test_lidar as TL          # (the lidar twin's scans)
import test_localiser as TLc     # (the step fleets, K3l's twin call)
import test_traffic as TT        # (K0t's law)
from delay import current_waypoint, t2s
from estimator import Estimator
from estimator import fresh as es_fresh
from localiser import Localiser
from localiser import fresh as lc_fresh
from plant import Plant

E_ARG, E_STATE = -1, -3
TS, L_CAR = TD.TS, TD.L_CAR
_same_bits, _in_flight, _code = TD._same_bits, TD._in_flight, TD._code
ES_STATS = ("err2_max", "err2_sum", "meas2_sum", "head2_sum")      # (es_emu_step's order)

# ---------------------------------------------------------------------------------------------------------- the law
# stage -> its candidate sources, the first one whose feature is on is the one it reads.  This table is the only statement of
# the choice in this module; compose and every assertion go through source() / wrong_sources().
SOURCES = {
    "K3e": ("fix", "meas", "true"),                    # what the filter measures (z)
    "K3d": ("est", "fix", "meas", "true"),             # what the prediction starts from
    "K3a": ("pred", "est", "fix", "meas", "true"),     # what the controller localises on (with "pred": at pred_s, else at s)
}
# these read the true pose whatever is on: K3n (the plant measures the car), K0l (the localiser's own scan), K0f (the audit),
# K0t (traffic), K0s (perception) and the plant's statistics
TRUE_POSE = ("K3n", "K0l", "K0f", "K0t", "K0s", "plant statistics")
MADE_BY = dict(true=None, meas="plant", fix="localising", est="estimating", pred="delaying")      # candidate -> its feature
# What an assertion on a stage rules out: every OTHER candidate of its row that exists in the combination (a candidate above
# the source cannot exist - its feature would be on and it would be the source), e.g. K3d with everything on reads est and
# must not have read fix, meas or the true pose; K3e over a localiser reads fix and must not have read meas or the true pose.
Combo = collections.namedtuple("Combo", "plant localising estimating delaying")
COMBOS = [Combo(*bits) for bits in itertools.product((False, True), repeat=4)]
SEP = 1e-5      # m and rad: two candidates count as apart when their positions AND their headings differ by more than this
T2S_TOL = 1e-13      # tests/test_plant.py's bound for t2s (test_consumers_keep_the_true_pose)
ULP4 = 4 * 2.0 ** -52


def _name(combo):
    return "+".join(f for f in Combo._fields if getattr(combo, f)) or "none"


def _exists(combo, cand):
    return MADE_BY[cand] is None or getattr(combo, MADE_BY[cand])


def source(stage, combo):
    return next(c for c in SOURCES[stage] if _exists(combo, c))


def wrong_sources(stage, combo):
    return [c for c in SOURCES[stage] if _exists(combo, c) and c != source(stage, combo)]


def stages(combo):
    return [s for s, f in (("K3e", "estimating"), ("K3d", "delaying"), ("K3a", None)) if f is None or getattr(combo, f)]


def _sep(a, b):
    """how far two candidate poses are apart: the smaller of the position's and the heading's difference.  Both must exceed SEP
    for a pair to count: K3a's e_psi sees the heading alone, meas2_sum and e_y the position alone."""
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(min(np.max(np.abs(a[:2] - b[:2])), abs(a[2] - b[2])))


# ------------------------------------------------------------------------------------------------------ the composer
class Chain:
    """What compose needs of a fleet: the path (a delay.Path), the assumed delays c [B], the settings of the features that may be
    on, which cars' routes are open, and the twins.  world: (grid, origin, res) for K3l's twin, which only the CPU half runs."""

    def __init__(self, path, B, c, plant=None, loc=None, est=None, N=10, circular=None, world=None):
        self.path, self.B, self.c, self.N = path, int(B), np.asarray(c, int), int(N)
        self.plant, self.loc, self.est = plant, loc, est
        self.circular = np.ones(self.B, bool) if circular is None else np.asarray(circular, bool)
        self.es_twin, self.dl_twin = estimator_twin.estimator(), delay_twin.delay()
        self.cars = None if est is None else [TE.TwinCar(self.es_twin, est.car(i)) for i in range(self.B)]
        self.world = world
        if world is not None and loc is not None:
            self.lc_twin, self.lidar = localiser_twin.localiser(), twins.lidar()
            self.field = TLc._twin_field(self.lc_twin, world[0], loc.D)

    def scan(self, poses):
        """K0l's twin on the base map"""
        grid, origin, res = self.world
        return TL._twin_scan(self.lidar, grid, origin, res, poses, self.loc.angles, self.loc.range)[0]

    def k3l(self, k, i, ranges, pose, cmd, prev):
        grid, origin, res = self.world
        return TLc._twin_step(self.lc_twin, self.loc, i, k, grid, self.field, origin, res, ranges, pose, cmd, {f: v[i] for f, v in prev.items()})

    def k3e(self, k, i, z, pose, cmd, prev):
        car = self.cars[i]
        car.est[:], car.cov[:], car.primed.value = prev["est"][i], prev["cov"][i], int(prev["primed"][i])
        car.st[:] = [prev[f][i] for f in ES_STATS]
        car.used.value, car.steps.value = int(prev["used"][i]), int(prev["steps"][i])
        car.step(k, z, pose, cmd)
        return dict(est=car.est.copy(), cov=car.cov.copy(), used=car.used.value, steps=car.steps.value, cmd=np.array(cmd, float),
                    **dict(zip(ES_STATS, car.st.copy())))

    def k3d(self, i, pose, s, q, c=None):
        wp, pp, ps, now, _ = TD._twin_predict(self.dl_twin, self.path, i, self.c[i] if c is None else c, q, pose, s)
        return dict(wp=wp, pred_pose=pp, pred_s=float(ps), now=now)

    def k3a(self, i, pose, s):
        first, n = self.path.car(i)
        wp = current_waypoint(self.path.cum[first:first + n], float(s))
        if wp < 0:
            return dict(wp=-1)
        r = first + wp
        pose = tuple(float(v) for v in pose)
        return dict(wp=wp, x0=np.array(t2s(pose, self.path.x[r], self.path.y[r], self.path.psi[r])),
                    ended=bool(not self.circular[i] and wp + self.N >= n))


def compose(ch, combo, k, i, found, prev, given=None, wiring=None, only=None):
    """What every stage of step k must produce for car i, each from the source the table names.
    found: what the step found - pose [B, 3] (true), s [B], u [B, 2] (the last step's command), queue [B, 8, 2] (the register
    before the step), meas_want [B, 3] (Plant.measure of pose; with a plant);  prev: dict(es=, lc=) the filter's and the
    localiser's state after the last step (fresh's keys);  given: the candidates a device already produced, by name (meas,
    fix, est, pred [B, 3], pred_s [B]) - a given candidate replaces compose's own, so that a stage is judged on the inputs the
    device had; nothing given: the open loop of the twins;  wiring: {stage: candidate} overrides the table (the negative
    control; "K3a.s": "s" localises at s under a delay, "K0l": the pose the localiser scans from);  only: that stage alone.
    -> (out, cand): out[stage] the stage's outputs, cand the candidate poses of the car by name."""
    given, wiring = given or {}, wiring or {}

    def pick(stage):
        return wiring.get(stage) or source(stage, combo)

    def wanted(stage):
        return only is None or only == stage
    cand, out = {"true": found["pose"][i]}, {}
    cmd = found["queue"][i, ch.c[i]] if combo.delaying else found["u"][i]      # the command believed executed in the last step
    if combo.plant:
        out["K3n"] = found["meas_want"][i]
        cand["meas"] = given["meas"][i] if "meas" in given else out["K3n"]
    if combo.localising:
        if "fix" in given:
            cand["fix"] = given["fix"][i]
        else:
            ranges = prev["lc"]["ranges"][i]
            if ch.loc.scheduled(k):
                ranges = ch.scan(cand[wiring.get("K0l", "true")])[0]
            out["K3l"] = ch.k3l(k, i, ranges, found["pose"][i], cmd, prev["lc"])
            cand["fix"] = out["K3l"]["fix"]
    if combo.estimating:
        if wanted("K3e"):
            out["K3e"] = ch.k3e(k, i, cand[pick("K3e")], found["pose"][i], cmd, prev["es"])
        cand["est"] = given["est"][i] if "est" in given else out["K3e"]["est"]
    s_loc = found["s"][i]
    if combo.delaying:
        if wanted("K3d"):
            out["K3d"] = ch.k3d(i, cand[pick("K3d")], found["s"][i], found["queue"][i])
        cand["pred"] = given["pred"][i] if "pred" in given else out["K3d"]["pred_pose"]
        if wiring.get("K3a.s") != "s":
            s_loc = given["pred_s"][i] if "pred_s" in given else out["K3d"]["pred_s"]
    if wanted("K3a"):
        out["K3a"] = ch.k3a(i, cand[pick("K3a")], s_loc)
    return out, cand


# ------------------------------------------------------------------------------------------- one step against compose
def _tol_k3e(cmd):
    """test_k3e_matches_the_twin_step_by_step's bound: 1e-14 for the arithmetic both sides round alike plus 4 ulp of cos / sin /
    tan through the time update's coefficients Ts v (position), Ts v / L (heading); the covariance: twice Ts v"""
    v = abs(float(cmd[0]))
    return 1e-14 + ULP4 * TS * v * (1.0 + 1.0 / L_CAR), 1e-14 + 2 * ULP4 * TS * v


def _tol_k3d(ch, i, pose, s, q):
    """K3d's one-call bound, K3e's per-step term summed over the c predicted steps.  A predicted step j drives the command
    q[j] (the oldest in flight first) through the nominal model: pose += Ts v (cos psi, sin psi, tan(delta) / L) - the device's
    cos / sin / tan against the host's, 4 ulp of a result below 1, is Ts |v_j| on the position and Ts |v_j| / L on the
    heading, as in K3e; what a heading that differs by that much moves the next step's cos / sin by is second order (1e-16
    times Ts v) and inside the 1e-14 for the arithmetic.  pred_s += Ts g v cos(e_psi), g = 1 / (1 - e_y kappa), with (e_y, e_psi)
    from t2s at the step's waypoint: t2s may differ by T2S_TOL on either (tests/test_plant.py's bound), cos by 4 ulp, so the
    step's term is Ts |v_j| g (4 ulp + T2S_TOL (1 + g |kappa|)); g and kappa are those of the twin's own intermediate states
    (the prediction cut after j steps).  -> (tolerance of pred_pose, tolerance of pred_s)"""
    c = int(ch.c[i])
    tol_p = tol_s = 1e-14
    first, n = ch.path.car(i)
    for done in range(c):
        j = c - 1 - done      # the command of the (done + 1)-th predicted step
        v = abs(float(q[j, 0]))
        part = ch.k3d(i, pose, s, q, c=done) if done else dict(pred_pose=np.asarray(pose, float), pred_s=float(s))
        at = ch.k3a(i, part["pred_pose"], part["pred_s"])
        if at["wp"] < 0:
            break
        kappa = abs(float(ch.path.kappa[first + at["wp"]]))
        g = abs(1.0 / (1.0 - at["x0"][0] * kappa))
        tol_p += ULP4 * TS * v * (1.0 + 1.0 / L_CAR)
        tol_s += TS * v * g * (ULP4 + T2S_TOL * (1.0 + g * kappa))
    return tol_p, tol_s


def _differences(stage, want, dev, i, ch, found, source_pose):
    """-> (the stage's differences against the device's outputs for car i as {what: (difference, tolerance)}, its exact
    mismatches as a list of names).  dev: dict(before=, state=, es=, dl=, es_prev=, dl_prev=) of the step."""
    diffs, wrong = {}, []
    if stage == "K3e":
        es = dev["es"]
        tol_e, tol_c = _tol_k3e(want["cmd"])
        diffs["est"] = (float(np.max(np.abs(want["est"] - es["est"][i]))), tol_e)
        diffs["cov"] = (float(np.max(np.abs(want["cov"] - es["cov"][i]))), tol_c)
        for f in ES_STATS:
            diffs[f] = (abs(float(want[f]) - float(es[f][i])), 1e-14)
        wrong += [f for f in ("used", "steps") if want[f] != es[f][i]]
    elif stage == "K3d":
        dl = dev["dl"]
        if want["wp"] < 0:      # s past the end: the prediction is the input, `now` is not written
            if not (_same_bits(dl["pred_pose"][i], source_pose) and dl["pred_s"][i] == found["s"][i]):
                wrong.append("pred passed through")
            if dev["dl_prev"] is not None and not _same_bits(dl["now"][i], dev["dl_prev"]["now"][i]):
                wrong.append("now kept")
        else:
            tol_p, tol_s = _tol_k3d(ch, i, source_pose, found["s"][i], found["queue"][i])
            diffs["pred_pose"] = (float(np.max(np.abs(want["pred_pose"] - dl["pred_pose"][i]))), tol_p)
            diffs["pred_s"] = (abs(want["pred_s"] - float(dl["pred_s"][i])), tol_s)
            diffs["now"] = (float(np.max(np.abs(want["now"][:2] - dl["now"][i, :2]))), T2S_TOL)
            if want["now"][2] != dl["now"][i, 2]:
                wrong.append("now kappa")
    else:
        st, before = dev["state"], dev["before"]
        if want["wp"] < 0:      # lap finished: alive 0, nothing written
            if not (st["alive"][i] == 0 and st["wp_id"][i] == before["wp_id"][i] and _same_bits(st["x0"][i], before["x0"][i])):
                wrong.append("lap finished")
        else:
            if st["wp_id"][i] != want["wp"]:
                wrong.append("wp_id")
            if want["ended"] and st["alive"][i] != -2:
                wrong.append("open end")
            diffs["x0"] = (float(np.max(np.abs(want["x0"] - st["x0"][i, :2]))), T2S_TOL)
    return diffs, wrong


def _violated(diffs, wrong):
    return bool(wrong) or any(not d <= tol for d, tol in diffs.values())


class Tally:
    """what a run measured: the worst difference per (stage, output), the largest tolerance used, the negative controls counted
    per (stage, wrong candidate) and the pairs left out because the candidates were not SEP apart"""

    def __init__(self):
        self.worst, self.tol_max = collections.defaultdict(float), 0.0
        self.ruled_out, self.too_close = collections.Counter(), collections.Counter()
        self.checked = collections.Counter()

    def report(self, what):
        print("pose chain, %s: checked %s" % (what, dict(self.checked)))
        print("  worst differences %s; largest tolerance %.2e" % ({"%s.%s" % k: "%.2e" % v for k, v in sorted(self.worst.items())}, self.tol_max))
        print("  wrong sources ruled out %s; pairs closer than SEP %s" % ({"%s<-%s" % k: v for k, v in sorted(self.ruled_out.items())},
                                                                         {"%s<-%s" % k: v for k, v in sorted(self.too_close.items())}))


def verify_step(ch, combo, k, dev, prev, tally, scan):
    """One step of a fleet against compose.  dev: before (pose, s, u, alive, wp_id, x0, queue as the step found them), state and
    the getters after it (plant, lc, es, dl; None where the feature is off), and the getters before it (*_prev; None before
    the first step);  prev: dict(es=) the filter's state with `primed`;  scan(poses) -> K0l's ranges [B, n_beams]."""
    before, st = dev["before"], dev["state"]
    on = before["alive"] == 1
    off = ~on
    found = dict(before)
    given = {}
    if combo.plant:
        found["meas_want"] = ch.plant.measure(k, before["pose"])
        assert _same_bits(dev["plant"]["meas"][on], found["meas_want"][on]), (k, "K3n measures the true pose")
        given["meas"] = dev["plant"]["meas"]
        tally.checked["K3n"] += int(on.sum())
    if combo.localising:
        given["fix"] = dev["lc"]["fix"]
        if ch.loc.scheduled(k):
            assert _same_bits(dev["lc"]["ranges"][on], scan(before["pose"])[on]), (k, "K0l scans from the true pose")
            tally.checked["K0l"] += int(on.sum())
            if combo.plant:      # (ranges are functions of cells: a scan from the measured pose need not differ car by car)
                tally.ruled_out["K0l", "meas"] += int(not _same_bits(dev["lc"]["ranges"][on], scan(dev["plant"]["meas"])[on]))
    if combo.estimating:
        given["est"] = dev["es"]["est"]
    if combo.delaying:
        given["pred"], given["pred_s"] = dev["dl"]["pred_pose"], dev["dl"]["pred_s"]
    for i in np.flatnonzero(on):
        out, cand = compose(ch, combo, k, i, found, prev, given)
        for stage in stages(combo):
            right = source(stage, combo)
            diffs, wrong = _differences(stage, out[stage], dev, i, ch, found, cand[right])
            for what, (d, tol) in diffs.items():
                tally.worst[stage, what] = max(tally.worst[stage, what], d)
                tally.tol_max = max(tally.tol_max, tol)
            assert not _violated(diffs, wrong), (k, i, stage, "reads " + right, diffs, wrong)
            tally.checked[stage] += 1
            for other in wrong_sources(stage, combo):      # the negative control
                if not _sep(cand[right], cand[other]) > SEP or (stage == "K3a" and out[stage]["wp"] < 0):      # (a lap finished: no pose is read)
                    tally.too_close[stage, other] += 1
                    continue
                o2, _ = compose(ch, combo, k, i, found, prev, given, wiring={stage: other}, only=stage)
                d2, w2 = _differences(stage, o2[stage], dev, i, ch, found, cand[other])
                assert _violated(d2, w2), (k, i, stage, "passes on " + other + " as well", d2)
                tally.ruled_out[stage, other] += 1
        if combo.delaying and out["K3a"]["wp"] != ch.k3a(i, cand["pred"], before["s"][i])["wp"]:
            tally.ruled_out["K3a.s", "s"] += 1      # (the waypoint of pred_s is not that of s, and wp_id passed above)
    # cars that are not running keep every field's bits
    for f in ("pose", "s", "u", "x0"):
        assert _same_bits(st[f][off], before[f][off]), (k, f)
    assert np.array_equal(st["wp_id"][off], before["wp_id"][off]) and np.array_equal(st["alive"][off], before["alive"][off]), k
    for name in ("plant", "lc", "es", "dl"):
        if dev.get(name) is not None and dev.get(name + "_prev") is not None:
            for f, v in dev[name].items():
                assert np.array_equal(v[off].view(np.uint8), dev[name + "_prev"][f][off].view(np.uint8)), (k, name, f)


def required(combo):
    """the (stage, wrong candidate) pairs a run of `combo` must rule out at least once.  With a plant (noise and mismatch) every
    candidate differs from every other; without one the true car drives the controller's own model, dead reckoning and the
    filter are exact (test_estimator.py::test_exact_on_the_device) and only the prediction differs from what it starts from."""
    return [(s, w) for s in stages(combo) for w in wrong_sources(s, combo) if combo.plant or source(s, combo) == "pred"]


def verify_run(fleet, ch, combo, steps, what):
    """drive `fleet` (before / step / after: the device, or the stand-in of the twins) one step per call through verify_step"""
    tally = Tally()
    prev = dict(es=es_fresh(ch.B))
    last = {}
    for k in range(steps):
        dev = dict(before=fleet.before(), **{n + "_prev": last.get(n) for n in ("plant", "lc", "es", "dl")})
        fleet.step(k)
        dev.update(fleet.after())
        verify_step(ch, combo, k, dev, prev, tally, fleet.scan)
        on = dev["before"]["alive"] == 1
        if combo.estimating:
            prev["es"] = dict(dev["es"], primed=np.where(on, 1, prev["es"]["primed"]))
        last = {n: dev.get(n) for n in ("plant", "lc", "es", "dl")}
    tally.report(what)
    assert SEP >= 1e6 * tally.tol_max, tally.tol_max
    for pair in required(combo) + [("K3a.s", "s")] * combo.delaying:
        assert tally.ruled_out[pair] > 0, (what, pair, dict(tally.ruled_out), dict(tally.too_close))
    return tally, dev


# ------------------------------------------------------------------------------------------------------------ CPU
CPU = dict(B=6, steps=12, w=np.array([3, 40, 77, 110, 150, 190]))


def _cpu_settings(sigma_r=0.004):
    """test_localiser.py::test_step_twin_equals_numpy's cars and localiser (period 2, range noise); the true car is a mismatched,
    noisy plant; an estimator with per-car periods and dropouts; assumed delays c = i % 3"""
    B = CPU["B"]
    plant = Plant(wheelbase_scale=1.05, speed_gain=1.04, position_noise=0.03, heading_noise=0.05, seed=7, car0=2)
    loc = Localiser(TLc._lidar(61, rng=0.6), D=5, step_cells=1, window=3, headings=1, step_psi=0.01, min_hits=4, sigma_r=sigma_r, period=2,
                    seed=11, car0=3, step0=-1)
    est = Estimator(1e-6, 1e-6, 0.03 ** 2 / 6, 0.05 ** 2 / 6, period=[1 + i % 3 for i in range(B)], drop=0.25, seed=21, car0=9, step0=-3)
    g1, grid, origin, res = TLc._sim_map()
    return Chain(TD._lap(), B, np.arange(B) % 3, plant, loc, est, world=(grid, origin, res))


class TwinFleet:
    """A fleet made of the twins alone, in an open loop with commands fixed in advance: what the device's getters would return
    if its stages were wired as `wiring` says (None: the table).  The true car drives ch.plant's mismatched model whether or
    not the combination has a plant (the plant of a combination is K3n, the measurement)."""

    def __init__(self, ch, combo, wiring=None):
        self.ch, self.combo, self.wiring = ch, combo, wiring
        B, w = ch.B, CPU["w"]
        p = ch.path
        self.pose, self.s = np.stack([p.x[w], p.y[w], p.psi[w]], 1), p.cum[w].copy()
        self.u, self.act, self.queue = np.zeros((B, 2)), np.zeros((B, 2)), _in_flight(B)
        self.alive, self.wp_id, self.x0 = np.ones(B, np.int32), np.zeros(B, np.int32), np.zeros((B, 3))
        self.prev = dict(es=es_fresh(B), lc=lc_fresh(B, ch.loc.angles.size))
        self.dl = dict(queue=self.queue.copy(), pred_pose=np.zeros((B, 3)), pred_s=np.zeros(B), now=np.zeros((B, 3)))
        self.meas, self.out, self.cands = np.zeros((B, 3)), {}, {}

    def scan(self, poses):
        return self.ch.scan(poses)

    def before(self):
        return dict(pose=self.pose.copy(), s=self.s.copy(), u=self.u.copy(), alive=self.alive.copy(), wp_id=self.wp_id.copy(),
                    x0=self.x0.copy(), queue=self.queue.copy())

    def step(self, k):
        ch, combo, B = self.ch, self.combo, self.ch.B
        found = dict(self.before(), meas_want=ch.plant.measure(k, self.pose))
        es, lc = {f: v.copy() for f, v in self.prev["es"].items()}, {f: v.copy() for f, v in self.prev["lc"].items()}
        dl = {f: v.copy() for f, v in self.dl.items()}
        meas = self.meas.copy()
        self.cands = {}
        on = self.alive == 1
        for i in np.flatnonzero(on):
            out, self.cands[i] = compose(ch, combo, k, i, found, self.prev, wiring=self.wiring)
            meas[i] = found["meas_want"][i]
            if combo.localising:
                for f in lc:
                    lc[f][i] = out["K3l"][f]
            if combo.estimating:
                for f in es:
                    es[f][i] = 1 if f == "primed" else out["K3e"][f]
            if combo.delaying:
                for f in ("pred_pose", "pred_s", "now"):
                    if f != "now" or out["K3d"]["wp"] >= 0:
                        dl[f][i] = out["K3d"][f]
            if out["K3a"]["wp"] < 0:      # lap finished: K3a ends the car and writes nothing
                self.alive[i] = 0
            else:
                self.wp_id[i], self.x0[i, :2] = out["K3a"]["wp"], out["K3a"]["x0"]
        self.prev, self.meas = dict(es=es, lc=lc), meas
        cmd = np.stack([np.full(B, 0.6), 0.1 * np.sin(0.3 * k + np.arange(B))], 1)
        drive = self.alive == 1
        pose, s_new, act = ch.plant.drive(k, cmd, self.pose, self.s, self.act, np.zeros((B, 2)), np.zeros(B), L_CAR, TS)
        self.pose, self.s, self.act = (np.where(drive.reshape((B,) + (1,) * (new.ndim - 1)), new, old)
                                       for new, old in ((pose, self.pose), (s_new, self.s), (act, self.act)))
        self.u = np.where(drive[:, None], cmd, self.u)
        self.queue = np.where(drive[:, None, None], np.concatenate([cmd[:, None, :], self.queue[:, :-1]], 1), self.queue)
        self.dl = dict(dl, queue=self.queue.copy())
        self.out = dict(plant=dict(meas=meas) if combo.plant else None, lc=lc if combo.localising else None,
                        es={f: v for f, v in es.items() if f != "primed"} if combo.estimating else None,
                        dl=self.dl if combo.delaying else None)

    def after(self):
        return dict(state=self.before(), **self.out)


def test_the_table_is_a_law():
    """every stage of every combination has exactly one source, it exists, and nothing above it does"""
    for combo in COMBOS:
        for stage, row in SOURCES.items():
            src = source(stage, combo)
            assert _exists(combo, src) and not any(_exists(combo, c) for c in row[:row.index(src)])
            assert set(wrong_sources(stage, combo)) == {c for c in row[row.index(src) + 1:] if _exists(combo, c)}
        assert source("K3e", combo) == ("fix" if combo.localising else "meas" if combo.plant else "true")
    assert all(r[-1] == "true" for r in SOURCES.values()) and len(COMBOS) == 16 and not set(TRUE_POSE) & set(SOURCES)
    full = Combo(True, True, True, True)
    assert [source(s, full) for s in ("K3e", "K3d", "K3a")] == ["fix", "est", "pred"] and len(required(full)) == 2 + 3 + 4


def test_the_candidates_are_apart():
    """The condition of the GPU half, on the twins alone: 12 steps, 6 cars, all 16 combinations.  From step 1 on (step 0 primes:
    fix = est = the true pose by design) every pair of candidates a stage could confuse differs by more than SEP - in position
    AND in heading - on at least half of the (car, step) pairs, and SEP is at least 1e6 times the largest tolerance of the GPU
    half (asserted there from the tolerances it used: verify_run).  The prediction equals what it starts from on the cars that
    assume no delay, a third of the fleet."""
    ch = _cpu_settings()
    seps = collections.defaultdict(list)
    for combo in COMBOS:
        fleet = TwinFleet(ch, combo)
        for k in range(CPU["steps"]):
            fleet.step(k)
            if k == 0:
                continue
            for cand in fleet.cands.values():
                for stage in stages(combo):
                    for other in wrong_sources(stage, combo):
                        seps[_name(combo), stage, source(stage, combo), other].append(_sep(cand[source(stage, combo)], cand[other]))
    assert {(k[1], k[3]) for k in seps} == {(s, w) for s, row in SOURCES.items() for w in row[1:]}      # every pair of the table occurs
    lowest_share, lowest_sep = 1.0, np.inf
    for key, v in sorted(seps.items()):
        v = np.array(v)
        counted = v > SEP
        assert v.size > (CPU["steps"] - 1) * (CPU["B"] - 1)      # (the car that starts at waypoint 190 may finish its lap)
        lowest_share, lowest_sep = min(lowest_share, counted.mean()), min(lowest_sep, v[counted].min())
        assert counted.mean() >= 0.5, (key, counted.mean())
    print("candidate separations: %d (combination, stage, source, other) rows; smallest counted separation %.3e (SEP %.0e), smallest "
          "share of pairs counted %.3f" % (len(seps), lowest_sep, SEP, lowest_share))
    assert lowest_share >= 0.5 and lowest_sep > SEP


SWAPS = ([("K3e", "meas"), ("K3e", "true"), ("K3d", "fix"), ("K3d", "meas"), ("K3d", "true"), ("K3a", "est"), ("K3a", "fix"), ("K3a", "meas"),
          ("K3a", "true"), ("K3a.s", "s"), ("K0l", "meas")])


@pytest.mark.parametrize("combo", COMBOS, ids=_name)
def test_the_verifier_fails_on_a_swapped_source(combo):
    """The GPU half's verifier on the stand-in fleet: it passes on the table's wiring - with every required negative control
    counted - and fails on every single swap the combination allows: each stage on each other candidate that exists, K3a
    localising at s in place of pred_s, K0l scanning from the measured pose."""
    ch = _cpu_settings(sigma_r=0.0)
    tally, _ = verify_run(TwinFleet(ch, combo), ch, combo, CPU["steps"], "stand-in, " + _name(combo))
    assert set(tally.ruled_out) >= set(required(combo))
    swaps = [(s, w) for s, w in SWAPS if s in SOURCES and s in stages(combo) and w in wrong_sources(s, combo)]
    swaps += [("K3a.s", "s")] * combo.delaying + [("K0l", "meas")] * (combo.localising and combo.plant)
    for stage, other in swaps:      # (the assertion that fails is the swapped stage's own: the later stages are fed the fleet's outputs)
        with pytest.raises(AssertionError, match="K0l scans from the true pose" if stage == "K0l" else "'%s', 'reads " % stage[:3]):
            verify_run(TwinFleet(ch, combo, wiring={stage: other}), ch, combo, CPU["steps"], "stand-in, %s, %s reads %s" % (_name(combo), stage, other))
    print("swaps caught, %s: %s" % (_name(combo), ["%s<-%s" % sw for sw in swaps]))
    assert len(swaps) == sum(len(wrong_sources(s, combo)) for s in stages(combo)) + combo.delaying + (combo.localising and combo.plant)


# ------------------------------------------------------------------------------------------------------------ GPU
STEPS = 14
GPU_PLANT = dict(seed=7, car0=2, **TE.NOISY)      # gains, offset, wheelbase, lags, rate limit, command noise; 3 cm and 0.05 rad of pose noise


def _gpu_settings(B, path, circular=None):
    plant = Plant(**GPU_PLANT)
    loc = Localiser(TLc._lidar(rng=0.8), D=6, step_cells=1, window=3, headings=1, step_psi=0.01, min_hits=5, period=2, seed=3, car0=1)
    est = Estimator(1e-6, 1e-6, TE.A_XY ** 2 / 6, TE.A_PSI ** 2 / 6, period=[1 + i % 3 for i in range(B)], drop=0.25, seed=21, car0=9, step0=-3)
    return Chain(path, B, np.arange(B) % 3, plant, loc, est, circular=circular)


class DeviceFleet:
    """a handle's rollout behind TwinFleet's interface; discs: the cars have worlds of their own (traffic) that K0l scans"""

    def __init__(self, h, ch, combo, cum, s0, poses, discs=False):
        self.h, self.ch, self.combo, self.discs = h, ch, combo, discs
        B = ch.B
        if combo.plant:
            h.rollout_set_plant(ch.plant.params(B), ch.plant.seed, ch.plant.car0)
        h.rollout_init(TS, cum, s0, poses)
        if combo.delaying:
            c = ch.c.astype(np.int32)
            h.rollout_set_delay(c, c, _in_flight(B))
        if combo.estimating:
            TE._set(h, ch.est, B)
        if combo.localising:
            TLc._set(h, ch.loc, B)
        self.queue = _in_flight(B)
        self.world = TLc._sim_map()[1:]

    def scan(self, poses):
        grid, origin, res = self.world
        return mpmpc.lidar_scan(grid, origin, res, poses, self.ch.loc.angles, self.ch.loc.range, self.h.rollout_obstacles() if self.discs else None)

    def before(self):
        st = self.h.rollout_state()
        return dict(st, queue=self.queue.copy())

    def step(self, k):
        self.h.rollout_step(1)

    def after(self):
        h, combo = self.h, self.combo
        out = dict(state=h.rollout_state(), plant=h.rollout_plant() if combo.plant else None, lc=h.rollout_localiser() if combo.localising else None,
                   es=h.rollout_estimator() if combo.estimating else None, dl=h.rollout_delay() if combo.delaying else None)
        if combo.delaying:
            self.queue = out["dl"]["queue"]
        return out


def _fleet(name):
    """-> (handle, chain, cum, s0, poses)"""
    N = 10
    if name == "two_routes":      # half of the cars on the open second route; car 1 starts 15 waypoints from its end
        B = 16
        h, cum, s0, poses = TLc._step_setup("two_routes", B, N)
        cat, first, circ = TD._two_routes()
        route = np.arange(B) % 2
        g = first[1] + 85
        s0, poses = s0.copy(), poses.copy()
        s0[1], poses[1] = cat["cum_lengths"][g], (cat["x"][g] + 0.00113, cat["y"][g] - 0.00071, cat["psi"][g])
        return h, _gpu_settings(B, TD._route_path(cat, first, route), circular=circ[route] != 0), cum, s0, poses
    if name == "big":      # a 256-thread block of K3a, K3e and K3d ends inside the fleet
        B = 272
        h = TLc._handle(N, B)
        _, s0, poses = TD._starts(B, 49, last=160)
        return h, _gpu_settings(B, TD._lap()), TLc._cum(), s0, poses + np.array([0.00113, -0.00071, 0.0])
    B = 16
    h, cum, s0, poses = TLc._step_setup("plain", B, N)      # (its car 0 starts at waypoint 198 and finishes the lap)
    return h, _gpu_settings(B, TD._lap()), cum, s0, poses


def _device_run(name, combo):
    h, ch, cum, s0, poses = _fleet(name)
    try:
        tally, dev = verify_run(DeviceFleet(h, ch, combo, cum, s0, poses), ch, combo, STEPS, "%s, %s" % (name, _name(combo)))
    finally:
        h.close()
    assert tally.checked["K3a"] > STEPS * ch.B // 2
    return tally, dev


@pytest.mark.gpu
@pytest.mark.parametrize("combo", COMBOS, ids=_name)
def test_sim_fleet_reads_its_sources(combo):
    """B = 16, 14 steps, every combination; the bounds are _tol_k3e's, _tol_k3d's (derived there) and T2S_TOL.  Measured on an
    MI355X over all runs of this module (printed by Tally.report; DESIGN.md, "A rollout step"): est 4.4e-16, cov 6.8e-21, meas2_sum
    0.0, pred_pose 4.4e-16, pred_s 0.0, now and x0 1.4e-17; the largest tolerance used was 3.3e-13 (pred_s)."""
    tally, dev = _device_run("sim", combo)
    assert dev["state"]["alive"][0] != 1      # the car that finished its lap


@pytest.mark.gpu
@pytest.mark.parametrize("combo", [c for c in COMBOS if c.delaying or c.localising], ids=_name)
def test_two_routes_fleet_reads_its_sources(combo):
    """every combination with a delay or a localiser, circular=False, every car on its own slice of the tables; a car reaches
    the open end of the second route within the run"""
    tally, dev = _device_run("two_routes", combo)
    assert dev["state"]["alive"][1] in (0, -2), dev["state"]["alive"]


@pytest.mark.gpu
def test_big_fleet_reads_its_sources():
    """all four features on, B = 272: the second block of K3a, K3e and K3d has 16 cars"""
    combo = Combo(True, True, True, True)
    tally, dev = _device_run("big", combo)
    assert tally.checked["K3e"] > STEPS * 272 // 2 and (dev["state"]["alive"][256:] == 1).any()


@pytest.mark.gpu
def test_consumers_keep_the_true_pose_under_the_whole_chain():
    """Sim_Track with all four features on, the audit and traffic in one group: beside the chain itself, K0f's verdicts are
    mpmpc.footprint_audit's of the pose the step found, K0t's slots sit at the cells of the neighbours' true poses and the plant's
    ey_sq grows by the lateral offset of the true pose from the waypoint the car is at.  The same quantities of the measured
    pose differ (counted)."""
    combo = Combo(True, True, True, True)
    h, ch, cum, s0, poses = _fleet("sim")
    B, S, length, width, reach = ch.B, 2, 0.12, 0.06, 0.2
    grid, origin, res = TLc._sim_map()[1:]
    group, rad, frame = np.zeros(B, np.int32), np.ones(B, np.int32), TT.Frame("sim")
    h.rollout_set_audit(1, length, width, reach)
    h.rollout_set_traffic(group, rad, S)
    fleet = DeviceFleet(h, ch, combo, cum, s0, poses, discs=True)
    tally, prev, last = Tally(), dict(es=es_fresh(B)), {}
    lap = TD._lap()
    seen = collections.Counter()
    for k in range(STEPS):
        dev = dict(before=fleet.before(), **{n + "_prev": last.get(n) for n in ("plant", "lc", "es", "dl")})
        fleet.step(k)
        dev.update(fleet.after())
        verify_step(ch, combo, k, dev, prev, tally, fleet.scan)
        before, st, pl = dev["before"], dev["state"], dev["plant"]
        on = before["alive"] == 1
        discs, aud = h.rollout_obstacles(), h.rollout_audit()
        # K0t
        want = TT._law(before["pose"], before["alive"], group, rad, S, -1, frame)
        assert all(np.array_equal(discs[b], want[b]) for b in np.flatnonzero(on)), k
        seen["K0t, measured differs"] += int(not np.array_equal(want, TT._law(pl["meas"], before["alive"], group, rad, S, -1, frame)))
        # K0f: the cars that were audited and drove on
        drove = on & (st["alive"] == 1)
        contact, clearance = mpmpc.footprint_audit(grid, origin, res, before["pose"], length, width, reach, discs)
        assert np.array_equal(aud["last_contact"][drove], contact[drove]) and _same_bits(aud["last_clearance"][drove], clearance[drove]), k
        other = mpmpc.footprint_audit(grid, origin, res, pl["meas"], length, width, reach, discs)[1]
        seen["K0f, measured differs"] += int(not _same_bits(other[drove], clearance[drove]))
        # the plant's statistics: e of the true pose at the waypoint the car is at (the waypoint of s: K3d's now_wp)
        old = dev["plant_prev"] or dict(ey_sq=np.zeros(B), steps=np.zeros(B, np.int32))
        for i in range(B):
            if pl["steps"][i] == old["steps"][i]:
                assert pl["ey_sq"][i] == old["ey_sq"][i], (k, i)
                continue
            w = current_waypoint(lap.cum, float(before["s"][i]))
            e = [t2s(tuple(float(v) for v in p[i]), lap.x[w], lap.y[w], lap.psi[w])[0] for p in (before["pose"], pl["meas"])]
            assert on[i] and abs((pl["ey_sq"][i] - old["ey_sq"][i]) - e[0] * e[0]) <= T2S_TOL, (k, i)
            seen["ey_sq"] += 1
            seen["ey_sq, measured differs"] += int(abs(e[1] * e[1] - e[0] * e[0]) > 1e6 * T2S_TOL)
        prev["es"] = dict(dev["es"], primed=np.where(on, 1, prev["es"]["primed"]))
        last = {n: dev.get(n) for n in ("plant", "lc", "es", "dl")}
    h.close()
    tally.report("sim with audit and traffic")
    print("  consumers of the true pose: %s" % dict(seen))
    assert seen["ey_sq"] > STEPS * B // 2
    for what in ("K0t", "K0f", "ey_sq"):
        assert seen[what + ", measured differs"] > 0, what


@pytest.mark.gpu
def test_the_first_refusal_that_applies_wins():
    """plan_step's order (csrc/mpmpc_rollout_step.hpp; DESIGN.md, "A rollout step"): for every adjacent pair of refusals that can
    apply at once both faults are set, the call returns the earlier one's code and message, and - the earlier fault mended -
    the later one's.  Returned error codes: no step runs, the state keeps its bits."""
    N, B = 10, 8
    g1, grid, origin, res = TLc._sim_map()
    cum = TLc._cum()
    _, s0, poses = TD._starts(B, 50, last=160)
    tr = scenarios.sim_track()
    loc = Localiser(TLc._lidar(rng=0.8), 6, 1, 3, 1, 0.01, min_hits=5)
    est = Estimator(1e-6, 1e-6, 1e-4, 1e-4)
    zero, eight = np.zeros(B, np.int32), np.full(B, 8, np.int32)

    def refused(h, code, word):
        with pytest.raises(mpmpc.MpmpcError) as err:
            h.rollout_step(1)
        assert _code(err) == code and word in str(err.value), (word, str(err.value))

    def same_state(h, want):
        got = h.rollout_state()
        assert all(np.array_equal(got[f], want[f]) for f in TD.KEYS)
    # the four settings' B: all set for 8 cars, the rollout holds 5
    h = TLc._handle(N, B)
    h.rollout_set_plant(Plant().params(B))
    h.rollout_init(TS, cum, s0, poses)
    h.rollout_set_delay(zero, zero)
    TE._set(h, est, B)
    TLc._set(h, loc, B)
    h.rollout_init(TS, cum, s0[:5], poses[:5])
    want = h.rollout_state()
    refused(h, E_STATE, "the plant was set for another number of cars")            # the plant's B before the delay's
    h.rollout_set_plant(None)
    refused(h, E_STATE, "the delay was set for another number of cars")            # the delay's before the estimator's
    h.rollout_set_delay(None)
    refused(h, E_STATE, "the estimator was set for another number of cars")        # the estimator's before the localiser's
    h.rollout_set_estimator(None)
    refused(h, E_STATE, "the localiser was set for another number of cars")
    same_state(h, want)
    # the delay under a lookahead, the estimator and the localiser under an assumed delay of DL_MAX = 8
    h.rollout_init(TS, cum, s0, poses)
    want = h.rollout_state()
    h.rollout_set_delay(eight, eight, _in_flight(B))
    TE._set(h, est, B)
    TLc._set(h, loc, B)
    h.rollout_set_lookahead(tr.ds_next / tr.v_ref, 2)
    refused(h, E_STATE, "lookahead under delay is not supported")                  # ... before the estimator under c = 8
    h.rollout_set_lookahead(None)
    refused(h, E_STATE, "an estimator is in force")                                # the estimator before the localiser
    h.rollout_set_estimator(None)
    refused(h, E_STATE, "a localiser is in force")
    h.rollout_set_delay(None)
    same_state(h, want)
    # the localiser's stale map before the audit: at half the resolution the audit's reach is more than 256 cells
    h.rollout_set_audit(1, 0.12, 0.06, 1.0)
    h.set_map(grid, origin, res / 2)
    refused(h, E_STATE, "changed since mpmpc_rollout_set_localiser")
    h.rollout_set_localiser(0)
    refused(h, E_ARG, "reach plus half the car's diagonal")
    same_state(h, want)
    h.close()
