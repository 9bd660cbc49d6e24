"""Per-step time of the device rollout with the pose chain in the trace (MPMPC_REC_PLANT .. MPMPC_REC_SCAN), step_cost.py's method.

    python profiles/rollout_trace/chain_cost.py [--quick] [--parent DIR] [--out FILE]

Sim_Track on the device's map, N = 30, the corridor built from the map, cars spread over the path, B = 1 024 and 8 192, a
plant (3 cm / 0.05 rad of pose noise, a lag and a gain), an estimator matched to it and a localiser (30 beams of 1 m,
W = T = 1, every step) in force.  Cases:
    parent   the library of the parent commit (--parent DIR: a directory that holds that commit's mpmpc.py and
             csrc/libmpmpc.so), unrecorded, TWICE (parent, parent2): the difference of the two is the run-to-run spread
             the other cases are read against
    off      this tree, recording off - must launch what `parent` launches and end in the same bits
    basic    this tree, s / pose / wp_id / x0 / u / status / counter / alive recorded
    chain    ... plus plant, delay, estimator and fix (the delay's group is empty: no delay is in force)
    scan     ... plus the localiser's scan, 30 ranges per car
Every repeat re-initialises the rollout from the same state, takes `warmup` steps, then times `steps` steps in one
rollout_step call ending in a synchronise; the cases alternate inside a repeat.  One JSON line per case and B: the
median, the fastest and the slowest repeat in ms per step."""
import importlib.util
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in ("multi-purpose-mpc_amd", "tests", "oracle", ""):
    sys.path.insert(0, os.path.join(ROOT, p))

import numpy as np  # noqa: E402

import mpmpc  # noqa: E402
import mpmpc_testlib as T  # noqa: E402
import scenarios  # noqa: E402
from estimator import Estimator  # noqa: E402
from plant import Plant  # noqa: E402


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def main():
    quick = "--quick" in sys.argv
    parent = arg("--parent")
    out = arg("--out")
    cases = [("off", mpmpc, None), ("basic", mpmpc, {}), ("chain", mpmpc, dict(chain=True)), ("scan", mpmpc, dict(chain=True, scan=True))]
    if parent:
        spec = importlib.util.spec_from_file_location("mpmpc_parent", os.path.join(parent, "mpmpc.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        cases = [("parent", mod, None)] + cases + [("parent2", mod, None)]
    g1, grid, origin, res = T.g1_world("sim")
    tr = scenarios.sim_track()
    sm = T.safety_margin("sim")
    N = 30
    cum = np.cumsum(g1["segment_lengths"])
    warmup, steps, repeats = (3, 20, 3) if quick else (10, 150, 9)
    plant = Plant(speed_gain=0.97, speed_lag=0.8, position_noise=0.03, heading_noise=0.05, seed=7)
    est = Estimator.matched(plant, seed=21)
    angles = np.linspace(-2.3, 2.3, 30)
    lines = []
    for B in (1024, 8192):
        rng = np.random.default_rng(B)
        starts = rng.integers(0, g1["x"].size, B)
        poses = np.stack([g1["x"][starts] + 0.00113, g1["y"][starts] - 0.00071, g1["psi"][starts]], 1)
        handles = {}

        def localise(h):
            h.rollout_set_localiser(B, angles=angles, range_m=1.0, D=6, m=1, W=1, T=1, step_psi=0.01, min_hits=5, sigma_r=0.004, period=1, seed=3)
        for name, mod, rec in cases:
            Q, R, QN = scenarios.WEIGHTS["stock"]
            h = mod.Handle(mod.make_config(N, Q, R, QN, scenarios.XMIN, scenarios.XMAX, scenarios.UMIN, scenarios.UMAX,
                                           scenarios.AY_MAX, scenarios.CAR_LENGTH, circular=True, max_batch=B))
            h.set_path(tr.kappa, tr.v_ref, tr.ds_next)
            h.set_map(grid, origin, res)
            h.set_path_geometry(g1["x"], g1["y"], g1["psi"], g1["border_ub"], g1["border_lb"])
            h.build_corridor(N, 2 * sm, sm)
            h.rollout_set_plant(plant.params(B), plant.seed)
            localise(h)
            if rec is not None:
                h.rollout_record(warmup + steps, B=B, **rec)
            handles[name] = h
        times = {name: [] for name, _, _ in cases}
        final = {}
        for _ in range(repeats):
            for name, _, _ in cases:
                h = handles[name]
                h.rollout_init(0.05, cum, cum[starts], poses)
                h.rollout_set_estimator(est.params(B), est.seed)
                localise(h)
                h.rollout_step(warmup)
                h.sync()
                t0 = time.perf_counter()
                h.rollout_step(steps)
                h.sync()
                times[name].append((time.perf_counter() - t0) / steps * 1e3)
                final[name] = h.rollout_state()
        for name, _, _ in cases:
            t = np.array(times[name])
            same = all(np.array_equal(final[name][k], final["off"][k]) for k in ("s", "pose", "cc", "counter", "alive"))
            lines.append(json.dumps(dict(B=B, N=N, case=name, steps=steps, repeats=repeats, ms_per_step_median=round(float(np.median(t)), 5),
                                         ms_per_step_min=round(float(t.min()), 5), ms_per_step_max=round(float(t.max()), 5),
                                         running=int((final[name]["alive"] == 1).sum()), same_final_state_as_off=bool(same))))
            print(lines[-1], flush=True)
        for h in handles.values():
            h.close()
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
