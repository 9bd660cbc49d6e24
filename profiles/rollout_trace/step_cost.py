"""Per-step time of the device rollout with the recorder (mpmpc_rollout_record) off, with the basic fields and with all.

    python profiles/rollout_trace/step_cost.py [--quick] [--parent DIR] [--out FILE]

Sim_Track, N = 30, shared corridor table, cars spread over the path, B = 1 024 and 8 192.  Cases:
    parent   the library of the parent commit (--parent DIR: a directory that holds that commit's mpmpc.py and
             csrc/libmpmpc.so), which has no recorder
    off      this tree, recording off - must launch what `parent` launches
    basic    this tree, s / pose / wp_id / x0 / u / status / counter / alive recorded (88 B per car and step)
    all      ... plus plan, predicted path and corridor row (1 496 B per car and step)
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
import scenarios  # noqa: E402


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def main():
    quick = "--quick" in sys.argv
    parent = arg("--parent")
    out = arg("--out")
    cases = [("off", mpmpc, None), ("basic", mpmpc, {}), ("all", mpmpc, dict(plan=True, prediction=True, rows=True))]
    if parent:
        spec = importlib.util.spec_from_file_location("mpmpc_parent", os.path.join(parent, "mpmpc.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        cases.insert(0, ("parent", mod, None))
    g1 = np.load(os.path.join(ROOT, "tests", "golden", "g1_path_sim_track.npz"))
    g3 = np.load(os.path.join(ROOT, "tests", "golden", "g3_corridor.npz"))
    tr = scenarios.sim_track()
    N = 30
    cum = np.cumsum(g1["segment_lengths"])
    warmup, steps, repeats = (3, 20, 3) if quick else (10, 150, 9)
    lines = []
    for B in (1024, 8192):
        rng = np.random.default_rng(B)
        starts = rng.integers(0, g1["x"].size, B)
        poses = np.stack([g1["x"][starts], g1["y"][starts], g1["psi"][starts]], 1)
        handles = {}
        for name, mod, rec in cases:
            Q, R, QN = scenarios.WEIGHTS["stock"]        # (tests/mpmpc_testlib.stock_config, through the case's own module)
            h = mod.Handle(mod.make_config(N, Q, R, QN, scenarios.XMIN, scenarios.XMAX, scenarios.UMIN, scenarios.UMAX,
                                           scenarios.AY_MAX, scenarios.CAR_LENGTH, circular=True, max_batch=B))
            h.set_path(tr.kappa, tr.v_ref, tr.ds_next)
            h.set_corridor(g3["ub_obstacles"], g3["lb_obstacles"])
            h.set_path_geometry(g1["x"], g1["y"], g1["psi"], g1["border_ub"], g1["border_lb"])
            if rec is not None:
                h.rollout_record(warmup + steps, B=B, **rec)
            handles[name] = h
        times = {name: [] for name, _, _ in cases}
        final = {}
        for _ in range(repeats):
            for name, _, _ in cases:
                h = handles[name]
                h.rollout_init(0.05, cum, cum[starts], poses)
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
