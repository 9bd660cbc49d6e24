"""Per-step time of the device rollout with the pose estimator (K3e): the setting off, and the estimator on under a plant with
pose noise (every car's filter takes its measurement on every step), the method of profiles/delay/delay_timing.py: N = 30,
Sim_Track's free corridor, the default warm start, 5 warm-up steps, then 60 timed steps between two synchronisations; every
variant is repeated, the variants alternating, and the median and the spread over the repeats are printed.

    python profiles/estimator/estimator_timing.py [--parent OTHER/libmpmpc.so] [--repeats 7] [--B 1024 8192]

--parent: a build of another commit's library, loaded into the same process and timed as a further variant (the parent has no
estimator: it is "estimator off" on the older code).  (GPU box)"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for d in ("multi-purpose-mpc_amd", "tests", "oracle"):
    sys.path.insert(0, os.path.join(ROOT, d))
import mpc_np as M                  # noqa: E402
import mpmpc                        # noqa: E402
import mpmpc_testlib as T           # noqa: E402
import scenarios                    # noqa: E402
from estimator import Estimator     # noqa: E402
from plant import Plant             # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--parent", default=None)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--B", type=int, nargs="+", default=[1024, 8192])
args = ap.parse_args()

g1 = np.load(M.GOLDEN + "/g1_path_sim_track.npz")
g3 = np.load(M.GOLDEN + "/g3_corridor.npz")
N, warmup, steps = 30, 5, 60
tr = scenarios.sim_track()
cum = np.cumsum(g1["segment_lengths"])
this_lib = mpmpc.load_library()
plant = Plant(position_noise=0.03, heading_noise=0.05, seed=1)
matched = Estimator.matched(plant)


def load_other(path):
    """another build of the library: every entry point it shares with this one, declared as this one's"""
    import ctypes
    lib = ctypes.CDLL(path)
    for name in mpmpc.EXPORTS:
        if hasattr(lib, name):
            getattr(lib, name).argtypes = getattr(this_lib, name).argtypes
            getattr(lib, name).restype = getattr(this_lib, name).restype
    return lib


parent_lib = load_other(args.parent) if args.parent else None


def handle(lib, B, with_plant):
    mpmpc._lib = lib      # (Handle binds the library it is made with)
    try:
        h = mpmpc.Handle(T.stock_config(N, max_batch=B))
    finally:
        mpmpc._lib = this_lib
    h.set_path(tr.kappa, tr.v_ref, tr.ds_next)
    h.set_corridor(g3["ub_free"], g3["lb_free"])
    h.set_path_geometry(g1["x"], g1["y"], g1["psi"], g1["border_ub"], g1["border_lb"])
    if with_plant:
        h.rollout_set_plant(plant.params(B), plant.seed)
    return h


def timed(h, s0, poses, est):
    h.rollout_init(0.05, cum, s0, poses)
    if est is not None:      # (behind rollout_init, like the delay)
        h.rollout_set_estimator(est.params(s0.size), est.seed, est.car0, est.step0)
    h.rollout_step(warmup)
    h.sync()
    t = time.perf_counter()
    h.rollout_step(steps)
    h.sync()
    return (time.perf_counter() - t) / steps * 1e3


for B in args.B:
    starts = np.random.default_rng(7).integers(0, 200, B)
    s0, poses = cum[starts], np.stack([g1["x"][starts], g1["y"][starts], g1["psi"][starts]], axis=1)
    variants = {}
    if parent_lib is not None:
        variants["parent"] = (handle(parent_lib, B, False), None)
    variants["estimator off"] = (handle(this_lib, B, False), None)
    variants["exact"] = (handle(this_lib, B, False), matched)              # K3e launched, nothing to estimate: the trajectories of off
    variants["noisy plant"] = (handle(this_lib, B, True), None)
    variants["noisy + K3e"] = (handle(this_lib, B, True), matched)
    ms = {k: [] for k in variants}
    for _ in range(args.repeats):
        for k, (h, e) in variants.items():
            ms[k].append(timed(h, s0, poses, e))
    for k, v in ms.items():
        v = np.sort(v)
        print("B=%5d %-13s  median %.4f ms/step   min %.4f  max %.4f   (%d repeats of %d steps)" % (B, k, np.median(v), v[0], v[-1], v.size, steps))
    state = {k: h.rollout_state() for k, (h, _) in variants.items()}
    if "parent" in variants:      # estimator off computes what the parent computed
        a, b = state["parent"], state["estimator off"]
        print("B=%5d estimator off against the parent: all of the state bit-equal: %s" % (B, all(np.array_equal(a[k], b[k]) for k in a)))
    a, b = state["estimator off"], state["exact"]
    print("B=%5d exact against estimator off: all of the state bit-equal: %s" % (B, all(np.array_equal(a[k], b[k]) for k in a)))
    es = variants["noisy + K3e"][0].rollout_estimator()
    on = es["steps"] > 0
    print("B=%5d noisy + K3e: sqrt(err2_sum / meas2_sum) median %.3f, max %.3f" %
          (B, np.median(np.sqrt(es["err2_sum"][on] / es["meas2_sum"][on])), np.max(np.sqrt(es["err2_sum"][on] / es["meas2_sum"][on]))))
    for name, q in state.items():
        print("B=%5d %-13s  alive == 1: %d of %d; statuses of the last step: %s; infeasibility counters > 0: %d" %
              (B, name, int((q["alive"] == 1).sum()), B, dict(zip(*(v.tolist() for v in np.unique(q["status"], return_counts=True)))),
               int((q["counter"] > 0).sum())))
    for h, _ in variants.values():
        h.close()
