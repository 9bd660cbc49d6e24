"""Per-step time of the device rollout with an actuation delay (K3d / K3q): the setting off, d = c = 0 on every car (the two
launches alone) and d = c = 3, the method of profiles/plant/plant_timing.py: N = 30, Sim_Track's free corridor, the default warm
start, 5 warm-up steps, then 60 timed steps between two synchronisations; every variant is repeated, the variants alternating,
and the median and the spread over the repeats are printed.

    python profiles/delay/delay_timing.py [--parent OTHER/libmpmpc.so] [--repeats 7] [--B 1024 8192]
    python profiles/delay/delay_timing.py --trace --B 1024      # d = c = 3 only, for a kernel trace around it (rocprofv3)

--parent: a build of another commit's library, loaded into the same process and timed as a further variant (the parent has no
delay: it is "delay off" on the older code).  (GPU box)"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for d in ("multi-purpose-mpc_amd", "tests", "oracle"):
    sys.path.insert(0, os.path.join(ROOT, d))
import mpc_np as M          # noqa: E402
import mpmpc                # noqa: E402
import mpmpc_testlib as T   # noqa: E402
import scenarios            # noqa: E402
from delay import Delay     # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--parent", default=None)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--B", type=int, nargs="+", default=[1024, 8192])
ap.add_argument("--trace", action="store_true")
args = ap.parse_args()

g1 = np.load(M.GOLDEN + "/g1_path_sim_track.npz")
g3 = np.load(M.GOLDEN + "/g3_corridor.npz")
N, warmup, steps = 30, 5, 60
tr = scenarios.sim_track()
cum = np.cumsum(g1["segment_lengths"])
this_lib = mpmpc.load_library()


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


def handle(lib, B):
    mpmpc._lib = lib      # (Handle binds the library it is made with)
    try:
        h = mpmpc.Handle(T.stock_config(N, max_batch=B))
    finally:
        mpmpc._lib = this_lib
    h.set_path(tr.kappa, tr.v_ref, tr.ds_next)
    h.set_corridor(g3["ub_free"], g3["lb_free"])
    h.set_path_geometry(g1["x"], g1["y"], g1["psi"], g1["border_ub"], g1["border_lb"])
    return h


def timed(h, s0, poses, delay):
    h.rollout_init(0.05, cum, s0, poses)
    if delay is not None:      # (behind rollout_init, which zeroes the registers: the commands in flight)
        h.rollout_set_delay(*delay.arrays(s0.size))
    h.rollout_step(warmup)
    h.sync()
    t = time.perf_counter()
    h.rollout_step(steps)
    h.sync()
    return (time.perf_counter() - t) / steps * 1e3


for B in args.B:
    starts = np.random.default_rng(7).integers(0, 200, B)
    s0, poses = cum[starts], np.stack([g1["x"][starts], g1["y"][starts], g1["psi"][starts]], axis=1)
    flying = np.zeros((B, 8, 2))
    flying[:, :, 0] = 0.6
    variants = {}
    if not args.trace:
        if parent_lib is not None:
            variants["parent"] = (handle(parent_lib, B), None)
        variants["delay off"] = (handle(this_lib, B), None)
        variants["d = c = 0"] = (handle(this_lib, B), Delay(0, queue0=flying))      # K3d and K3q launched, the trajectories those of delay off
    variants["d = c = 3"] = (handle(this_lib, B), Delay(3, queue0=flying))
    ms = {k: [] for k in variants}
    for _ in range(1 if args.trace else args.repeats):
        for k, (h, dl) in variants.items():
            ms[k].append(timed(h, s0, poses, dl))
    for k, v in ms.items():
        v = np.sort(v)
        print("B=%5d %-9s  median %.4f ms/step   min %.4f  max %.4f   (%d repeats of %d steps)" % (B, k, np.median(v), v[0], v[-1], v.size, steps))
    state = {k: h.rollout_state() for k, (h, _) in variants.items()}
    if "parent" in variants:      # delay off computes what the parent computed
        a, b = state["parent"], state["delay off"]
        print("B=%5d delay off against the parent: all of the state bit-equal: %s" % (B, all(np.array_equal(a[k], b[k]) for k in a)))
    if "d = c = 0" in variants:
        a, b = state["delay off"], state["d = c = 0"]
        print("B=%5d d = c = 0 against delay off: all of the state bit-equal: %s" % (B, all(np.array_equal(a[k], b[k]) for k in a)))
    for name, q in state.items():
        print("B=%5d %-9s  alive == 1: %d of %d; statuses of the last step: %s; infeasibility counters > 0: %d" %
              (B, name, int((q["alive"] == 1).sum()), B, dict(zip(*(v.tolist() for v in np.unique(q["status"], return_counts=True)))),
               int((q["counter"] > 0).sum())))
    for h, _ in variants.values():
        h.close()
