"""Per-step time of the device rollout with the dynamic plant (K3y in place of K3p): an identity plant alone, and the dynamic
car behind it at n = 8 and n = 32 sub-steps, the method of profiles/plant/plant_timing.py: N = 30, Sim_Track's free corridor,
the default warm start, 5 warm-up steps, then 60 timed steps between two synchronisations; every variant is repeated, the
variants alternating, and the median and the spread over the repeats are printed.

    python profiles/dynamics/dynamics_timing.py [--parent OTHER/libmpmpc.so] [--repeats 7] [--B 1024 8192]
    python profiles/dynamics/dynamics_timing.py --trace 8 --B 1024      # n = 8 only (0: the plant alone), for a kernel trace around it (rocprofv3)

--parent: a build of another commit's library, loaded into the same process and timed as a further variant (the parent has no
dynamics: it is "plant alone" on the older code).  (GPU box)"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for d in ("multi-purpose-mpc_amd", "tests", "oracle"):
    sys.path.insert(0, os.path.join(ROOT, d))
import mpc_np as M              # noqa: E402
import mpmpc                    # noqa: E402
import mpmpc_testlib as T       # noqa: E402
import scenarios                # noqa: E402
from dynamics import Dynamics   # noqa: E402
from plant import Plant         # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--parent", default=None)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--B", type=int, nargs="+", default=[1024, 8192])
ap.add_argument("--trace", type=int, default=None, help="one variant, one repeat: the number of sub-steps (0: the plant alone)")
args = ap.parse_args()

g1 = np.load(M.GOLDEN + "/g1_path_sim_track.npz")
g3 = np.load(M.GOLDEN + "/g3_corridor.npz")
N, warmup, steps = 30, 5, 60
tr = scenarios.sim_track()
cum = np.cumsum(g1["segment_lengths"])
this_lib = mpmpc.load_library()
# a car that is stable at 8 sub-steps from 0.4 m/s on (lambda * Ts / n = 0.94), so that nearly every step is a dynamic one
CAR = dict(mass=1.0, inertia=0.004, lf=0.06, Cf=30.0, Cr=30.0, mu=1.0, v_dyn=0.4)


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


def handle(lib, B, dyn):
    mpmpc._lib = lib      # (Handle binds the library it is made with)
    try:
        h = mpmpc.Handle(T.stock_config(N, max_batch=B))
    finally:
        mpmpc._lib = this_lib
    h.set_path(tr.kappa, tr.v_ref, tr.ds_next)
    h.set_corridor(g3["ub_free"], g3["lb_free"])
    h.set_path_geometry(g1["x"], g1["y"], g1["psi"], g1["border_ub"], g1["border_lb"])
    h.rollout_set_plant(Plant().params(B))
    if dyn is not None:
        h.rollout_set_dynamics(dyn.params(B))
    return h


def timed(h, s0, poses):
    h.rollout_init(0.05, cum, s0, poses)
    h.rollout_step(warmup)
    h.sync()
    t = time.perf_counter()
    h.rollout_step(steps)
    h.sync()
    return (time.perf_counter() - t) / steps * 1e3


for B in args.B:
    starts = np.random.default_rng(7).integers(0, 200, B)
    s0, poses = cum[starts], np.stack([g1["x"][starts], g1["y"][starts], g1["psi"][starts]], axis=1)
    if args.trace is not None:
        h = handle(this_lib, B, Dynamics(substeps=args.trace, **CAR) if args.trace > 0 else None)
        print("B=%5d %s  %.4f ms/step (one repeat of %d steps)" % (B, "n = %d" % args.trace if args.trace else "plant alone", timed(h, s0, poses), steps))
        h.close()
        continue
    variants = {}
    if parent_lib is not None:
        variants["parent"] = handle(parent_lib, B, None)
    variants["plant alone"] = handle(this_lib, B, None)
    variants["n = 8"] = handle(this_lib, B, Dynamics(substeps=8, **CAR))
    variants["n = 32"] = handle(this_lib, B, Dynamics(substeps=32, **CAR))
    ms = {k: [] for k in variants}
    for _ in range(args.repeats):
        for k, h in variants.items():
            ms[k].append(timed(h, s0, poses))
    base = float(np.median(ms["plant alone"]))
    for k, v in ms.items():
        v = np.sort(v)
        print("B=%5d %-11s  median %.4f ms/step   min %.4f  max %.4f   over the plant alone %+.1f us   (%d repeats of %d steps)" %
              (B, k, np.median(v), v[0], v[-1], (np.median(v) - base) * 1e3, v.size, steps))
    state = {k: h.rollout_state() for k, h in variants.items()}
    if "parent" in variants:      # the plant alone computes what the parent computed
        a, b = state["parent"], state["plant alone"]
        print("B=%5d plant alone against the parent: all of the state bit-equal: %s" % (B, all(np.array_equal(a[k], b[k]) for k in a)))
    for name in ("n = 8", "n = 32"):
        dy, q = variants[name].rollout_dynamics(), state[name]
        print("B=%5d %-11s  alive == 1: %d of %d; dynamic steps: %.1f %% of the driven ones; cars that clipped the front / rear: %d / %d; "
              "statuses of the last step: %s" % (B, name, int((q["alive"] == 1).sum()), B,
                                                 100.0 * dy["dyn_steps"].sum() / max(1, variants[name].rollout_plant()["steps"].sum()),
                                                 int((dy["sat_front"] > 0).sum()), int((dy["sat_rear"] > 0).sum()),
                                                 dict(zip(*(v.tolist() for v in np.unique(q["status"], return_counts=True))))))
    for h in variants.values():
        h.close()
