"""Per-step time of the device rollout with the lidar localiser (K0l + K3l) and the time of K0d, the method of
profiles/estimator/estimator_timing.py: N = 30, Sim_Track's free corridor and its map, the default warm start, 5 warm-up steps,
then 60 timed steps between two synchronisations; every variant is repeated, the variants alternating, and the median and the
spread over the repeats are printed.  90 beams over 270 degrees, range 1 m, D = 6, m = 1.  Variants:
    localiser off     no setting: what the parent launches
    dead reckoning    period 10^6: K3l alone, prior and statistics (no K0l, no match)
    one candidate     W = T = 0: K0l and K3l with a single candidate
    W=3 T=2           K0l and K3l with 245 candidates

    python profiles/localiser/localiser_timing.py [--parent OTHER/libmpmpc.so] [--repeats 5] [--B 1024 8192]

--parent: a build of another commit's library, loaded into the same process and timed as a further variant.  (GPU box)"""
import argparse
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for d in ("multi-purpose-mpc_amd", "tests", "oracle"):
    sys.path.insert(0, os.path.join(ROOT, d))
import mpc_np as M                  # noqa: E402
import mpmpc                        # noqa: E402
import mpmpc_testlib as T           # noqa: E402
import scenarios                    # noqa: E402
from localiser import Localiser     # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--parent", default=None)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--B", type=int, nargs="+", default=[1024, 8192])
args = ap.parse_args()

g1 = np.load(M.GOLDEN + "/g1_path_sim_track.npz")
g3 = np.load(M.GOLDEN + "/g3_corridor.npz")
_, grid, origin, res = T.g1_world("sim")
grid = np.ascontiguousarray(grid, np.int8)
N, warmup, steps = 30, 5, 60
tr = scenarios.sim_track()
cum = np.cumsum(g1["segment_lengths"])
this_lib = mpmpc.load_library()
ang = np.linspace(-2.356194490192345, 2.356194490192345, 90)
lidar = types.SimpleNamespace(measurements=np.stack([ang, np.ones(90)]), range=1.0)
SETTINGS = {"dead reckoning": Localiser(lidar, 6, 1, 3, 2, 0.01, min_hits=5, period=10 ** 6, step0=1),
            "one candidate": Localiser(lidar, 6, 1, 0, 0, 0.0, min_hits=5),
            "W=3 T=2": Localiser(lidar, 6, 1, 3, 2, 0.01, min_hits=5)}


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
    h.set_map(grid, origin, res)
    h.set_path_geometry(g1["x"], g1["y"], g1["psi"], g1["border_ub"], g1["border_lb"])
    return h


def timed(h, s0, poses, loc):
    h.rollout_init(0.05, cum, s0, poses)
    if loc is not None:      # (behind rollout_init, like the estimator)
        h.rollout_set_localiser(s0.size, **loc.setting())
    h.rollout_step(warmup)
    h.sync()
    t = time.perf_counter()
    h.rollout_step(steps)
    h.sync()
    return (time.perf_counter() - t) / steps * 1e3


# K0d once on the map, through mpmpc_distance_field (the upload of the grid and the download of the field included)
mpmpc.distance_field(grid, 6)
t_field = []
for _ in range(9):
    t = time.perf_counter()
    mpmpc.distance_field(grid, 6)
    t_field.append((time.perf_counter() - t) * 1e3)
print("K0d on the %d x %d map, D = 6, with both copies: median %.3f ms, min %.3f, max %.3f (9 calls)" %
      (grid.shape[0], grid.shape[1], np.median(t_field), min(t_field), max(t_field)))
t_field = []
for _ in range(9):
    t = time.perf_counter()
    mpmpc.distance_field(grid, 15)
    t_field.append((time.perf_counter() - t) * 1e3)
print("K0d on the %d x %d map, D = 15, with both copies: median %.3f ms, min %.3f, max %.3f (9 calls)" %
      (grid.shape[0], grid.shape[1], np.median(t_field), min(t_field), max(t_field)))

for B in args.B:
    starts = np.random.default_rng(7).integers(0, 200, B)
    s0, poses = cum[starts], np.stack([g1["x"][starts], g1["y"][starts], g1["psi"][starts]], axis=1)
    variants = {}
    if parent_lib is not None:
        variants["parent"] = (handle(parent_lib, B), None)
    variants["localiser off"] = (handle(this_lib, B), None)
    for name, loc in SETTINGS.items():
        variants[name] = (handle(this_lib, B), loc)
    ms = {k: [] for k in variants}
    for _ in range(args.repeats):
        for k, (h, loc) in variants.items():
            ms[k].append(timed(h, s0, poses, loc))
    for k, v in ms.items():
        v = np.sort(v)
        print("B=%5d %-15s  median %.4f ms/step   min %.4f  max %.4f   (%d repeats of %d steps)" % (B, k, np.median(v), v[0], v[-1], v.size, steps))
    state = {k: h.rollout_state() for k, (h, _) in variants.items()}
    if "parent" in variants:      # localiser off computes what the parent computed
        a, b = state["parent"], state["localiser off"]
        print("B=%5d localiser off against the parent: all of the state bit-equal: %s" % (B, all(np.array_equal(a[k], b[k]) for k in a)))
    for name in SETTINGS:
        lc = variants[name][0].rollout_localiser()
        print("B=%5d %-15s  matched %d, lost %d, edge %d; err2_sum %.4e, prior2_sum %.4e m^2; alive == 1: %d of %d" %
              (B, name, lc["matched"].sum(), lc["lost"].sum(), lc["edge"].sum(), lc["err2_sum"].sum(), lc["prior2_sum"].sum(),
               int((state[name]["alive"] == 1).sum()), B))
    for h, _ in variants.values():
        h.close()
