"""What perception (K0s) costs: per rollout step with perception on against off, and the rollout that never perceives against
the library of the commit before.

    python profiles/perception/perception_cost.py [--parent-lib PATH/libmpmpc.so] [--quick] [--trace B]

K0l's recorded operating point (profiles/lidar): Sim_Track, N = 30, cars spread over the path, 6 static discs per car,
B = 1 024 / 8 192; the sensor: FoV 180 deg, 1 deg, range 0.3 m (181 beams, a window of 121 x 121 cells); hold = 2.  Cases, run
in turn `rounds` times in one process, one JSON line per case and round:
  parent_steps   the parent commit's library (--parent-lib): one rollout_step(steps) call
  steps          this tree's library, the same call, perception never set
  steps_per      this tree's library, the same call with perception on
ms per step = host clock, the window closed by a device synchronise.  --trace B: the workload for a kernel trace instead (a run
of its own, no counters): 20 perceiving steps of B cars, then 20 rollout_scan calls on the same state - K0s and K0l side by
side in one run."""
import ctypes as C
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
from lidar_model import LidarModel  # noqa: E402
from map import Map, Obstacle  # noqa: E402

NINE = [(0.0, 0.0, 0.05), (-0.8, -0.5, 0.08), (-0.7, -1.5, 0.05), (-0.3, -1.0, 0.08), (0.27, -1.0, 0.05),
        (0.78, -1.47, 0.05), (0.73, -0.9, 0.07), (1.2, 0.0, 0.08), (0.67, -0.05, 0.06)]
TS, N = 0.05, 30
KEYS = ("s", "pose", "cc", "wp_id", "status", "counter", "alive")


def older_library(path):
    """a libmpmpc.so from before this tree's newest entry points: the declarations of those it has"""
    new, old = mpmpc.load_library(), C.CDLL(path)
    for name in mpmpc.EXPORTS:
        if hasattr(old, name):
            getattr(old, name).argtypes = getattr(new, name).argtypes
            getattr(old, name).restype = getattr(new, name).restype
    return old


def handle(lib, B, tr, g1, grid, sm):
    keep, mpmpc._lib = mpmpc._lib, lib
    try:
        h = mpmpc.Handle(T.stock_config(N, max_batch=B))
    finally:
        mpmpc._lib = keep
    h.set_path(tr.kappa, tr.v_ref, tr.ds_next)
    h.set_map(grid, (-1.0, -2.0), 0.005)
    h.set_path_geometry(g1["x"], g1["y"], g1["psi"], g1["border_ub"], g1["border_lb"])
    h.build_corridor(N, 2 * sm, sm, want_tables=False)
    return h


def main():
    quick = "--quick" in sys.argv
    parent = sys.argv[sys.argv.index("--parent-lib") + 1] if "--parent-lib" in sys.argv else None
    trace = int(sys.argv[sys.argv.index("--trace") + 1]) if "--trace" in sys.argv else 0
    g1 = np.load(os.path.join(ROOT, "tests", "golden", "g1_path_sim_track.npz"))
    h_, w_ = g1["grid_shape"]
    grid = np.ascontiguousarray(np.unpackbits(g1["grid_free"])[:h_ * w_].reshape(h_, w_).astype(np.int8))
    tr = scenarios.sim_track()
    sm = float(np.load(os.path.join(ROOT, "tests", "golden", "g3o_sim_obstacles.npz"))["safety_margin"][0])
    m = Map.from_grid(grid, (-1.0, -2.0), 0.005)
    cum = np.cumsum(g1["segment_lengths"])
    n_wp = g1["x"].size
    warmup, steps, rounds = (3, 10, 2) if quick else (5, 40, 5)
    lidar = LidarModel(FoV=180, range=0.3, resolution=1)
    ang, rng_m, hold = lidar.measurements[0], lidar.range, 2
    new = mpmpc.load_library()
    print(json.dumps(dict(library=new.mpmpc_version().decode(),
                          parent=older_library(parent).mpmpc_version().decode() if parent else None)), flush=True)
    for B in ((trace,) if trace else (1024, 8192)):
        rng = np.random.default_rng(B)
        starts = rng.integers(0, n_wp, B)
        poses = np.stack([g1["x"][starts], g1["y"][starts], g1["psi"][starts]], 1)
        static6 = [m.obstacle_discs([Obstacle(c[0] + rng.uniform(-0.05, 0.05), c[1] + rng.uniform(-0.05, 0.05),
                                              rng.uniform(0.04, 0.07)) for c in NINE[:6]]) for _ in range(B)]
        h_new = handle(new, B, tr, g1, grid, sm)
        h_old = handle(older_library(parent), B, tr, g1, grid, sm) if parent and not trace else None
        for h in (h_new, h_old):
            if h:
                h.rollout_set_obstacles(static6)
        if trace:
            h_new.rollout_set_perception(ang, rng_m, hold)
            h_new.rollout_init(TS, cum, cum[starts], poses)
            h_new.rollout_step(20)
            for _ in range(20):
                h_new.rollout_scan(ang, rng_m)
            per = h_new.rollout_perception()
            print(json.dumps(dict(B=B, case="trace", slots_seen=int(np.sum(per["disc_first"] >= 0)), slots=6 * B)), flush=True)
            h_new.close()
            continue

        def timed(h):
            h.rollout_init(TS, cum, cum[starts], poses)
            h.rollout_step(warmup)
            h.rollout_state()
            t0 = time.perf_counter()
            h.rollout_step(steps)
            st = h.rollout_state()
            return (time.perf_counter() - t0) / steps, st

        first = None
        for r in range(rounds):
            for case in ("parent_steps", "steps", "steps_per"):
                if case == "parent_steps":
                    if not h_old:
                        continue
                    dt, st = timed(h_old)
                elif case == "steps":
                    h_new.rollout_set_perception(None)
                    dt, st = timed(h_new)
                else:
                    h_new.rollout_set_perception(ang, rng_m, hold)
                    dt, st = timed(h_new)
                    h_new.rollout_set_perception(None)
                if case != "steps_per":
                    first = first or st
                print(json.dumps(dict(B=B, N=N, case=case, round=r, ms=round(dt * 1e3, 4), running=int((st["alive"] == 1).sum()),
                                      same_as_first=bool(all(np.array_equal(st[k], first[k]) for k in KEYS)))), flush=True)
        h_new.close()
        if h_old:
            h_old.close()


if __name__ == "__main__":
    main()
