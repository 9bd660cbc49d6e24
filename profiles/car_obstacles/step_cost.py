"""Per-step time of the device rollout with per-car obstacles (K0c) against the shared corridor table.

    python profiles/car_obstacles/step_cost.py [--quick]

Sim_Track, N = 30, cars spread over the path; 0 / 9 / 32 discs per car (jittered copies of the nine obstacles of
src/simulation.py:40-48, the rest random on the map), B = 16 / 1 024 / 8 192.  One JSON line per case: ms per step
(wall clock over `steps` steps, after `warmup`), and the cars still running at the end."""
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
from map import Map, Obstacle  # noqa: E402

NINE = [(0.0, 0.0, 0.05), (-0.8, -0.5, 0.08), (-0.7, -1.5, 0.05), (-0.3, -1.0, 0.08), (0.27, -1.0, 0.05),
        (0.78, -1.47, 0.05), (0.73, -0.9, 0.07), (1.2, 0.0, 0.08), (0.67, -0.05, 0.06)]


def discs_for(m, k, rng):
    obs = [Obstacle(c[0] + rng.uniform(-0.05, 0.05), c[1] + rng.uniform(-0.05, 0.05), rng.uniform(0.04, 0.07))
           for c in NINE[:k]]
    while len(obs) < k:
        obs.append(Obstacle(rng.uniform(-0.9, 1.4), rng.uniform(-1.9, 0.4), rng.uniform(0.02, 0.05)))
    return m.obstacle_discs(obs)


def main():
    quick = "--quick" in sys.argv
    g1 = np.load(os.path.join(ROOT, "tests", "golden", "g1_path_sim_track.npz"))
    h_, w_ = g1["grid_shape"]
    grid = np.ascontiguousarray(np.unpackbits(g1["grid_free"])[:h_ * w_].reshape(h_, w_).astype(np.int8))
    tr = scenarios.sim_track()
    sm = float(np.load(os.path.join(ROOT, "tests", "golden", "g3o_sim_obstacles.npz"))["safety_margin"][0])
    N = 30
    m = Map.from_grid(grid, (-1.0, -2.0), 0.005)
    cum = np.cumsum(g1["segment_lengths"])
    warmup, steps = (3, 10) if quick else (5, 40)
    for B in (16, 1024, 8192):
        h = mpmpc.Handle(T.stock_config(N, max_batch=B))
        h.set_path(tr.kappa, tr.v_ref, tr.ds_next)
        h.set_map(grid, (-1.0, -2.0), 0.005)
        h.set_path_geometry(g1["x"], g1["y"], g1["psi"], g1["border_ub"], g1["border_lb"])
        h.build_corridor(N, 2 * sm, sm, want_tables=False)
        rng = np.random.default_rng(B)
        starts = rng.integers(0, g1["x"].size, B)
        poses = np.stack([g1["x"][starts], g1["y"][starts], g1["psi"][starts]], 1)
        for mode, k in (("shared", 0), ("per_car", 0), ("per_car", 9), ("per_car", 32)):
            h.rollout_set_obstacles(None if mode == "shared" else [discs_for(m, k, rng) for _ in range(B)])
            h.rollout_init(0.05, cum, cum[starts], poses)
            h.rollout_step(warmup)
            h.rollout_state()
            t0 = time.perf_counter()
            h.rollout_step(steps)
            st = h.rollout_state()
            dt = (time.perf_counter() - t0) / steps
            print(json.dumps(dict(B=B, N=N, mode=mode, discs=k, ms_per_step=round(dt * 1e3, 4),
                                  running=int((st["alive"] == 1).sum()), blocked=int((st["alive"] == -3).sum()),
                                  overflow=int((st["alive"] == -4).sum()))), flush=True)
        h.close()


if __name__ == "__main__":
    main()
