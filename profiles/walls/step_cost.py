"""Cost of one rollout step with per-car worlds: 8 walls per car, 8 discs per car, or the shared table.

    python profiles/walls/step_cost.py --world walls|discs|none [--pkg DIR] [--B 1024] [--steps 40] [--repeats 7]

--pkg: the package directory to import mpmpc from (default: this tree's) - a build of another commit measures that commit
with the same script (it has no walls: --world discs / none only).  Prints one JSON line: the median, the smallest and the
largest time of a step in microseconds over `repeats` windows of `steps` steps, each window a fresh rollout_init, timed by
the host clock around rollout_step(steps) + rollout_state() (which synchronises)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--world", required=True, choices=["walls", "discs", "none"])
ap.add_argument("--pkg", default=os.path.join(ROOT, "multi-purpose-mpc_amd"))
ap.add_argument("--B", type=int, default=1024)
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--repeats", type=int, default=7)
a = ap.parse_args()
sys.path[:0] = [a.pkg, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), ROOT]
import mpmpc                      # noqa: E402
import mpmpc_testlib as T         # noqa: E402
import scenarios                  # noqa: E402
from map import Map, Obstacle     # noqa: E402

N, B = 30, a.B
g1 = np.load(os.path.join(ROOT, "tests", "golden", "g1_path_sim_track.npz"))
hh, ww = g1["grid_shape"]
grid = np.ascontiguousarray(np.unpackbits(g1["grid_free"])[:hh * ww].reshape(hh, ww).astype(np.int8))
origin, res = tuple(float(v) for v in g1["origin"]), float(g1["resolution"][0])
sm = float(np.load(os.path.join(ROOT, "tests", "golden", "g3o_sim_obstacles.npz"))["safety_margin"][0])
tr = scenarios.sim_track()
m = Map.from_grid(grid, origin, res)
n = g1["x"].size
idx = list(range(15, n, n // 7)) + [15 + n // 14]                          # 8 gates: 45 % of the way across, sides alternating
bounds = []
for k, i in enumerate(idx):
    p, q = (g1["border_ub"][i], g1["border_lb"][i]) if k % 2 == 0 else (g1["border_lb"][i], g1["border_ub"][i])
    bounds.append((tuple(p), tuple(p + 0.45 * (q - p))))
discs = m.obstacle_discs([Obstacle(c[0], c[1], c[2]) for c in g1["obstacles"][:8]])
h = mpmpc.Handle(T.stock_config(N, max_batch=B), mpmpc.default_settings())
h.set_path(tr.kappa, tr.v_ref, tr.ds_next)
h.set_map(grid, origin, res)
h.set_path_geometry(g1["x"], g1["y"], g1["psi"], g1["border_ub"], g1["border_lb"])
h.build_corridor(N, 2 * sm, sm, want_tables=False)
rng = np.random.default_rng(9)
starts = rng.integers(0, n, B)
cum = np.cumsum(g1["segment_lengths"])
poses = np.stack([g1["x"][starts], g1["y"][starts], g1["psi"][starts]], 1)
if a.world == "walls":
    h.rollout_set_walls([m.boundary_walls(bounds)] * B)
elif a.world == "discs":
    h.rollout_set_obstacles([discs] * B)
times = []
for r in range(a.repeats + 1):                                             # (the first window warms up)
    h.rollout_init(0.05, cum, cum[starts], poses)
    h.rollout_step(2)
    h.rollout_state()
    t0 = time.perf_counter()
    h.rollout_step(a.steps)
    st = h.rollout_state()
    times.append((time.perf_counter() - t0) / a.steps * 1e6)
times = times[1:]
print(json.dumps(dict(world=a.world, pkg=os.path.relpath(a.pkg, ROOT), B=B, N=N, steps=a.steps, repeats=a.repeats,
                      us_per_step_median=round(float(np.median(times)), 1), us_min=round(min(times), 1), us_max=round(max(times), 1),
                      alive=int((st["alive"] == 1).sum()), version=h.lib.mpmpc_version().decode())))
h.close()
