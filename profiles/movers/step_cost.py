"""Per-step time of the device rollout with movers (K0m) against static per-car discs, and against the library of the
commit before.

    python profiles/movers/step_cost.py [--parent-lib PATH/libmpmpc.so] [--quick]

Sim_Track, N = 30, cars spread over the path, B = 1 024 / 8 192.  Cases, run in turn `rounds` times in one process (so that
whatever else the machine does hits all of them alike):
  parent_static   the parent commit's library (--parent-lib), 6 static discs per car
  static          this tree's library, the same 6 static discs
  movers          this tree's library, the first 3 of those discs + 3 movers per car (two along the path ahead of the car
                  at a third to two thirds of v_ref, one crossing the track)
  host_loop       the same world without K0m: every step evaluates the movers in numpy, uploads every car's disc list
                  and calls rollout_step(1)
One JSON line per case and round: ms per step = host clock over `steps` steps after `warmup`, the window closed by
rollout_state (a device synchronise); the cars still running at the end; and whether the final state equals the first
case's of the same world (static = parent_static, host_loop = movers).  K0m's own time per launch comes from a kernel trace
of this script (README.md)."""
import ctypes as C
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in ("multi-purpose-mpc_amd", "tests", "oracle", ""):
    sys.path.insert(0, os.path.join(ROOT, p))

import numpy as np  # noqa: E402

import movers  # noqa: E402
import mpmpc  # noqa: E402
import mpmpc_testlib as T  # noqa: E402
import scenarios  # noqa: E402
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
    g1 = np.load(os.path.join(ROOT, "tests", "golden", "g1_path_sim_track.npz"))
    h_, w_ = g1["grid_shape"]
    grid = np.ascontiguousarray(np.unpackbits(g1["grid_free"])[:h_ * w_].reshape(h_, w_).astype(np.int8))
    tr = scenarios.sim_track()
    sm = float(np.load(os.path.join(ROOT, "tests", "golden", "g3o_sim_obstacles.npz"))["safety_margin"][0])
    m = Map.from_grid(grid, (-1.0, -2.0), 0.005)
    cum = np.cumsum(g1["segment_lengths"])
    n_wp = g1["x"].size
    warmup, steps, rounds = (3, 10, 2) if quick else (5, 40, 5)
    new = mpmpc.load_library()
    print(json.dumps(dict(library=new.mpmpc_version().decode(),
                          parent=older_library(parent).mpmpc_version().decode() if parent else None)), flush=True)
    for B in (1024, 8192):
        rng = np.random.default_rng(B)
        starts = rng.integers(0, n_wp, B)
        poses = np.stack([g1["x"][starts], g1["y"][starts], g1["psi"][starts]], 1)
        static6, rows = [], []
        for b in range(B):
            static6.append(m.obstacle_discs([Obstacle(c[0] + rng.uniform(-0.05, 0.05), c[1] + rng.uniform(-0.05, 0.05),
                                                      rng.uniform(0.04, 0.07)) for c in NINE[:6]]))
            w0 = int(starts[b])
            mv = [movers.Mover.along_path(cum[(w0 + int(rng.integers(5, 26))) % n_wp], rng.uniform(-0.08, 0.08),
                                          rng.uniform(1 / 3, 2 / 3) * tr.v_ref[w0], rng.uniform(0.03, 0.05)) for _ in range(2)]
            wc = (w0 + int(rng.integers(10, 30))) % n_wp
            nx, ny = -math.sin(g1["psi"][wc]), math.cos(g1["psi"][wc])
            mv.append(movers.Mover.line(g1["x"][wc] - 0.3 * nx, g1["y"][wc] - 0.3 * ny, 0.6 * nx / (steps * TS),
                                        0.6 * ny / (steps * TS), rng.uniform(0.03, 0.05)))
            rows.append(np.array([q.row(TS, m.resolution) for q in mv]))
        static3 = [d[:3] for d in static6]
        flat = np.concatenate(rows)
        path = dict(cum=cum, x=g1["x"], y=g1["y"], psi=g1["psi"], circular=True)
        h_new = handle(new, B, tr, g1, grid, sm)
        h_old = handle(older_library(parent), B, tr, g1, grid, sm) if parent else None

        def timed(h, per_step=None):
            h.rollout_init(TS, cum, cum[starts], poses)
            t0 = None
            if per_step is None:
                h.rollout_step(warmup)
                h.rollout_state()
                t0 = time.perf_counter()
                h.rollout_step(steps)
            else:
                for k in range(warmup + steps):
                    if k == warmup:
                        h.rollout_state()
                        t0 = time.perf_counter()
                    per_step(k)
                    h.rollout_step(1)
            st = h.rollout_state()
            return (time.perf_counter() - t0) / steps, st

        def host_step(k):
            d = movers.mover_discs_rows(flat, float(k), m.origin, m.resolution, m.width, m.height, **path).reshape(B, 3, 3)
            h_new.rollout_set_obstacles([np.concatenate([static3[b], d[b]]) for b in range(B)])

        first = {}
        for r in range(rounds):
            for case in ("parent_static", "static", "movers", "host_loop"):
                if case == "parent_static":
                    if not h_old:
                        continue
                    h_old.rollout_set_obstacles(static6)
                    dt, st = timed(h_old)
                elif case == "static":
                    h_new.rollout_set_movers(None)
                    h_new.rollout_set_obstacles(static6)
                    dt, st = timed(h_new)
                elif case == "movers":
                    h_new.rollout_set_obstacles(static3)
                    h_new.rollout_set_movers(rows)
                    dt, st = timed(h_new)
                else:
                    h_new.rollout_set_movers(None)
                    dt, st = timed(h_new, host_step)
                world = "six" if case in ("parent_static", "static") else "moving"
                ref = first.setdefault(world, st)
                print(json.dumps(dict(B=B, N=N, case=case, round=r, ms_per_step=round(dt * 1e3, 4),
                                      running=int((st["alive"] == 1).sum()), blocked=int((st["alive"] == -3).sum()),
                                      same_as_first=bool(all(np.array_equal(st[k], ref[k]) for k in KEYS)))), flush=True)
        h_new.close()
        if h_old:
            h_old.close()


if __name__ == "__main__":
    main()
