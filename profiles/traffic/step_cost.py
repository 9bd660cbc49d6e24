"""Per-step time of the device rollout with traffic (K0t) against the step-by-step host loop on the same world, and of the
static-disc rollout against the library of the commit before.

    python profiles/traffic/step_cost.py [--parent-lib PATH/libmpmpc.so] [--quick]

Sim_Track, N = 30, B = 1 024 / 8 192.  Cases, run in turn `rounds` times in one process (so that whatever else the machine
does hits all of them alike):
  parent_static   the parent commit's library (--parent-lib), 6 static discs per car, cars spread over the path
  static          this tree's library, the same 6 static discs (no traffic set: nothing new is launched)
  traffic         this tree's library, a traffic world: groups of 8 cars that follow each other 4 .. 10 waypoints apart,
                  radius 0.03 .. 0.05 m, S = 4 slots, range 0.5 m, no other discs; one call
  host_loop       the same world without K0t: every step reads rollout_state, evaluates the law in numpy
                  (traffic.traffic_discs), uploads every car's disc list and calls rollout_step(1)
One JSON line per case and round: ms per step = host clock over `steps` steps after `warmup`, the window closed by
rollout_state (a device synchronise); the cars still running at the end; and whether the final state equals the first
case's of the same world (static = parent_static, host_loop = traffic).  K0t's own time per launch comes from a kernel trace
of this script (README.md)."""
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
import traffic  # noqa: E402
from map import Map, Obstacle  # noqa: E402

NINE = [(0.0, 0.0, 0.05), (-0.8, -0.5, 0.08), (-0.7, -1.5, 0.05), (-0.3, -1.0, 0.08), (0.27, -1.0, 0.05),
        (0.78, -1.47, 0.05), (0.73, -0.9, 0.07), (1.2, 0.0, 0.08), (0.67, -0.05, 0.06)]
TS, N = 0.05, 30
GROUP, SLOTS, RANGE = 8, 4, 0.5
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
        static6 = [m.obstacle_discs([Obstacle(c[0] + rng.uniform(-0.05, 0.05), c[1] + rng.uniform(-0.05, 0.05),
                                              rng.uniform(0.04, 0.07)) for c in NINE[:6]]) for _ in range(B)]
        # the traffic world: car b belongs to group b // 8, the cars of a group follow each other
        gaps = rng.integers(4, 11, B)
        gaps[::GROUP] = 0
        t_starts = (np.repeat(rng.integers(0, n_wp, B // GROUP), GROUP) + np.cumsum(gaps) - np.repeat(np.cumsum(gaps)[::GROUP], GROUP)) % n_wp
        t_poses = np.stack([g1["x"][t_starts], g1["y"][t_starts], g1["psi"][t_starts]], 1)
        grp, rad, S, rc = traffic.Traffic(np.arange(B) // GROUP, rng.uniform(0.03, 0.05, B), SLOTS, RANGE).cells(m.resolution)
        h_new = handle(new, B, tr, g1, grid, sm)
        h_old = handle(older_library(parent), B, tr, g1, grid, sm) if parent else None

        def timed(h, s0, p0, per_step=None):
            h.rollout_init(TS, cum, cum[s0], p0)
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
            st = h_new.rollout_state()
            d = traffic.traffic_discs(st["pose"], st["alive"], grp, rad, S, rc, m.origin, m.resolution, m.width, m.height)
            h_new.rollout_set_obstacles(list(d))

        first = {}
        for r in range(rounds):
            for case in ("parent_static", "static", "traffic", "host_loop"):
                if case == "parent_static":
                    if not h_old:
                        continue
                    h_old.rollout_set_obstacles(static6)
                    dt, st = timed(h_old, starts, poses)
                elif case == "static":
                    h_new.rollout_set_traffic(None)
                    h_new.rollout_set_obstacles(static6)
                    dt, st = timed(h_new, starts, poses)
                elif case == "traffic":
                    h_new.rollout_set_obstacles(None)
                    h_new.rollout_set_traffic(grp, rad, S, rc)
                    dt, st = timed(h_new, t_starts, t_poses)
                else:
                    h_new.rollout_set_traffic(None)
                    dt, st = timed(h_new, t_starts, t_poses, host_step)
                world = "six" if case in ("parent_static", "static") else "traffic"
                ref = first.setdefault(world, st)
                print(json.dumps(dict(B=B, N=N, case=case, round=r, ms_per_step=round(dt * 1e3, 4),
                                      running=int((st["alive"] == 1).sum()), blocked=int((st["alive"] == -3).sum()),
                                      same_as_first=bool(all(np.array_equal(st[k], ref[k]) for k in KEYS)))), flush=True)
        h_new.close()
        if h_old:
            h_old.close()


if __name__ == "__main__":
    main()
