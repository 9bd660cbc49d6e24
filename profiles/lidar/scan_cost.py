"""What a lidar scan (K0l) costs: per fleet scan, per rollout step with and without a scan, against the numpy route a user
had before, and the rollout that never scans against the library of the commit before.

    python profiles/lidar/scan_cost.py [--parent-lib PATH/libmpmpc.so] [--quick]

Sim_Track, N = 30, cars spread over the path, 6 static discs per car, B = 1 024 / 8 192; the sensor: FoV 180 deg, 1 deg,
range 0.3 m (181 beams, a window of 121 x 121 cells).  Cases, run in turn `rounds` times in one process (so that whatever
else the machine does hits all of them alike), one JSON line per case and round:
  parent_steps   the parent commit's library (--parent-lib): one rollout_step(steps) call, no scans
  steps          this tree's library, the same call
  step_sync      this tree's library, rollout_step(1) + a device synchronise (rollout_state of nothing), `steps` times
  step_scan      this tree's library, rollout_step(1) + rollout_scan, `steps` times
  scan           rollout_scan alone, `steps` times on the last state (kernel + the copy of B x 181 doubles to the host)
  numpy          the numpy restatement of the law (tests/test_lidar.py) on `numpy_cars` of the same cars: s per scan
ms per step / per call = host clock, the window closed by a device synchronise.  K0l's own time per launch, its registers,
LDS and scratch come from a kernel trace of this script (a run of its own, no counters) and from
profiles/kernel_resources.py (README.md)."""
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
    g1 = np.load(os.path.join(ROOT, "tests", "golden", "g1_path_sim_track.npz"))
    h_, w_ = g1["grid_shape"]
    grid = np.ascontiguousarray(np.unpackbits(g1["grid_free"])[:h_ * w_].reshape(h_, w_).astype(np.int8))
    tr = scenarios.sim_track()
    sm = float(np.load(os.path.join(ROOT, "tests", "golden", "g3o_sim_obstacles.npz"))["safety_margin"][0])
    m = Map.from_grid(grid, (-1.0, -2.0), 0.005)
    cum = np.cumsum(g1["segment_lengths"])
    n_wp = g1["x"].size
    warmup, steps, rounds, numpy_cars = (3, 10, 2, 4) if quick else (5, 40, 5, 16)
    lidar = LidarModel(FoV=180, range=0.3, resolution=1)
    ang, rng_m = lidar.measurements[0], lidar.range
    new = mpmpc.load_library()
    print(json.dumps(dict(library=new.mpmpc_version().decode(),
                          parent=older_library(parent).mpmpc_version().decode() if parent else None)), flush=True)
    for B in (1024, 8192):
        rng = np.random.default_rng(B)
        starts = rng.integers(0, n_wp, B)
        poses = np.stack([g1["x"][starts], g1["y"][starts], g1["psi"][starts]], 1)
        static6 = [m.obstacle_discs([Obstacle(c[0] + rng.uniform(-0.05, 0.05), c[1] + rng.uniform(-0.05, 0.05),
                                              rng.uniform(0.04, 0.07)) for c in NINE[:6]]) for _ in range(B)]
        h_new = handle(new, B, tr, g1, grid, sm)
        h_old = handle(older_library(parent), B, tr, g1, grid, sm) if parent else None
        for h in (h_new, h_old):
            if h:
                h.rollout_set_obstacles(static6)

        def timed(h, each=None):
            """-> s per step of `steps` steps after `warmup`: one call, or one step at a time followed by each()"""
            h.rollout_init(TS, cum, cum[starts], poses)
            h.rollout_step(warmup)
            if each:
                each()
            h.rollout_state()
            t0 = time.perf_counter()
            if each is None:
                h.rollout_step(steps)
            else:
                for _ in range(steps):
                    h.rollout_step(1)
                    each()
            st = h.rollout_state()
            return (time.perf_counter() - t0) / steps, st

        first = None
        for r in range(rounds):
            for case in ("parent_steps", "steps", "step_sync", "step_scan", "scan", "numpy"):
                extra = {}
                if case == "parent_steps":
                    if not h_old:
                        continue
                    dt, st = timed(h_old)
                elif case == "steps":
                    dt, st = timed(h_new)
                elif case == "step_sync":
                    dt, st = timed(h_new, h_new.sync)
                elif case == "step_scan":
                    dt, st = timed(h_new, lambda: h_new.rollout_scan(ang, rng_m))
                elif case == "scan":
                    h_new.rollout_scan(ang, rng_m)
                    t0 = time.perf_counter()
                    for _ in range(steps):
                        got = h_new.rollout_scan(ang, rng_m)
                    dt = (time.perf_counter() - t0) / steps
                    st = h_new.rollout_state()
                    # and the handle-free entry point on the same cars: + the uploads of the grid, the poses, the discs
                    discs = h_new.rollout_obstacles()
                    t0 = time.perf_counter()
                    same = mpmpc.lidar_scan(grid, m.origin, m.resolution, st["pose"], ang, rng_m, discs)
                    extra = dict(ms_lidar_scan=round((time.perf_counter() - t0) * 1e3, 4), lidar_scan_equal=bool(np.array_equal(got, same)),
                                 beams_hit=round(float(np.mean(got < rng_m)), 4))
                else:
                    if r > 0:
                        continue
                    from test_lidar import _law
                    st = h_new.rollout_state()
                    discs = h_new.rollout_obstacles()
                    t0 = time.perf_counter()
                    want, _, _ = _law(grid, m.origin, m.resolution, st["pose"][:numpy_cars], ang, rng_m, discs[:numpy_cars])
                    dt = (time.perf_counter() - t0) / numpy_cars
                    got = h_new.rollout_scan(ang, rng_m)[:numpy_cars]
                    extra = dict(cars=numpy_cars, beams_differing_from_device=int(np.sum(got != want)))
                first = first or st
                print(json.dumps(dict(B=B, N=N, case=case, round=r, ms=round(dt * 1e3, 4), running=int((st["alive"] == 1).sum()),
                                      same_as_first=bool(all(np.array_equal(st[k], first[k]) for k in KEYS)), **extra)), flush=True)
        h_new.close()
        if h_old:
            h_old.close()


if __name__ == "__main__":
    main()
