"""What corridor commitment (K0k) costs per step and what it changes, on the worlds of profiles/movers/step_cost.py: Sim_Track,
N = 30, cars spread over the path, every car with 6 static discs ("six") or with the first 3 of them and 3 movers ("moving": two
along the path ahead of the car, one crossing the track).

    python profiles/commitment/commitment_timing.py [--parent-lib PATH/libmpmpc.so] [--quick]

Timing, B = 1 024 / 8 192, cases run in turn `rounds` times in one process (whatever else the machine does hits all alike);
ms per step = host clock over `steps` steps after `warmup`, the window closed by rollout_state (a device synchronise):
  parent      the parent commit's library (--parent-lib), the six-disc world
  off         this tree's library, the same world, the setting off (keep == NULL)
  keep_zero   ... keep = 0 for every car: the KEEP instantiation of K0c with every car off (memory and counters are kept)
  committed   ... keep = inf for every car
What it changes, B = 1 024 in both worlds, one fleet as its own A/B: cars b and b + B / 2 share start, pose and world, the first
half off (keep = 0) and the second at keep = inf; `steps_ab` steps one at a time with the audit on.  Per half: moved, the steps of
running cars whose solve was infeasible (-3) or inaccurate (2), audited steps with contact, cars with a contact, and how the
cars ended.  One JSON line per measurement."""
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
CAR_LENGTH, CAR_WIDTH = 0.12, 0.06


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


def worlds(B, rng, m, g1, tr, cum, steps):
    """profiles/movers/step_cost.py's: per car a start, 6 static discs and 3 movers"""
    n_wp = g1["x"].size
    starts = rng.integers(0, n_wp, B)
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
    return starts, static6, rows


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
    warmup, steps, rounds, steps_ab = (3, 10, 2, 20) if quick else (5, 40, 5, 120)
    new = mpmpc.load_library()
    old = older_library(parent) if parent else None
    print(json.dumps(dict(library=new.mpmpc_version().decode(), parent=old.mpmpc_version().decode() if old else None)), flush=True)

    # ---- what a step costs
    for B in (1024, 8192):
        starts, static6, _ = worlds(B, np.random.default_rng(B), m, g1, tr, cum, steps)
        poses = np.stack([g1["x"][starts], g1["y"][starts], g1["psi"][starts]], 1)
        h_new = handle(new, B, tr, g1, grid, sm)
        h_old = handle(old, B, tr, g1, grid, sm) if old else None
        for h in (h_new, h_old):
            if h:
                h.rollout_set_obstacles(static6)

        def timed(h, keep):
            h.rollout_init(TS, cum, cum[starts], poses)
            if h is h_new:
                h.rollout_set_commitment(keep)
            h.rollout_step(warmup)
            h.rollout_state()
            t0 = time.perf_counter()
            h.rollout_step(steps)
            st = h.rollout_state()
            return (time.perf_counter() - t0) / steps, st

        first = None
        for r in range(rounds):
            for case in ("parent", "off", "keep_zero", "committed"):
                if case == "parent" and not h_old:
                    continue
                dt, st = timed(h_old if case == "parent" else h_new,
                               None if case in ("parent", "off") else np.full(B, 0.0 if case == "keep_zero" else math.inf))
                first = first or st
                line = dict(B=B, N=N, case=case, round=r, ms_per_step=round(dt * 1e3, 4), running=int((st["alive"] == 1).sum()),
                            same_as_first=bool(all(np.array_equal(st[k], first[k]) for k in KEYS)))
                if case in ("keep_zero", "committed"):
                    c = h_new.rollout_commitment()
                    line.update(kept=int(c["kept"].sum()), moved=int(c["moved"].sum()))
                print(json.dumps(line), flush=True)
        h_new.close()
        if h_old:
            h_old.close()

    # ---- what it changes: one fleet, its first half off, its second half committed, in pairwise equal worlds
    B = 1024
    half = B // 2
    starts, static6, rows = worlds(half, np.random.default_rng(7), m, g1, tr, cum, steps_ab)
    starts = np.concatenate([starts, starts])
    poses = np.stack([g1["x"][starts], g1["y"][starts], g1["psi"][starts]], 1)
    keep = np.concatenate([np.zeros(half), np.full(half, math.inf)])
    h = handle(new, B, tr, g1, grid, sm)
    h.rollout_set_audit(1, CAR_LENGTH, CAR_WIDTH, 0.1)
    for world in ("six", "moving"):
        h.rollout_set_movers(None)
        if world == "six":
            h.rollout_set_obstacles(static6 + static6)
        else:
            h.rollout_set_obstacles([d[:3] for d in static6] * 2)
            h.rollout_set_movers(rows + rows)
        h.rollout_init(TS, cum, cum[starts], poses)
        h.rollout_set_commitment(keep)
        bad = np.zeros(B, np.int64)
        driven = np.zeros(B, np.int64)
        alive = np.ones(B, np.int32)
        for _ in range(steps_ab):
            h.rollout_step(1)
            st = h.rollout_state()
            run = alive == 1                       # the cars the step found running
            bad += run & ((st["status"] == -3) | (st["status"] == 2))
            driven += run
            alive = st["alive"]
        c, a = h.rollout_commitment(), h.rollout_audit()
        for name, sel in (("off", slice(0, half)), ("keep_inf", slice(half, B))):
            ends = dict(zip(*(v.tolist() for v in np.unique(alive[sel], return_counts=True))))
            print(json.dumps(dict(world=world, half=name, cars=half, steps=steps_ab, car_steps=int(driven[sel].sum()),
                                  moved=int(c["moved"][sel].sum()), cars_moved=int((c["moved"][sel] > 0).sum()),
                                  kept=int(c["kept"][sel].sum()), infeasible_or_inaccurate_steps=int(bad[sel].sum()),
                                  contact_steps=int(a["contact_steps"][sel].sum()), cars_with_contact=int((a["contact_steps"][sel] > 0).sum()),
                                  alive={str(k): v for k, v in ends.items()})), flush=True)
    h.close()


if __name__ == "__main__":
    main()
