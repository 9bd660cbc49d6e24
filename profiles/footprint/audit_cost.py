"""What the footprint audit (K0f) costs: a rollout step with the audit off and on, against the library of the commit
before, on the shared corridor table and in per-car worlds.

    python profiles/footprint/audit_cost.py [--parent-lib PATH/libmpmpc.so] [--reach METRES] [--cases a,b] [--quick]

Sim_Track, N = 30, the stock car (0.12 m x 0.06 m).  B = 1 024 is the fleet of config 2 (scenarios.make(2): its start
waypoints, the shared table); B = 8 192 the same draw at that size.  --reach: how far clearances are measured (default: the
car's length, a window of 77 x 77 cells; 0.25 gives R = 64, 129 x 129).  Cases, run in turn `rounds` times in one process (so
that whatever else the machine does hits all of them alike), one JSON line per case and round:
  parent_steps   the parent commit's library (--parent-lib): one rollout_step(steps) call, shared table
  mode0          this tree's library, the same call, audit off
  mode1          ... audit on
  discs_mode0    6 static discs per car (K0c builds every car's rows), audit off
  discs_mode1    ... audit on
  audit_call     mpmpc.footprint_audit on the last state's poses and discs (kernel + uploads of grid, poses, discs)
ms per step / per call = host clock, the window closed by a device synchronise.  K0f's own time per launch comes from a
kernel trace of this script (a run of its own, no counters): README.md."""
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
    only = sys.argv[sys.argv.index("--cases") + 1].split(",") if "--cases" in sys.argv else None
    parent = sys.argv[sys.argv.index("--parent-lib") + 1] if "--parent-lib" in sys.argv else None
    length, width = scenarios.CAR_LENGTH, scenarios.CAR_WIDTH
    reach = float(sys.argv[sys.argv.index("--reach") + 1]) if "--reach" in sys.argv else length
    g1 = np.load(os.path.join(ROOT, "tests", "golden", "g1_path_sim_track.npz"))
    h_, w_ = g1["grid_shape"]
    grid = np.ascontiguousarray(np.unpackbits(g1["grid_free"])[:h_ * w_].reshape(h_, w_).astype(np.int8))
    tr = scenarios.sim_track()
    sm = float(np.load(os.path.join(ROOT, "tests", "golden", "g3o_sim_obstacles.npz"))["safety_margin"][0])
    m = Map.from_grid(grid, (-1.0, -2.0), 0.005)
    cum = np.cumsum(g1["segment_lengths"])
    warmup, steps, rounds = (3, 10, 2) if quick else (5, 40, 5)
    new = mpmpc.load_library()
    R = int((reach + 0.5 * np.hypot(length, width)) / m.resolution) + 1
    print(json.dumps(dict(library=new.mpmpc_version().decode(), parent=older_library(parent).mpmpc_version().decode() if parent else None,
                          length=length, width=width, reach=reach, R=R)), flush=True)
    for B in (1024, 8192):
        starts = scenarios.make(2, tr, B=B).wp_id
        rng = np.random.default_rng(B)
        poses = np.stack([g1["x"][starts], g1["y"][starts], g1["psi"][starts]], 1)
        static6 = [m.obstacle_discs([Obstacle(c[0] + rng.uniform(-0.05, 0.05), c[1] + rng.uniform(-0.05, 0.05),
                                              rng.uniform(0.04, 0.07)) for c in NINE[:6]]) for _ in range(B)]
        h_new = handle(new, B, tr, g1, grid, sm)
        h_old = handle(older_library(parent), B, tr, g1, grid, sm) if parent else None

        def timed(h, mode, discs):
            """-> s per step of one rollout_step(steps) call after `warmup` steps, the final state, the audit"""
            h.rollout_set_obstacles(static6 if discs else None)
            if h is h_new:
                h.rollout_set_audit(mode, length, width, reach)
            h.rollout_init(TS, cum, cum[starts], poses)
            h.rollout_step(warmup)
            h.rollout_state()
            t0 = time.perf_counter()
            h.rollout_step(steps)
            st = h.rollout_state()
            return (time.perf_counter() - t0) / steps, st, (h.rollout_audit() if mode else None)

        first = {}
        for r in range(rounds):
            for case in ("parent_steps", "mode0", "mode1", "discs_mode0", "discs_mode1", "audit_call"):
                extra = {}
                discs = case.startswith("discs")
                if only and case not in only:
                    continue
                if case == "parent_steps":
                    if not h_old:
                        continue
                    dt, st, _ = timed(h_old, 0, False)
                elif case == "audit_call":
                    st = h_new.rollout_state()
                    lists = h_new.rollout_obstacles()
                    mpmpc.footprint_audit(grid, m.origin, m.resolution, st["pose"], length, width, reach, lists)
                    t0 = time.perf_counter()
                    for _ in range(steps):
                        con, clr = mpmpc.footprint_audit(grid, m.origin, m.resolution, st["pose"], length, width, reach, lists)
                    dt = (time.perf_counter() - t0) / steps
                    extra = dict(contacts=int(con.sum()), at_reach=int((clr == reach).sum()), discs=True)
                    discs = True
                else:
                    dt, st, aud = timed(h_new, int(case.endswith("1")), discs)
                    if aud:
                        extra = dict(cars_with_contact=int((aud["contact_steps"] > 0).sum()), contact_steps=int(aud["contact_steps"].sum()),
                                     cars_never_within_reach=int((aud["min_step"] < 0).sum()))
                ref = first.setdefault(discs, st)
                print(json.dumps(dict(B=B, N=N, case=case, round=r, ms=round(dt * 1e3, 4), running=int((st["alive"] == 1).sum()),
                                      same_as_first=bool(all(np.array_equal(st[k], ref[k]) for k in KEYS)), **extra)), flush=True)
        h_new.close()
        if h_old:
            h_old.close()


if __name__ == "__main__":
    main()
