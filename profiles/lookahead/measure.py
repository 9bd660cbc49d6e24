"""Per-step time of the device rollout with and without lookahead (K0h + K0c<., true>), against the library of the commit
before, and what the lookahead does to a fleet that crossing movers cut off.

    python profiles/lookahead/measure.py [--parent-lib PATH/libmpmpc.so] [--quick] [--no-effect]

Sim_Track, N = 30, cars spread over the path, B = 1 024 / 8 192, the worlds of profiles/movers/step_cost.py.  Cases, run in
turn `rounds` times in one process (whatever else the machine does hits all of them alike):
  parent_static   the parent commit's library (--parent-lib), 6 static discs per car
  static          this tree's library, lookahead never set, the same 6 static discs
  movers_off      this tree's library, 3 of those discs + 3 movers per car, lookahead off
  movers_on       the same world, lookahead on (seg_time = ds_next / v_ref, max_lead = 40)
One JSON line per case and round: ms per step = host clock over `steps` steps after `warmup`, the window closed by
rollout_state (a device synchronise); the cars still running / blocked at the end; whether the final state equals the first
case's of the same world (static = parent_static).  The kernels' own times come from a kernel trace of `--quick --no-effect`,
a run of its own (README.md).

The effect: B = 1 024 cars, each with one mover crossing the track 12 .. 25 waypoints ahead of it within the first 25 steps,
audit on (footprint 0.12 m x 0.06 m), 40 steps, lookahead off against on: cars still running, cars that ended blocked (-3)
or infeasible (-1), cars with a contact step and contact steps in all."""
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in ("multi-purpose-mpc_amd", "tests", "oracle", "profiles/movers", ""):
    sys.path.insert(0, os.path.join(ROOT, p))

import numpy as np  # noqa: E402

import movers  # noqa: E402
import mpmpc  # noqa: E402
import scenarios  # noqa: E402
import step_cost as SC  # noqa: E402
from lookahead import Lookahead  # noqa: E402
from map import Map, Obstacle  # noqa: E402

TS, N, MAX_LEAD = SC.TS, SC.N, 40


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
    seg = Lookahead.seg_time_of(tr.ds_next, tr.v_ref)
    warmup, steps, rounds = (3, 10, 2) if quick else (5, 40, 5)
    new = mpmpc.load_library()
    print(json.dumps(dict(library=new.mpmpc_version().decode(),
                          parent=SC.older_library(parent).mpmpc_version().decode() if parent else None)), flush=True)
    for B in (1024, 8192):
        rng = np.random.default_rng(B)
        starts = rng.integers(0, n_wp, B)
        poses = np.stack([g1["x"][starts], g1["y"][starts], g1["psi"][starts]], 1)
        static6, rows = [], []
        for b in range(B):
            static6.append(m.obstacle_discs([Obstacle(c[0] + rng.uniform(-0.05, 0.05), c[1] + rng.uniform(-0.05, 0.05),
                                                      rng.uniform(0.04, 0.07)) for c in SC.NINE[:6]]))
            w0 = int(starts[b])
            mv = [movers.Mover.along_path(cum[(w0 + int(rng.integers(5, 26))) % n_wp], rng.uniform(-0.08, 0.08),
                                          rng.uniform(1 / 3, 2 / 3) * tr.v_ref[w0], rng.uniform(0.03, 0.05)) for _ in range(2)]
            wc = (w0 + int(rng.integers(10, 30))) % n_wp
            nx, ny = -math.sin(g1["psi"][wc]), math.cos(g1["psi"][wc])
            mv.append(movers.Mover.line(g1["x"][wc] - 0.3 * nx, g1["y"][wc] - 0.3 * ny, 0.6 * nx / (steps * TS),
                                        0.6 * ny / (steps * TS), rng.uniform(0.03, 0.05)))
            rows.append(np.array([q.row(TS, m.resolution) for q in mv]))
        static3 = [d[:3] for d in static6]
        h_new = SC.handle(new, B, tr, g1, grid, sm)
        h_old = SC.handle(SC.older_library(parent), B, tr, g1, grid, sm) if parent else None

        def timed(h):
            h.rollout_init(TS, cum, cum[starts], poses)
            h.rollout_step(warmup)
            h.rollout_state()
            t0 = time.perf_counter()
            h.rollout_step(steps)
            st = h.rollout_state()
            return (time.perf_counter() - t0) / steps, st

        first = {}
        for r in range(rounds):
            for case in ("parent_static", "static", "movers_off", "movers_on"):
                if case == "parent_static":
                    if not h_old:
                        continue
                    h_old.rollout_set_obstacles(static6)
                    dt, st = timed(h_old)
                elif case == "static":
                    h_new.rollout_set_lookahead(None)
                    h_new.rollout_set_movers(None)
                    h_new.rollout_set_obstacles(static6)
                    dt, st = timed(h_new)
                else:
                    h_new.rollout_set_obstacles(static3)
                    h_new.rollout_set_movers(rows)
                    h_new.rollout_set_lookahead(seg if case == "movers_on" else None, MAX_LEAD)
                    dt, st = timed(h_new)
                world = "six" if case in ("parent_static", "static") else case
                ref = first.setdefault(world, st)
                print(json.dumps(dict(B=B, N=N, case=case, round=r, ms_per_step=round(dt * 1e3, 4),
                                      running=int((st["alive"] == 1).sum()), blocked=int((st["alive"] == -3).sum()),
                                      same_as_first=bool(all(np.array_equal(st[k], ref[k]) for k in SC.KEYS)))), flush=True)
        h_new.close()
        if h_old:
            h_old.close()
    if "--no-effect" in sys.argv:
        return
    # ---- the effect: one crossing mover per car, audit on
    B, steps = 1024, 40
    rng = np.random.default_rng(7)
    starts = rng.integers(0, n_wp, B)
    poses = np.stack([g1["x"][starts], g1["y"][starts], g1["psi"][starts]], 1)
    rows = []
    for b in range(B):
        wc = (int(starts[b]) + int(rng.integers(12, 26))) % n_wp
        nx, ny = -math.sin(g1["psi"][wc]), math.cos(g1["psi"][wc])
        side, t_cross = rng.choice([-1.0, 1.0]), int(rng.integers(10, 26))      # reaches the centre line at step t_cross
        rows.append(np.array([movers.Mover.line(g1["x"][wc] - side * 0.3 * nx, g1["y"][wc] - side * 0.3 * ny, side * 0.3 * nx / (t_cross * TS),
                                                side * 0.3 * ny / (t_cross * TS), rng.uniform(0.03, 0.05)).row(TS, m.resolution)]))
    h = SC.handle(new, B, tr, g1, grid, sm)
    h.rollout_set_movers(rows)
    h.rollout_set_audit(1, 0.12, 0.06, 0.1)
    for on in (False, True):
        h.rollout_set_lookahead(seg if on else None, MAX_LEAD)
        h.rollout_init(TS, cum, cum[starts], poses)
        h.rollout_step(steps)
        st, au = h.rollout_state(), h.rollout_audit()
        print(json.dumps(dict(effect=True, B=B, steps=steps, lookahead=on, running=int((st["alive"] == 1).sum()),
                              blocked=int((st["alive"] == -3).sum()), infeasible=int((st["alive"] == -1).sum()),
                              finished=int((st["alive"] == 0).sum()), cars_with_contact=int((au["contact_steps"] > 0).sum()),
                              contact_steps=int(au["contact_steps"].sum()), mean_s=round(float(np.mean(st["s"] - cum[starts])), 4))), flush=True)
    h.close()


if __name__ == "__main__":
    main()
