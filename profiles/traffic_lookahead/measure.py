"""Per-step time of the device rollout with traffic, with the traffic lookahead off and on (K3t, K0ht, K0c<., true, true>),
against the library of the commit before, and what the traffic lookahead does to the drive of a fleet on two routes.

    python profiles/traffic_lookahead/measure.py [--parent-lib PATH/libmpmpc.so [--parent-first]] [--quick] [--no-effect] [--only B]

Sim_Track, N = 30, B = 1 024 / 8 192 cars in groups of 8 that follow each other 5 .. 9 waypoints apart in the same lane, S = 4
slots, no range limit, radius 6 .. 10 cells; the movers of profiles/lookahead/measure.py (two along the path, one crossing, per
car) where a case has movers.  Cases, run in turn `rounds` times in one process:
  parent_traffic       the parent commit's library (--parent-lib): traffic only
  traffic              this tree's library, the flag off: traffic only
  parent_look          the parent's library: traffic + 3 movers per car + lookahead (seg_time = ds_next / v_ref, max_lead = 40)
  look_off             this tree's library, the same world and lookahead, the flag off
  look_on              the same, the flag on
  traffic_look_on      traffic + lookahead without movers, the flag on
(odd rounds swap the two members of every pair).  One JSON line per case and round: ms per step = host clock over `steps`
= 200 steps after `warmup` = 5 (--quick: 10 after 3, two rounds), the window closed by
rollout_state (a device synchronise); the cars still running / blocked at the end; whether the final state equals the first
case's of the same world and setting.  The kernels' own times come from a kernel trace of `--quick --no-effect`, a run of its
own (README.md).

The effect: B = 1 024 cars on the two fixture routes of tests/test_routes.py - the lap and the open second half of it, which
merge - in groups of 8 whose cars alternate between the routes, audit on (footprint 0.12 m x 0.06 m), 60 steps, lookahead on,
the flag off against on: contact steps, minimum clearance, cars ended."""
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
import mpmpc_testlib as T  # noqa: E402
import scenarios  # noqa: E402
import step_cost as SC  # noqa: E402
from lookahead import Lookahead  # noqa: E402
from map import Map  # noqa: E402

TS, N, MAX_LEAD, S, GROUP = SC.TS, SC.N, 40, 4, 8


def groups_of(B, n_wp, rng):
    """starts, group, radius of B cars in groups of GROUP: a leader at a random waypoint, the others 5 .. 9 waypoints apart behind it"""
    starts, group = np.zeros(B, np.int64), np.arange(B) // GROUP
    for g in range(B // GROUP):
        w = int(rng.integers(0, n_wp))
        for k in range(GROUP):
            starts[g * GROUP + k] = w % n_wp
            w -= int(rng.integers(5, 10))
    return starts, group.astype(np.int32), rng.integers(6, 11, B).astype(np.int32)


def main():
    quick = "--quick" in sys.argv
    parent = sys.argv[sys.argv.index("--parent-lib") + 1] if "--parent-lib" in sys.argv else None
    only = int(sys.argv[sys.argv.index("--only") + 1]) if "--only" in sys.argv else None
    g1 = np.load(os.path.join(ROOT, "tests", "golden", "g1_path_sim_track.npz"))
    h_, w_ = g1["grid_shape"]
    grid = np.ascontiguousarray(np.unpackbits(g1["grid_free"])[:h_ * w_].reshape(h_, w_).astype(np.int8))
    tr = scenarios.sim_track()
    sm = float(np.load(os.path.join(ROOT, "tests", "golden", "g3o_sim_obstacles.npz"))["safety_margin"][0])
    m = Map.from_grid(grid, (-1.0, -2.0), 0.005)
    cum = np.cumsum(g1["segment_lengths"])
    n_wp = g1["x"].size
    seg = Lookahead.seg_time_of(tr.ds_next, tr.v_ref)
    warmup, steps, rounds = (3, 10, 2) if quick else (5, 200, 5)
    new = mpmpc.load_library()
    old = SC.older_library(parent) if parent else None
    print(json.dumps(dict(library=new.mpmpc_version().decode(), parent=old.mpmpc_version().decode() if old else None)), flush=True)
    for B in (1024, 8192):
        if only and B != only:
            continue
        rng = np.random.default_rng(B)
        starts, group, rad = groups_of(B, n_wp, rng)
        poses = np.stack([g1["x"][starts], g1["y"][starts], g1["psi"][starts]], 1)
        rows = []
        for b in range(B):
            w0 = int(starts[b])
            mv = [movers.Mover.along_path(cum[(w0 + int(rng.integers(5, 26))) % n_wp], rng.uniform(-0.08, 0.08),
                                          rng.uniform(1 / 3, 2 / 3) * tr.v_ref[w0], rng.uniform(0.03, 0.05)) for _ in range(2)]
            wc = (w0 + int(rng.integers(10, 30))) % n_wp
            nx, ny = -math.sin(g1["psi"][wc]), math.cos(g1["psi"][wc])
            mv.append(movers.Mover.line(g1["x"][wc] - 0.3 * nx, g1["y"][wc] - 0.3 * ny, 0.6 * nx / (steps * TS),
                                        0.6 * ny / (steps * TS), rng.uniform(0.03, 0.05)))
            rows.append(np.array([q.row(TS, m.resolution) for q in mv]))
        if "--parent-first" in sys.argv and old:      # (which handle is made first decides where its memory lies)
            h_old = SC.handle(old, B, tr, g1, grid, sm)
            h_new = SC.handle(new, B, tr, g1, grid, sm)
        else:
            h_new = SC.handle(new, B, tr, g1, grid, sm)
            h_old = SC.handle(old, B, tr, g1, grid, sm) if old else None

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
            order = ("parent_traffic", "traffic", "parent_look", "look_off", "look_on", "traffic_look_on")
            if r % 2:      # the two libraries alternate: whichever runs first in a pair, it is not always the same one
                order = ("traffic", "parent_traffic", "look_off", "parent_look", "traffic_look_on", "look_on")
            for case in order:
                h = h_old if case.startswith("parent") else h_new
                if h is None:
                    continue
                with_movers = case in ("parent_look", "look_off", "look_on")
                h.rollout_set_movers(rows if with_movers else None)
                h.rollout_set_traffic(group, rad, S, -1)
                h.rollout_set_lookahead(seg if case not in ("parent_traffic", "traffic") else None, MAX_LEAD)
                if h is h_new:
                    h.rollout_set_lookahead_traffic(case in ("look_on", "traffic_look_on"))
                dt, st = timed(h)
                world = dict(parent_traffic="t", traffic="t", parent_look="l", look_off="l").get(case, case)
                ref = first.setdefault(world, st)
                print(json.dumps(dict(B=B, N=N, case=case, round=r, ms_per_step=round(dt * 1e3, 4),
                                      running=int((st["alive"] == 1).sum()), blocked=int((st["alive"] == -3).sum()),
                                      same_as_first=bool(all(np.array_equal(st[k], ref[k]) for k in SC.KEYS)))), flush=True)
        h_new.close()
        if h_old:
            h_old.close()
    if "--no-effect" in sys.argv:
        return
    # ---- the effect: two routes that merge, groups that span them, audit on
    import test_routes as TR
    own, cat, first_row, circ, rgrid, rsm = TR._route_tables(tr, ["L", "Bo"])
    first_row = np.asarray(first_row, np.int64)
    B, steps = 1024, 60
    rng = np.random.default_rng(7)
    route, wp, group = np.zeros(B, np.int32), np.zeros(B, np.int64), (np.arange(B) // GROUP).astype(np.int32)
    for g in range(B // GROUP):
        lap = int(rng.integers(101, 120))      # the leader; the others BEHIND it, the last at lap - 56 at the most ...
        for k in range(GROUP):
            b = g * GROUP + k
            route[b] = (k + g) % 2 if lap >= 100 else 0      # ... alternating between the routes where both exist
            wp[b] = lap - 100 if route[b] else lap
            lap -= int(rng.integers(4, 9))
    rad = rng.integers(6, 11, B).astype(np.int32)
    rows_g = first_row[route] + wp
    s0 = np.asarray(cat["cum_lengths"], float)[rows_g]
    poses = np.stack([cat["x"][rows_g], cat["y"][rows_g], cat["psi"][rows_g]], 1)
    h = mpmpc.Handle(T.stock_config(N, max_batch=B, circular=False), mpmpc.default_settings())
    h.set_path(cat["kappa"], cat["v_ref"], cat["ds_next"])
    h.set_routes(first_row, circ)
    h.set_map(rgrid, (-1.0, -2.0), 0.005)
    h.set_path_geometry(cat["x"], cat["y"], cat["psi"], cat["border_ub"], cat["border_lb"])
    h.build_corridor(N, 2 * rsm, rsm, want_tables=False)
    h.set_car_routes(route)
    h.rollout_set_traffic(group, rad, S, -1)
    h.rollout_set_lookahead(Lookahead.seg_time_of(cat["ds_next"], cat["v_ref"]), MAX_LEAD)
    h.rollout_set_audit(1, 0.12, 0.06, 0.1)
    for on in (False, True):
        h.rollout_set_lookahead_traffic(on)
        h.rollout_init(TS, cat["cum_lengths"], s0, poses)
        h.rollout_step(steps)
        st, au = h.rollout_state(), h.rollout_audit()
        print(json.dumps(dict(effect=True, B=B, steps=steps, traffic_lookahead=on, running=int((st["alive"] == 1).sum()),
                              blocked=int((st["alive"] == -3).sum()), infeasible=int((st["alive"] == -1).sum()),
                              path_end=int((st["alive"] == -2).sum()), finished=int((st["alive"] == 0).sum()),
                              cars_with_contact=int((au["contact_steps"] > 0).sum()), contact_steps=int(au["contact_steps"].sum()),
                              min_clearance=round(float(au["min_clearance"].min()), 4),
                              median_min_clearance=round(float(np.median(au["min_clearance"])), 4),
                              mean_s=round(float(np.mean(st["s"] - s0)), 4))), flush=True)
    h.close()


if __name__ == "__main__":
    main()
