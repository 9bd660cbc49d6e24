"""Generate G3o / G6o (per-car obstacle worlds) by IMPORTING the reference, like make_golden.py (same interpreter, cwd =
the reference's src/, the stand-in osqp):

    cd <reference>/src && MPLBACKEND=Agg python3.9 -W ignore <this repository>/tests/golden/make_g3o.py [g3o] [g6o]

Everything written is DATA: the obstacle sets, their discs in map cells and the reference's outputs on them.

  g3o   g3o_sim_obstacles.npz / g3o_real_obstacles.npz: for seeded obstacle sets (jittered copies of the obstacles of
        src/simulation.py:40-48 on Sim_Track, of src/simulation.py:73-80 on Real_Track), the reference's
        update_path_constraints(w + 1, 30, 2 sm, sm) for every start waypoint w after Map.add_obstacles (Real_Track, an
        open path: only w + 30 < n_wp); NaN rows + blocked flag where the reference raises (no free segment at the first
        horizon waypoint).
  g6o   g6o_closed_loop_N30.npz: the closed loop of src/simulation.py:134-140 (N = 30) in the first 3 Sim_Track worlds,
        G6's record layout per world (without z and cc_next: the next step's cc_prev), concatenated (world[k] = which world a step belongs to).
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402  (sets up the stand-in osqp and the reference's flat imports)

import numpy as np  # noqa: E402
from map import Obstacle  # noqa: E402
from spatial_bicycle_models import BicycleModel  # noqa: E402

NCOL = 30
SIM_SETS, REAL_SETS = 6, 2


def discs_of(m, obstacles):
    """the integer discs Map.add_obstacles rasterises (src/map.py:129-133)"""
    out = []
    for ob in obstacles:
        r = int(np.ceil(ob.radius / m.resolution))
        cx, cy = m.w2m(ob.cx, ob.cy)
        out.append((cx, cy, r))
    return np.array(out, np.int32).reshape(-1, 3)


def sim_sets():
    sets = []
    for k in range(SIM_SETS):
        rng = np.random.default_rng(1000 + k)
        obs = [(c[0] + rng.uniform(-0.05, 0.05), c[1] + rng.uniform(-0.05, 0.05), rng.uniform(0.04, 0.09))
               for c in G.OBSTACLES]
        if k == SIM_SETS - 1:
            # two discs across the straight at x = 0, y in [-1.5, -0.5]: blocks the start waypoints whose border line
            # passes there completely (the reference raises)
            obs += [(-0.25 + 0.06, -1.0, 0.09), (-0.25 - 0.06, -1.0, 0.09)]
        sets.append(obs)
    return sets


def real_sets():
    sets = []
    for k in range(REAL_SETS):
        rng = np.random.default_rng(2000 + k)
        sets.append([(c[0] + rng.uniform(-0.2, 0.2), c[1] + rng.uniform(-0.2, 0.2), c[2] * rng.uniform(0.8, 1.2))
                     for c in G.REAL_OBSTACLES])
    return sets


def rows(rp, sm, n_start):
    n = n_start
    ub, lb = np.full((n, NCOL), np.nan), np.full((n, NCOL), np.nan)
    blocked = np.zeros(n, bool)
    for w in range(n):
        try:
            u, l, _ = rp.update_path_constraints(w + 1, NCOL, 2 * sm, sm)
            ub[w], lb[w] = u, l
        except ValueError:      # max([]): no free segment at the first horizon waypoint
            blocked[w] = True
    return ub, lb, blocked


def stage_g3o():
    out = {}
    for k, obs in enumerate(sim_sets()):
        m, rp = G.build_track()
        sm = BicycleModel(reference_path=rp, **G.CAR).safety_margin
        o = [Obstacle(cx=c[0], cy=c[1], radius=c[2]) for c in obs]
        out["discs_%d" % k] = discs_of(m, o)
        out["obstacles_%d" % k] = np.array(obs, float)
        m.add_obstacles(o)
        out["ub_%d" % k], out["lb_%d" % k], out["blocked_%d" % k] = rows(rp, sm, rp.n_waypoints)
        print("G3o sim %d: %d discs, blocked rows %d" % (k, len(obs), out["blocked_%d" % k].sum()))
    np.savez_compressed(os.path.join(HERE, "g3o_sim_obstacles.npz"), n_sets=np.array([SIM_SETS]),
                        n_cols=np.array([NCOL]), safety_margin=np.array([sm]), **out)
    out = {}
    for k, obs in enumerate(real_sets()):
        m, rp = G.build_real_track()
        sm = BicycleModel(reference_path=rp, **G.REAL_CAR).safety_margin
        o = [Obstacle(cx=c[0], cy=c[1], radius=c[2]) for c in obs]
        out["discs_%d" % k] = discs_of(m, o)
        out["obstacles_%d" % k] = np.array(obs, float)
        m.add_obstacles(o)
        n_start = rp.n_waypoints - NCOL      # w + 30 < n_wp: the reference exits past that
        out["ub_%d" % k], out["lb_%d" % k], out["blocked_%d" % k] = rows(rp, sm, n_start)
        print("G3o real %d: %d discs, %d start waypoints, blocked rows %d" % (k, len(obs), n_start,
                                                                             out["blocked_%d" % k].sum()))
    np.savez_compressed(os.path.join(HERE, "g3o_real_obstacles.npz"), n_sets=np.array([REAL_SETS]),
                        n_cols=np.array([NCOL]), safety_margin=np.array([sm]), **out)


def stage_g6o(worlds=(0, 1, 2)):
    import osqp
    N = NCOL
    keys = ("s", "pose", "cc_prev", "wp_id", "x0", "lb", "ub", "status", "u", "counter")      # (size: no z; cc_next = next cc_prev)
    rec = {k: [] for k in keys + ("world",)}
    sets = sim_sets()
    discs, exited = {}, []
    for wi in worlds:
        m, rp = G.build_track()
        o = [Obstacle(cx=c[0], cy=c[1], radius=c[2]) for c in sets[wi]]
        discs["discs_%d" % wi] = discs_of(m, o)
        m.add_obstacles(o)
        car, mpc = G.make_controller(rp, N, "stock")
        rp.compute_speed_profile(dict(G.SPEED))
        ex = False
        while car.s < rp.length:
            s, pose = car.s, [car.temporal_state.x, car.temporal_state.y, car.temporal_state.psi]
            cc_prev = mpc.current_control.copy()
            osqp.CAPTURES.clear()
            try:
                u = mpc.get_control()
            except SystemExit:
                ex = True
                break
            res = osqp.CAPTURES[-1]["res"]
            ub, lb, _ = rp.update_path_constraints(car.wp_id + 1, N, 2 * car.safety_margin, car.safety_margin)
            for k, v in (("s", s), ("pose", pose), ("cc_prev", cc_prev), ("wp_id", car.wp_id),
                         ("x0", car.spatial_state[:]), ("lb", lb), ("ub", ub), ("status", res.status),
                         ("u", np.array(u, float)), ("counter", mpc.infeasibility_counter), ("world", wi)):
                rec[k].append(v)
            car.drive(u)
        exited.append(ex)
        print("G6o world %d: %d steps, exit(1) %s" % (wi, sum(1 for w in rec["world"] if w == wi), ex))
    np.savez_compressed(os.path.join(HERE, "g6o_closed_loop_N30.npz"), **{k: np.array(v) for k, v in rec.items()},
                        N=np.array([N]), worlds=np.array(worlds), exited=np.array(exited), **discs)


if __name__ == "__main__":
    stages = sys.argv[1:] or ["g3o", "g6o"]
    if "g3o" in stages:
        stage_g3o()
    if "g6o" in stages:
        stage_g6o()
