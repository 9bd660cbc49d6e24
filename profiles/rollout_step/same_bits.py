"""The rollout step of this tree against the library of the commit before, with everything on at once: the same rollouts on
both libraries in one process, every getter compared byte for byte.

    python profiles/rollout_step/same_bits.py --parent-lib PATH/libmpmpc.so

Sim_Track, N = 30, B = 8 cars in two traffic groups of 4 (S = 2 slots), 12 steps taken as one call of 5 steps and seven calls of
one.  Worlds: the shared table; one per instantiation of K0c (static discs; + walls; + movers and lookahead, without and with
walls; + traffic and its lookahead, without and with walls - the last one the richest); the richest again with perception, with
a plant, on the two fixture routes of tests/test_routes.py (the lap and its open second half), and with all three.  Every world
runs with the recorder at stride 2 and the audit on; the table and the richest world also run with both off.  After every call:
rollout_state, the whole trace, rollout_obstacles, rollout_corridor, rollout_lookahead, rollout_lookahead_traffic,
rollout_tracks, rollout_plant, rollout_audit and rollout_perception, where the world has them.  One JSON line per case; exit
status 1 on any difference, or when fewer than half of a world's cars are still running at the end (such a world would compare
little)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in ("multi-purpose-mpc_amd", "tests", "oracle", "profiles/movers", ""):
    sys.path.insert(0, os.path.join(ROOT, p))

import numpy as np  # noqa: E402

import mpmpc  # noqa: E402
import mpmpc_testlib as T  # noqa: E402
import scenarios  # noqa: E402
import step_cost as SC  # noqa: E402
import test_routes as TR  # noqa: E402
from lookahead import Lookahead  # noqa: E402
from plant import Plant  # noqa: E402

TS, N, B, S, MAX_LEAD = 0.05, 30, 8, 2, 40
CALLS = (5,) + (1,) * 7
LAP = np.array([130, 123, 116, 109, 160, 153, 146, 139])      # rows of the lap, all on its second half: both routes hold them
GROUP = (np.arange(B) // 4).astype(np.int32)


def fixture():
    """the per-car settings of the worlds, in map cells and arc lengths that mean the same on the lap and on the two routes"""
    own, cat, first, circ, grid, sm = TR._route_tables(scenarios.sim_track(), ["L", "Bo"])
    L = own[0]
    route = (np.arange(B) % 2).astype(np.int32)      # the cars of a group alternate between the routes
    discs, walls = [], []
    for i, w0 in enumerate(LAP):
        w = (w0 + 9) % 200
        discs.append(np.concatenate([TR._cells(L["border_ub"][w]), [[3]]], 1).astype(np.int32))
        w = (w0 + 14) % 200
        a, c = TR._cells(L["border_lb"][w])[0], TR._cells([L["x"][w], L["y"][w]])[0]
        walls.append(np.array([[a[0], a[1], a[0] + (c[0] - a[0]) // 3, a[1] + (c[1] - a[1]) // 3]], np.int32) if i % 2 else np.zeros((0, 4), np.int32))

    def movers(s):      # one straight-line and one along-the-path mover per car; s: the cars' arc lengths on their own paths
        out = []
        for i, w0 in enumerate(LAP):
            w2 = (w0 + 20) % 200
            out.append(np.array([[0, 2, L["border_lb"][w2][0], L["border_lb"][w2][1], 0.001, -0.001], [1, 2, s[i] + 0.9, -0.08, 0.004, 0.0]]))
        return out

    one = dict(tab=L, circular=True, routes=None, car_routes=None, s=L["cum_lengths"][LAP], grid=grid, sm=sm)
    wp = np.where(route == 1, LAP - 100, LAP)
    rows = np.asarray(first, np.int64)[route] + wp
    two = dict(tab=cat, circular=False, routes=(first, circ), car_routes=route, s=np.asarray(cat["cum_lengths"], float)[rows], grid=grid, sm=sm)
    poses = np.stack([L["x"][LAP], L["y"][LAP], L["psi"][LAP]], 1)
    return one, two, poses, discs, walls, movers


def worlds():
    """name -> the set of features in force"""
    w = {"table": set(), "K0c<false>": {"discs"}, "K0c<true>": {"discs", "walls"}, "K0c<false,true>": {"discs", "movers", "look"},
         "K0c<true,true>": {"discs", "walls", "movers", "look"}, "K0c<false,true,true>": {"discs", "movers", "traffic", "look", "ahead"}}
    rich = {"discs", "walls", "movers", "traffic", "look", "ahead"}
    w["K0c<true,true,true>"] = rich
    w["richest+perception"] = rich | {"perception"}
    w["richest+plant"] = rich | {"plant"}
    w["richest+routes"] = rich | {"routes"}
    w["richest+perception+plant+routes"] = rich | {"perception", "plant", "routes"}
    out = {k: v | {"record", "audit"} for k, v in w.items()}
    out["table, no recorder, no audit"] = set()
    out["richest, no recorder, no audit"] = rich
    return out


def flat(x, out, where):
    """every array below x as (where, bytes)"""
    if isinstance(x, dict):
        for k in sorted(x):
            flat(x[k], out, where + "." + str(k))
    elif isinstance(x, (tuple, list)):
        for i, v in enumerate(x):
            flat(v, out, "%s[%d]" % (where, i))
    else:
        a = np.ascontiguousarray(x)
        out.append((where, str(a.dtype) + str(a.shape), a.tobytes()))


def run(lib, on, fx):
    one, two, poses, discs, walls, movers = fx
    p = two if "routes" in on else one
    keep, mpmpc._lib = mpmpc._lib, lib
    try:
        h = mpmpc.Handle(T.stock_config(N, max_batch=B, circular=p["circular"]), mpmpc.default_settings())
    finally:
        mpmpc._lib = keep
    try:
        tab = p["tab"]
        h.set_path(tab["kappa"], tab["v_ref"], tab["ds_next"])
        if p["routes"] is not None:
            h.set_routes(*p["routes"])
        h.set_map(p["grid"], (-1.0, -2.0), 0.005)
        h.set_path_geometry(tab["x"], tab["y"], tab["psi"], tab["border_ub"], tab["border_lb"])
        assert h.build_corridor(N, 2 * p["sm"], p["sm"], want_tables=False)[2] == 0
        if p["car_routes"] is not None:
            h.set_car_routes(p["car_routes"])
        if "walls" in on:
            h.rollout_set_walls(walls)
        if "discs" in on:
            h.rollout_set_obstacles(discs)
        if "movers" in on:
            h.rollout_set_movers(movers(p["s"]))
        if "traffic" in on:
            h.rollout_set_traffic(GROUP, np.full(B, 5, np.int32), S, 120)
        if "look" in on:
            h.rollout_set_lookahead(Lookahead.seg_time_of(tab["ds_next"], tab["v_ref"]), MAX_LEAD)
        if "ahead" in on:
            h.rollout_set_lookahead_traffic(True)
        if "audit" in on:
            h.rollout_set_audit(1, 0.12, 0.06, 0.1)
        if "perception" in on:
            h.rollout_set_perception(np.linspace(-1.2, 1.2, 25), 1.0, 2)
        if "plant" in on:
            pl = Plant(speed_gain=0.97, steer_gain=1.03, steer_offset=0.004, speed_lag=0.8, steer_lag=0.7, steer_rate=0.2, speed_noise=0.01,
                       steer_noise=0.004, position_noise=0.002, heading_noise=0.002, seed=11)
            h.rollout_set_plant(pl.params(B), seed=pl.seed, car0=pl.car0, step0=pl.step0)
        if "record" in on:
            h.rollout_record(sum(CALLS), plan=True, prediction=True, rows=True, stride=2, B=B)
        h.rollout_init(TS, tab["cum_lengths"], p["s"], poses)
        got = []
        for c, n in enumerate(CALLS):
            h.rollout_step(n)
            snap = dict(state=h.rollout_state())
            if "record" in on:
                snap["trace"] = h.rollout_trace()
            if "discs" in on:
                snap["obstacles"] = h.rollout_obstacles()
                snap["corridor"] = h.rollout_corridor()
            if "look" in on:
                snap["lookahead"] = h.rollout_lookahead()
            if "ahead" in on:
                snap["lookahead_traffic"] = h.rollout_lookahead_traffic()
                snap["tracks"] = h.rollout_tracks()
            if "plant" in on:
                snap["plant"] = h.rollout_plant()
            if "audit" in on:
                snap["audit"] = h.rollout_audit()
            if "perception" in on:
                snap["perception"] = h.rollout_perception()
            flat(snap, got, "call %d" % c)
        return got, int((snap["state"]["alive"] == 1).sum())
    finally:
        h.close()


def main():
    new = mpmpc.load_library()
    old = SC.older_library(sys.argv[sys.argv.index("--parent-lib") + 1])
    print(json.dumps(dict(library=new.mpmpc_version().decode(), parent=old.mpmpc_version().decode())), flush=True)
    fx = fixture()
    bad = 0
    for name, on in worlds().items():
        a, running = run(new, on, fx)
        b, running_parent = run(old, on, fx)
        differ = [x[0] for x, y in zip(a, b) if x != y]
        ok = len(a) == len(b) and not differ and running == running_parent and 2 * running >= B
        bad += not ok
        print(json.dumps(dict(case=name, running=running, of=B, arrays=len(a), bytes=sum(len(x[2]) for x in a), identical=not differ and len(a) == len(b),
                              first_differences=differ[:4])), flush=True)
    print(json.dumps(dict(cases=len(worlds()), failed=bad)), flush=True)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
