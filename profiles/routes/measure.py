"""Route fleets: what they cost, and that a handle without routes costs what it did (profiles/routes/README.md).

    python profiles/routes/measure.py --parent-pkg OTHER/multi-purpose-mpc_amd [--rounds 5]     # 1: no regression without routes
    python profiles/routes/measure.py --copies                                         # 2: cost of the feature
    python profiles/routes/measure.py --fleet                                          # 3: one fleet (solve; rollout) against 64 solo handles

Every figure comes from a child process of its own (a fresh HIP context per library and measurement); part 1 alternates this
tree's package with another checkout's (the parent commit's multi-purpose-mpc_amd directory with its built libmpmpc.so: its
Python and its library), `--rounds` children each.  Resident rate: config 2's batch (scenarios.make(2, B)) uploaded once, K resident launches
as bench.py issues them (pipelined inside the handle), one sync, host clock around both; the median of R such windows.
K3 step: mpmpc_rollout_step(n) followed by mpmpc_rollout_state, host clock, per step.  One JSON line per child."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "multi-purpose-mpc_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def _handle(B, copies, N=30):
    """a handle on `copies` copies of the Sim_Track lap (0: the lap as ONE path, no routes), config 2's batch uploaded"""
    import numpy as np
    import mpmpc
    import mpmpc_testlib as T
    import scenarios
    tr = scenarios.sim_track()
    sc = scenarios.make(2, tr, B=B)
    h = mpmpc.Handle(T.stock_config(N, max_batch=B), mpmpc.default_settings())
    own = dict(kappa=tr.kappa, v_ref=tr.v_ref, ds_next=tr.ds_next, ub=tr.ub_free[:, :N], lb=tr.lb_free[:, :N])
    if copies:
        cat, first = mpmpc.concat_routes([own] * copies)
        h.set_path(cat["kappa"], cat["v_ref"], cat["ds_next"])
        h.set_corridor(cat["ub"], cat["lb"])
        h.set_routes(first, np.ones(copies, np.int32))
        h.set_car_routes(np.arange(B) % copies)
    else:
        h.set_path(own["kappa"], own["v_ref"], own["ds_next"])
        h.set_corridor(own["ub"], own["lb"])
    h.upload(sc.wp_id, sc.x0, sc.cc_prev)
    return h, tr, sc


def resident_rate(B, copies, K=200, R=15, warm=300):
    h, _, _ = _handle(B, copies)
    for _ in range(warm):
        h.solve_resident(B)
    h.sync()
    rates = []
    for _ in range(R):
        t0 = time.perf_counter()
        for _ in range(K):
            h.solve_resident(B)
        h.sync()
        rates.append(K * B / (time.perf_counter() - t0))
    sol = h.download(B)
    h.close()
    return statistics.median(rates), float((sol.status == 1).mean())


def _rollout_ready(h, tr, copies):
    """the geometry of `copies` copies of the lap (0: the lap itself) on the handle -> (g1, cum_lengths for rollout_init)"""
    import numpy as np
    g1 = np.load(os.path.join(ROOT, "tests", "golden", "g1_path_sim_track.npz"))
    c = max(copies, 1)
    h.set_path_geometry(*(np.concatenate([g1[k]] * c) for k in ("x", "y", "psi", "border_ub", "border_lb")))
    return g1, np.concatenate([np.cumsum(tr.segment_lengths)] * c)


def k3_step_ms(B, copies=0, n=100, R=5, warm=20):
    import numpy as np
    h, tr, _ = _handle(B, copies)
    g1, cum = _rollout_ready(h, tr, copies)
    starts = np.random.default_rng(3).integers(0, 200, B)
    poses = np.stack([g1["x"][starts], g1["y"][starts], g1["psi"][starts]], axis=1)
    out = []
    for _ in range(R):
        h.rollout_init(0.05, cum, cum[starts], poses)          # (cum[starts]: local arc lengths - the first copy's rows)
        h.rollout_step(warm)
        h.rollout_state()
        t0 = time.perf_counter()
        h.rollout_step(n)
        st = h.rollout_state()
        out.append(1e3 * (time.perf_counter() - t0) / n)
    h.close()
    return statistics.median(out), float((st["alive"] == 1).mean())


def fleet_against_solo(P=64, cars=16, K=50, R=7, N=30):
    """P routes x `cars` instances: ONE handle with routes, one resident launch of P * cars instances - against P single-path
    handles of `cars` instances each (what a user had to do without routes), all launched before any is waited for."""
    import numpy as np
    import mpmpc
    B = P * cars
    h, tr, sc = _handle(B, P)
    solo = []
    for p in range(P):
        idx = np.flatnonzero(np.arange(B) % P == p)
        s = mpmpc.Handle(__import__("mpmpc_testlib").stock_config(N, max_batch=cars), mpmpc.default_settings())
        s.set_path(tr.kappa, tr.v_ref, tr.ds_next)
        s.set_corridor(tr.ub_free[:, :N], tr.lb_free[:, :N])
        s.upload(sc.wp_id[idx], sc.x0[idx], sc.cc_prev[idx])
        solo.append(s)

    def one_fleet():
        h.solve_resident(B)
        h.sync()

    def one_solo():          # every handle's launch enqueued first (each on its own stream), then waited for: nothing serialised by the host
        for s in solo:
            s.solve_resident(cars)
        for s in solo:
            s.sync()
    out = {}
    for name, f in (("fleet", one_fleet), ("solo", one_solo)):
        for _ in range(10):
            f()
        ts = []
        for _ in range(R):
            t0 = time.perf_counter()
            for _ in range(K):
                f()
            ts.append(1e3 * (time.perf_counter() - t0) / K)
        out[name + "_ms"] = statistics.median(ts)
    a = h.download(B)
    same = all(np.array_equal(s.download(cars).u0, a.u0[np.arange(B) % P == p]) for p, s in enumerate(solo))
    for s in solo:
        s.close()
    h.close()
    out.update(P=P, cars=cars, factor=out["solo_ms"] / out["fleet_ms"], same_controls=bool(same))
    return out


def fleet_rollout_against_solo(P=64, cars=16, n=20, R=5, N=30):
    """P routes x `cars` cars in closed loop for n steps: ONE route-fleet rollout (rollout_step(n), then rollout_state) against P
    single-path handles of `cars` cars - every handle's n steps enqueued before any state is read ("together"), and one
    handle after the other ("in turn": steps and state, then the next)."""
    import numpy as np
    import mpmpc
    B = P * cars
    h, tr, _ = _handle(B, P)
    g1, cum = _rollout_ready(h, tr, P)
    lap = np.cumsum(tr.segment_lengths)
    starts = np.random.default_rng(3).integers(0, 200, B)
    poses = np.stack([g1["x"][starts], g1["y"][starts], g1["psi"][starts]], axis=1)
    solo = []
    for p in range(P):
        s, _, _ = _handle(cars, 0)
        _rollout_ready(s, tr, 0)
        solo.append(s)
    idx = [np.flatnonzero(np.arange(B) % P == p) for p in range(P)]

    def start():
        h.rollout_init(0.05, cum, lap[starts], poses)
        for p, s in enumerate(solo):
            s.rollout_init(0.05, lap, lap[starts[idx[p]]], poses[idx[p]])
    out = {}
    last = {}
    for name in ("fleet", "solo_together", "solo_in_turn"):
        ts = []
        for _ in range(R + 1):
            start()
            t0 = time.perf_counter()
            if name == "fleet":
                h.rollout_step(n)
                last[name] = h.rollout_state()
            elif name == "solo_together":
                for s in solo:
                    s.rollout_step(n)
                last[name] = [s.rollout_state() for s in solo]
            else:
                last[name] = []
                for s in solo:
                    s.rollout_step(n)
                    last[name].append(s.rollout_state())
            ts.append(1e3 * (time.perf_counter() - t0) / n)
        out[name + "_ms_per_step"] = statistics.median(ts[1:])
    same = all(np.array_equal(st["alive"], last["fleet"]["alive"][idx[p]]) and np.abs(st["s"] - last["fleet"]["s"][idx[p]]).max() <= 1e-8
               for p, st in enumerate(last["solo_together"]))
    for s in solo:
        s.close()
    h.close()
    out.update(P=P, cars=cars, steps=n, factor_together=out["solo_together_ms_per_step"] / out["fleet_ms_per_step"],
               factor_in_turn=out["solo_in_turn_ms_per_step"] / out["fleet_ms_per_step"], same_states=bool(same))
    return out


def child(args):
    if args.pkg:          # another checkout's package: its mpmpc.py and the libmpmpc.so beside it (imported before anything else is)
        sys.path.insert(0, os.path.abspath(args.pkg))
    import mpmpc
    if args.child == "baseline":
        out = dict(pkg=os.path.dirname(mpmpc.LIB_PATH), version=mpmpc.load_library().mpmpc_version().decode())
        for B in (1024, 8192):
            out["resident_%d" % B], out["solved_%d" % B] = resident_rate(B, 0)
            out["k3_ms_%d" % B], out["alive_%d" % B] = k3_step_ms(B)
    elif args.child == "copies":
        out = dict(copies=args.n)
        for B in (1024, 8192):
            out["resident_%d" % B], out["solved_%d" % B] = resident_rate(B, args.n)
            out["k3_ms_%d" % B], out["alive_%d" % B] = k3_step_ms(B, args.n)
    elif args.child == "fleet":
        out = fleet_against_solo()
    else:
        out = fleet_rollout_against_solo()
    print(json.dumps(out), flush=True)


def run_child(*extra):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + list(extra), capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise SystemExit("child %r failed (%d): %s" % (extra, r.returncode, r.stderr[-2000:]))
    line = r.stdout.strip().splitlines()[-1]
    print(line, flush=True)
    return json.loads(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-pkg")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--copies", action="store_true")
    ap.add_argument("--fleet", action="store_true")
    ap.add_argument("--child")
    ap.add_argument("--pkg")
    ap.add_argument("--n", type=int, default=0)
    args = ap.parse_args()
    if args.child:
        return child(args)
    if args.parent_pkg:
        rows = {"parent": [], "branch": []}
        for _ in range(args.rounds):
            rows["parent"].append(run_child("--child", "baseline", "--pkg", args.parent_pkg))
            rows["branch"].append(run_child("--child", "baseline"))
        for key in ("resident_1024", "resident_8192", "k3_ms_1024", "k3_ms_8192"):
            for who in ("parent", "branch"):
                v = [r[key] for r in rows[who]]
                print("%-14s %-7s median %.6g  min %.6g  max %.6g" % (key, who, statistics.median(v), min(v), max(v)), flush=True)
    if args.copies:
        for n in (0, 1, 4, 64):
            run_child("--child", "copies", "--n", str(n))
    if args.fleet:
        run_child("--child", "fleet")
        run_child("--child", "fleet_rollout")


if __name__ == "__main__":
    main()
