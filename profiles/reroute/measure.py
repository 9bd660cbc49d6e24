"""Re-routing a running rollout and projecting poses: what the calls cost and what they replace (profiles/reroute/README.md).

    python profiles/reroute/measure.py --reroute                                   # a: mpmpc_rollout_reroute against the host detour
    python profiles/reroute/measure.py --project                                   # b: mpmpc_project against the numpy restatement
    python profiles/reroute/measure.py --parent-pkg OTHER/multi-purpose-mpc_amd [--rounds 5]     # c: K3 step of a route fleet that never re-routes

Every figure comes from a child process of its own (a fresh HIP context per measurement); part c alternates this tree's package
with another checkout's (the parent commit's multi-purpose-mpc_amd directory with its built libmpmpc.so), `--rounds` children
each.  Host clock around calls that end with the device drained; warm-up first; medians with min and max.  One JSON line per child."""
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

SPANS = (("L", 0, 200, 1), ("A", 0, 120, 0), ("Bo", 100, 200, 0))      # the fixture routes of tests/test_reroute.py


def _routes(N):
    import numpy as np
    import mpmpc
    import scenarios
    tr = scenarios.sim_track()
    cum = np.cumsum(tr.segment_lengths)
    own = [dict(kappa=tr.kappa[lo:hi], v_ref=tr.v_ref[lo:hi], ds_next=tr.ds_next[lo:hi], ub=tr.ub_free[lo:hi, :N], lb=tr.lb_free[lo:hi, :N],
                x=tr.x[lo:hi], y=tr.y[lo:hi], psi=tr.psi[lo:hi], cum_lengths=cum[lo:hi] - cum[lo]) for _, lo, hi, _ in SPANS]
    cat, first = mpmpc.concat_routes(own)
    return own, cat, first, np.array([c for *_, c in SPANS], np.int32)


def _fleet(B, N, hand_over):
    """B cars on L / A / Bo (route = i % 3) on the first 15 waypoints of their routes, on a handle ready for rollout_init;
    hand_over: A's cars start on rows 100 .. 104 instead, which Bo shares - a re-route onto Bo accepts them"""
    import numpy as np
    import mpmpc
    import mpmpc_testlib as T
    own, cat, first, circ = _routes(N)
    h = mpmpc.Handle(T.stock_config(N, max_batch=B, circular=False), mpmpc.default_settings())
    h.set_path(cat["kappa"], cat["v_ref"], cat["ds_next"])
    h.set_corridor(cat["ub"], cat["lb"])
    h.set_routes(first, circ)
    n = int(first[-1])
    h.set_path_geometry(cat["x"], cat["y"], cat["psi"], np.zeros((n, 2)), np.zeros((n, 2)))
    route = (np.arange(B) % 3).astype(np.int32)
    rng = np.random.default_rng(4)
    wp = np.where((route == 1) & hand_over, rng.integers(100, 105, B), rng.integers(0, 15, B))
    s = np.array([own[p]["cum_lengths"][w] for p, w in zip(route, wp)])
    poses = np.array([[own[p]["x"][w], own[p]["y"][w], own[p]["psi"][w]] for p, w in zip(route, wp)])
    return h, own, cat, route, s, poses


def np_project(tab, poses, max_heading):
    """the numpy restatement of the law (tests/test_reroute.py), one route"""
    import numpy as np
    x, y, psi, cum = tab["x"], tab["y"], tab["psi"], tab["cum_lengths"]
    dx, dy = poses[:, 0:1] - x[None], poses[:, 1:2] - y[None]
    d2 = dx * dx + dy * dy
    t = np.fmod(poses[:, 2:3] - psi[None] + np.pi, 2 * np.pi)
    e = np.where(t < 0, t + 2 * np.pi, t) - np.pi
    ok = np.abs(e) <= max_heading
    wp = np.argmin(np.where(ok, d2, np.inf), 1)
    r = np.arange(poses.shape[0])
    return np.where(ok.any(1), wp, -1), np.sqrt(d2[r, wp]), cum[wp]


def reroute_cost(B, R=15, warm=3):
    """mpmpc_rollout_reroute (A's cars onto Bo, the rest kept) against the detour it removes: rollout_state, numpy projection,
    set_car_routes, rollout_init, rollout_set_counters - both from the same state after 3 steps, both timed to the device drained"""
    import numpy as np
    h, own, cat, route, s, poses = _fleet(B, 10, True)          # (N = 10: A's rows 100 .. 109 are before its end)
    ask = np.where(route == 1, 2, -1).astype(np.int32)
    t_call, t_detour, accepted = [], [], 0
    for k in range(warm + R):
        h.set_car_routes(route)
        h.rollout_init(0.05, cat["cum_lengths"], s, poses)
        h.rollout_step(3)
        h.rollout_state()
        t0 = time.perf_counter()
        acc = h.rollout_reroute(ask)          # (returns with the verdicts: the device is drained)
        t1 = time.perf_counter()
        accepted = int(acc.sum())
        h.set_car_routes(route)
        h.rollout_init(0.05, cat["cum_lengths"], s, poses)
        h.rollout_step(3)
        h.rollout_state()
        t2 = time.perf_counter()
        st = h.rollout_state()
        idx = np.flatnonzero((ask >= 0) & (st["alive"] == 1))
        wp, dist, s_new = np_project(own[2], st["pose"][idx], np.pi / 2)
        take = idx[wp >= 0]
        new_route, new_s = route.copy(), st["s"].copy()
        new_route[take], new_s[take] = 2, s_new[wp >= 0]
        h.set_car_routes(new_route)
        h.rollout_init(0.05, cat["cum_lengths"], new_s, st["pose"], st["cc"])
        h.rollout_set_counters(st["counter"])
        t3 = time.perf_counter()
        if k >= warm:
            t_call.append(1e3 * (t1 - t0))
            t_detour.append(1e3 * (t3 - t2))
    h.close()
    return dict(B=B, accepted=accepted, asked=int((ask >= 0).sum()), reroute_ms=statistics.median(t_call), reroute_min=min(t_call),
                reroute_max=max(t_call), detour_ms=statistics.median(t_detour), detour_min=min(t_detour), detour_max=max(t_detour),
                factor=statistics.median(t_detour) / statistics.median(t_call))


def project_cost(B=1024, P=64, R=15, warm=3):
    """1 024 poses x 64 routes (copies of the lap) in one mpmpc_project call (tables up, results back) against numpy route by route"""
    import numpy as np
    import mpmpc
    own, _, _, _ = _routes(30)
    lap = own[0]
    cat, first = mpmpc.concat_routes([lap] * P)
    rng = np.random.default_rng(2)
    w = rng.integers(0, 200, B)
    poses = np.stack([lap["x"][w] + rng.uniform(-0.1, 0.1, B), lap["y"][w] + rng.uniform(-0.1, 0.1, B), lap["psi"][w] + rng.uniform(-0.3, 0.3, B)], 1)
    t_dev, t_np = [], []
    for k in range(warm + R):
        t0 = time.perf_counter()
        out = mpmpc.project(cat["x"], cat["y"], cat["psi"], cat["cum_lengths"], poses, first=first, max_heading=np.pi / 2)
        t1 = time.perf_counter()
        ref = [np_project(lap, poses, np.pi / 2) for _ in range(P)]
        t2 = time.perf_counter()
        if k >= warm:
            t_dev.append(1e3 * (t1 - t0))
            t_np.append(1e3 * (t2 - t1))
    same = all(np.array_equal(out["wp"][:, p], ref[p][0]) and np.array_equal(out["dist"][:, p], ref[p][1]) for p in range(P))
    return dict(B=B, P=P, project_ms=statistics.median(t_dev), project_min=min(t_dev), project_max=max(t_dev), numpy_ms=statistics.median(t_np),
                numpy_min=min(t_np), numpy_max=max(t_np), factor=statistics.median(t_np) / statistics.median(t_dev), same=bool(same))


def k3_step_ms(B, n=40, R=5, warm=10):
    """a route-fleet rollout on L / A / Bo that never re-routes: rollout_step(n) then rollout_state, per step (uses nothing this
    feature adds, so that the parent's package runs it too)"""
    h, own, cat, route, s, poses = _fleet(B, 30, False)          # (50 steps from rows 0 .. 14: no open route ends)
    h.set_car_routes(route)
    out = []
    for _ in range(R):
        h.rollout_init(0.05, cat["cum_lengths"], s, poses)
        h.rollout_step(warm)
        h.rollout_state()
        t0 = time.perf_counter()
        h.rollout_step(n)
        st = h.rollout_state()
        out.append(1e3 * (time.perf_counter() - t0) / n)
    h.close()
    return statistics.median(out), float((st["alive"] == 1).mean())


def child(args):
    if args.pkg:          # another checkout's package: its mpmpc.py and the libmpmpc.so beside it (imported before anything else is)
        sys.path.insert(0, os.path.abspath(args.pkg))
    import mpmpc
    if args.child == "reroute":
        out = reroute_cost(args.n)
    elif args.child == "project":
        out = project_cost()
    else:
        out = dict(pkg=os.path.dirname(mpmpc.LIB_PATH), version=mpmpc.load_library().mpmpc_version().decode())
        for B in (1024, 8192):
            out["k3_ms_%d" % B], out["alive_%d" % B] = k3_step_ms(B)
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
    ap.add_argument("--reroute", action="store_true")
    ap.add_argument("--project", action="store_true")
    ap.add_argument("--parent-pkg")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--child")
    ap.add_argument("--pkg")
    ap.add_argument("--n", type=int, default=0)
    args = ap.parse_args()
    if args.child:
        return child(args)
    if args.reroute:
        for B in (1024, 8192):
            run_child("--child", "reroute", "--n", str(B))
    if args.project:
        run_child("--child", "project")
    if args.parent_pkg:
        rows = {"parent": [], "branch": []}
        for _ in range(args.rounds):
            rows["parent"].append(run_child("--child", "k3", "--pkg", args.parent_pkg))
            rows["branch"].append(run_child("--child", "k3"))
        for key in ("k3_ms_1024", "k3_ms_8192"):
            for who in ("parent", "branch"):
                v = [r[key] for r in rows[who]]
                print("%-12s %-7s median %.6g  min %.6g  max %.6g" % (key, who, statistics.median(v), min(v), max(v)), flush=True)


if __name__ == "__main__":
    main()
