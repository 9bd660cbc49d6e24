"""The fixed cost of an entry point without a handle: warm-call wall time of mpmpc_speed_profile and mpmpc_lidar_scan, this tree's
library against another checkout's (profiles/one_shot/README.md).

    python profiles/one_shot/measure.py --parent-pkg OTHER/multi-purpose-mpc_amd [--rounds 5]

Every figure comes from a child process of its own (a fresh HIP context per library); the other checkout's package (its mpmpc.py
and the libmpmpc.so beside it) and this tree's alternate, `--rounds` children each.  A child calls each entry point 20 times to
warm up (the first call allocates the scratch and creates its stream), then 200 times inside a host clock per call, and prints
the medians as one JSON line.  speed profile: B = 1, n = 256 (the `iid` family of tests/speed_profile_cases.py; the wave kernel).
lidar: B = 16 cars on waypoints of the Sim_Track lap, 64 beams over 180 degrees, 3 m range, no discs."""
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
WARM, CALLS = 20, 200


def _median_us(call):
    for _ in range(WARM):
        call()
    ts = []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        call()
        ts.append(1e6 * (time.perf_counter() - t0))
    return statistics.median(ts)


def child(args):
    if args.pkg:          # another checkout's package, imported before anything else is
        sys.path.insert(0, os.path.abspath(args.pkg))
    import numpy as np
    import mpmpc
    import mpmpc_testlib as T
    import speed_profile_cases as S
    li, kappa, lim = S.make("iid", 256)
    g1, grid, origin, res = T.g1_world("sim")
    wp = np.arange(16) * (g1["x"].size // 16)
    poses = np.ascontiguousarray(np.stack([g1["x"][wp], g1["y"][wp], g1["psi"][wp]], 1))
    angles = np.linspace(-np.pi / 2, np.pi / 2, 64)
    out = dict(pkg=os.path.dirname(mpmpc.LIB_PATH), version=mpmpc.load_library().mpmpc_version().decode())
    out["speed_profile_us"] = _median_us(lambda: mpmpc.speed_profile(li, kappa, lim))
    out["lidar_scan_us"] = _median_us(lambda: mpmpc.lidar_scan(grid, origin, res, poses, angles, 3.0))
    v, status, _ = mpmpc.speed_profile(li, kappa, lim)
    out["solved"] = bool(status[0] == 1)
    out["hits"] = int((mpmpc.lidar_scan(grid, origin, res, poses, angles, 3.0) < 3.0).sum())
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
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--pkg")
    args = ap.parse_args()
    if args.child:
        return child(args)
    rows = {"parent": [], "branch": []}
    for r in range(args.rounds):
        for who in (("parent", "branch") if r % 2 == 0 else ("branch", "parent")):      # (who goes first alternates too)
            if who == "branch":
                rows[who].append(run_child("--child"))
            elif args.parent_pkg:
                rows[who].append(run_child("--child", "--pkg", args.parent_pkg))
    for key in ("speed_profile_us", "lidar_scan_us"):
        for who in ("parent", "branch"):
            v = [r[key] for r in rows[who]]
            if v:
                print("%-17s %-7s median %.2f  min %.2f  max %.2f" % (key, who, statistics.median(v), min(v), max(v)), flush=True)


if __name__ == "__main__":
    main()
