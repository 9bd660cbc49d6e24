"""What building reference paths on the device (K0p) costs, against the host constructor.

    python profiles/path_build/path_cost.py [--quick]

Real_Track's grid (867 x 767 cells of 0.06 m) and route (4 corners, path resolution 0.2 m, smoothing 5, max_width 1.5 m, open:
302 waypoints), the corners of every route jittered by up to 0.4 m from one seed.  Cases, run in turn `rounds` times in one
process, one JSON line per case and round:
  build P        mpmpc.path_build of P = 1 / 64 / 1 024 routes: `calls` timed calls after `warm` of warm-up.  call_ms = host
                 clock around the whole call (it ends in a stream synchronise); host_ms / walls_ms / kernel_ms = the call's own
                 split (mpmpc_path_build_timed: steps 1 - 4 by the host clock, K0w and K0p between device events), medians
  build_walls P  the same with two walls per route, so that K0w has work
  host           ReferencePath(...) of ONE route on this machine's host: the baseline, s per path
Each build also reports that the device's ub / lb / border cells of route 0 equal the host constructor's."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in ("multi-purpose-mpc_amd", "tests", "oracle", ""):
    sys.path.insert(0, os.path.join(ROOT, p))

import numpy as np  # noqa: E402

import mpmpc  # noqa: E402
from map import Map  # noqa: E402
from reference_path import ReferencePath  # noqa: E402

R_P, SD, MW = 0.2, 5, 1.5


def main():
    quick = "--quick" in sys.argv
    g1 = np.load(os.path.join(ROOT, "tests", "golden", "g1_path_real_track.npz"))
    h_, w_ = g1["grid_shape"]
    grid = np.ascontiguousarray(np.unpackbits(g1["grid_free"])[:h_ * w_].reshape(h_, w_).astype(np.int8))
    origin, res = tuple(float(v) for v in g1["origin"]), float(g1["resolution"][0])
    base = np.stack([g1["wp_x"], g1["wp_y"]], 1)
    rng = np.random.default_rng(7)
    routes = [base] + [base + rng.uniform(-0.4, 0.4, base.shape) for _ in range(1023)]
    m = Map.from_grid(grid, origin=list(origin), resolution=res)
    wall = m.boundary_walls([((-20.0, -20.0), (-15.0, -18.0)), ((15.0, 15.0), (18.0, 12.0))])
    rounds, warm, calls = (1, 1, 3) if quick else (3, 3, 20)
    print(json.dumps(dict(case="setup", version=mpmpc.load_library().mpmpc_version().decode(), rounds=rounds, warm=warm, calls=calls)), flush=True)
    t0 = time.perf_counter()
    host = ReferencePath(m, list(base[:, 0]), list(base[:, 1]), R_P, SD, MW, False)
    host_s = time.perf_counter() - t0
    ub = np.array([w.ub for w in host.waypoints])
    lb = np.array([w.lb for w in host.waypoints])
    cells = np.array([[w.static_border_cells[0], w.static_border_cells[1]] for w in host.waypoints]).reshape(-1, 4)
    print(json.dumps(dict(case="host", round=0, s_per_path=host_s, n_wp=host.n_waypoints)), flush=True)
    for rnd in range(rounds):
        for P in (1, 64, 1024):
            for walls in (False, True):
                kw = dict(walls=[wall] * P) if walls else {}
                ms, wall_clock = [], []
                for c in range(warm + calls):
                    split = []
                    t0 = time.perf_counter()
                    rec = mpmpc.path_build(grid, origin, res, routes[:P], R_P, SD, MW, circular=False, timings=split, **kw)
                    dt = time.perf_counter() - t0
                    if c >= warm:
                        ms.append(split)
                        wall_clock.append(1e3 * dt)
                r0 = rec[0]
                same = bool(np.array_equal(r0["ub"], ub) and np.array_equal(r0["lb"], lb) and
                            np.array_equal(np.hstack([r0["border_ub"], r0["border_lb"]]), cells))
                med = np.median(np.array(ms), 0)
                print(json.dumps(dict(case="build_walls" if walls else "build", round=rnd, P=P, waypoints=int(sum(r["n_wp"] for r in rec)),
                                      call_ms=float(np.median(wall_clock)), call_ms_min=float(np.min(wall_clock)),
                                      call_ms_max=float(np.max(wall_clock)), host_ms=float(med[0]), walls_ms=float(med[1]),
                                      kernel_ms=float(med[2]), kernel_ms_min=float(np.min(np.array(ms)[:, 2])),
                                      kernel_ms_max=float(np.max(np.array(ms)[:, 2])), statuses=sorted(set(r["status"] for r in rec)),
                                      route0_equals_host=same)), flush=True)
        if rnd + 1 < rounds:
            t0 = time.perf_counter()
            ReferencePath(m, list(base[:, 0]), list(base[:, 1]), R_P, SD, MW, False)
            print(json.dumps(dict(case="host", round=rnd + 1, s_per_path=time.perf_counter() - t0, n_wp=host.n_waypoints)), flush=True)


if __name__ == "__main__":
    main()
