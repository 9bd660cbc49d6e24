"""Child process of tests/test_hw_queues.py: config 2 at B = 1 024 on a fresh HIP runtime whose GPU_MAX_HW_QUEUES the parent
chose (the runtime reads the variable at its first call, so it has to be in this process's environment from the start).

    python tests/hw_queue_child.py equal      depth-4 resident launches against depth 1, byte for byte
    python tests/hw_queue_child.py rate       depth 3 against depth 4: median rate of 200-step regions after bench.py's clock ramp

Prints one JSON line."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "multi-purpose-mpc_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import mpmpc  # noqa: E402
import mpmpc_testlib as T  # noqa: E402
import scenarios  # noqa: E402

B = 1024
FIELDS = ("z", "u0", "status", "iters", "resid")


def handle(tr, sc, want_y):
    h = mpmpc.Handle(T.stock_config(sc.N, sc.weights, max_batch=B), mpmpc.default_settings())
    h.set_path(tr.kappa, tr.v_ref, tr.ds_next)
    h.set_outputs(want_y)
    h.upload(sc.wp_id, sc.x0, sc.cc_prev, sc.lb, sc.ub)
    return h


def equal(tr, sc):
    h = handle(tr, sc, True)
    got = {}
    for depth in (1, 4):
        h.set_pipeline(depth)
        for _ in range(9):          # the slots rotated more than twice
            h.solve_resident(B)
        got[depth] = h.download(B, want_y=True)
    h.close()
    same = {k: bool(np.array_equal(getattr(got[1], k), getattr(got[4], k)) and
                    getattr(got[1], k).tobytes() == getattr(got[4], k).tobytes()) for k in FIELDS + ("y",)}
    return {"same": same, "solved": int(np.sum(got[4].status == 1)), "instances": B}


def ramp(h):
    """bench.py's clock ramp: 300 launches, then groups of >= 10 ms until a group is no faster than the best before it (3 %)
    twice in a row, at most 3 s"""
    for _ in range(300):
        h.solve_resident(B)
    h.sync()
    t_end, g, best, calm = time.perf_counter() + 3.0, 50, None, 0
    while time.perf_counter() < t_end and calm < 2:
        t0 = time.perf_counter()
        for _ in range(g):
            h.solve_resident(B)
        h.sync()
        dt = time.perf_counter() - t0
        if dt < 0.010:
            g = min(5000, int(g * max(2.0, 0.012 / max(dt, 1e-6))))
            continue
        calm = calm + 1 if (best is not None and dt / g > 0.97 * best) else 0
        best = dt / g if best is None else min(best, dt / g)


def rate(tr, sc, regions=9, steps=200):
    h = handle(tr, sc, False)
    h.set_pipeline(4)
    ramp(h)
    rates = {3: [], 4: []}
    for _ in range(regions):          # the two depths in turn: a drift of the clocks meets both alike
        for depth in (3, 4):
            h.set_pipeline(depth)
            for _ in range(10):
                h.solve_resident(B)
            h.sync()
            t0 = time.perf_counter()
            for _ in range(steps):
                h.solve_resident(B)
            h.sync()
            rates[depth].append(B * steps / (time.perf_counter() - t0))
    h.close()
    med = {d: float(np.median(v)) for d, v in rates.items()}
    return {"solves_per_s_depth3": med[3], "solves_per_s_depth4": med[4], "ratio_depth4_over_depth3": med[4] / med[3],
            "regions": {str(d): v for d, v in rates.items()}, "steps_per_region": steps}


if __name__ == "__main__":
    tr = scenarios.sim_track()
    sc = scenarios.make(2, tr, B=B)
    out = (equal if sys.argv[1] == "equal" else rate)(tr, sc)
    out["GPU_MAX_HW_QUEUES"] = os.environ.get("GPU_MAX_HW_QUEUES")
    out["streams_at_depth4"] = int(mpmpc.load_library().mpmpc_pipeline_streams(4, mpmpc.load_library().mpmpc_hw_queue_budget(
        os.environ["GPU_MAX_HW_QUEUES"].encode() if "GPU_MAX_HW_QUEUES" in os.environ else None)))
    print(json.dumps(out))
