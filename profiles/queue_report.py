"""Which hardware queue each launch stream of a traced bench run sat on, and how many solve kernels were on the chip.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python bench.py --full --no-extra-legs --no-cpu > DIR.json
    python profiles/queue_report.py DIR DIR.json [OUT.json]

Reads the kernel trace rows (Queue_Id, Stream_Id, start / end time stamps) of the TIMED launches - the window that
profiles/summarize.py uses: the first kernels of the steps in start order, without the ramp and the warm-up - and prints /
writes: per stream the queue ids of its solve dispatches, the streams that share a queue, `solve_kernels_in_flight_avg` over
the window, the mean kernel duration, and the bench line's own `value`, library and GPU_MAX_HW_QUEUES as the run recorded them."""
import collections
import csv
import glob
import json
import os
import sys


def report(trace_dir, line):
    f = max(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True), key=os.path.getmtime)
    rows = [r for r in csv.DictReader(open(f)) if "mpmpc_reduced" in r["Kernel_Name"] or "mpmpc_solve_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    first = [r for r in rows if "mpmpc_reduced_kernel" in r["Kernel_Name"] or "mpmpc_reduced_t_kernel" in r["Kernel_Name"]] or rows
    n = int(line["steps"]) * int(line.get("repeats", 1))
    skip = int(line.get("prewarm", 300)) + int(line["warmup"])
    if int(line.get("repeats", 1)) > 1 and len(first) >= skip + int(line["steps"]) + n:
        skip += int(line["steps"])          # (--full runs a pilot region of K steps before the repeats)
    win = first[skip:skip + n]
    if len(win) < n:
        raise SystemExit("trace too short: %d launches after %d skipped, %d expected" % (len(win), skip, n))
    t0, t1 = int(win[0]["Start_Timestamp"]), max(int(r["End_Timestamp"]) for r in win)
    inside = [r for r in rows if t0 <= int(r["Start_Timestamp"]) <= t1]
    busy = sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in inside)
    queues = collections.defaultdict(collections.Counter)
    for r in inside:
        queues[r["Stream_Id"]][r["Queue_Id"]] += 1
    by_queue = collections.defaultdict(list)
    for s, c in queues.items():
        for q in c:
            by_queue[q].append(s)
    # every kernel dispatch of the process, solve or not, by queue: who else holds one
    others = collections.defaultdict(collections.Counter)
    for r in csv.DictReader(open(f)):
        others[r["Queue_Id"]][r["Kernel_Name"].split("(")[0].replace("void ", "")[:60]] += 1
    return {"library": line.get("library"), "value": line.get("value"), "ms_per_step_reported": line.get("ms_per_step"),
            "launches_in_flight_asked": line.get("launches_in_flight"), "steps": int(line["steps"]), "repeats": int(line.get("repeats", 1)),
            "timed_launches": n, "solve_kernels_in_flight_avg": busy / float(t1 - t0),
            "kernel_avg_us": busy * 1e-3 / max(1, len(inside)), "ms_per_step_in_trace": (t1 - t0) * 1e-6 / n,
            "queue_ids_by_stream": {s: dict(c) for s, c in sorted(queues.items())},
            "streams_by_queue": {q: sorted(v) for q, v in sorted(by_queue.items())},
            "launch_streams": len(queues), "distinct_queues": len(by_queue),
            "streams_sharing_a_queue": sorted(s for v in by_queue.values() if len(v) > 1 for s in v),
            "all_kernel_dispatches_by_queue": {q: dict(c) for q, c in sorted(others.items())}}


if __name__ == "__main__":
    line = json.loads(open(sys.argv[2]).read().strip().splitlines()[-1])
    out = report(sys.argv[1], line)
    text = json.dumps(out, indent=1)
    if len(sys.argv) > 3:
        open(sys.argv[3], "w").write(text + "\n")
    print(text)
