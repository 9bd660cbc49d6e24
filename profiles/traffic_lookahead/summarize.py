"""Tables of profiles/traffic_lookahead/README.md from measure.py's lines and a kernel trace of `measure.py --quick --no-effect`.

    python profiles/traffic_lookahead/summarize.py cost.jsonl [trace_kernel_trace.csv]
"""
import csv
import json
import statistics as S
import sys

CASES = ("parent_traffic", "traffic", "parent_look", "look_off", "look_on", "traffic_look_on")
KERNELS = ("corridor_kernel", "traffic_kernel", "traffic_horizon", "plan_track", "mover_horizon")


def main():
    rows = [json.loads(l) for l in open(sys.argv[1]) if l.startswith("{")]
    print(rows[0])
    for B in (1024, 8192):
        for case in CASES:
            mine = [r for r in rows if r.get("B") == B and r.get("case") == case]
            v = [r["ms_per_step"] for r in mine]
            if v:
                print("B %5d %-16s median %.4f (%.4f .. %.4f) ms per step, spread %.1f %%; running %d, blocked %d, same %s" %
                      (B, case, S.median(v), min(v), max(v), 100 * (max(v) - min(v)) / S.median(v), mine[-1]["running"], mine[-1]["blocked"],
                       all(r["same_as_first"] for r in mine)))
    for r in rows:
        if r.get("effect"):
            print(r)
    if len(sys.argv) > 2:
        by = {}
        for r in csv.DictReader(open(sys.argv[2])):
            name = r["Kernel_Name"].split("(")[0].replace("void ", "")
            if any(k in name for k in KERNELS):
                blocks = int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"])
                if name.endswith("<false, true, true>"):      # (--quick without a parent: 13 launches per case and round, look_on then traffic_look_on)
                    seen = len(by.get((name + " look_on", blocks), [])) + len(by.get((name + " traffic_look_on", blocks), []))
                    name += " look_on" if (seen // 13) % 2 == 0 else " traffic_look_on"
                by.setdefault((name, blocks), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
        for (name, blocks), v in sorted(by.items()):
            print("%-60s blocks %5d launches %3d median %6.1f (%.1f .. %.1f) us" % (name, blocks, len(v), S.median(v), min(v), max(v)))


if __name__ == "__main__":
    main()
