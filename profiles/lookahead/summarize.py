"""Tables of profiles/lookahead/README.md from measure.py's lines and a kernel trace of it.

    python profiles/lookahead/summarize.py lookahead_cost.jsonl [trace_kernel_trace.csv]
"""
import csv
import json
import statistics as S
import sys


def main():
    rows = [json.loads(l) for l in open(sys.argv[1]) if l.startswith("{")]
    print(rows[0])
    for B in (1024, 8192):
        for case in ("parent_static", "static", "movers_off", "movers_on"):
            v = [r["ms_per_step"] for r in rows if r.get("B") == B and r.get("case") == case]
            if v:
                last = [r for r in rows if r.get("B") == B and r.get("case") == case][-1]
                print("B %5d %-14s median %.4f (%.4f .. %.4f) ms per step, spread %.1f %%; running %d, blocked %d, same %s" %
                      (B, case, S.median(v), min(v), max(v), 100 * (max(v) - min(v)) / S.median(v), last["running"], last["blocked"],
                       all(r["same_as_first"] for r in rows if r.get("B") == B and r.get("case") == case)))
    for r in rows:
        if r.get("effect"):
            print(r)
    if len(sys.argv) > 2:
        by = {}
        for r in csv.DictReader(open(sys.argv[2])):
            name = r["Kernel_Name"].split("(")[0].replace("void ", "")
            if "corridor_kernel" in name or "horizon" in name or "obstacle_move" in name:
                blocks = int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"])
                if name.endswith("<false, false>"):      # (--quick: 13 launches per case and round, static then movers_off)
                    seen = len(by.get((name + " static", blocks), [])) + len(by.get((name + " movers_off", blocks), []))
                    name += " static" if (seen // 13) % 2 == 0 else " movers_off"
                by.setdefault((name, blocks), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
        for (name, blocks), v in sorted(by.items()):
            print("%-45s blocks %5d launches %3d median %6.1f (%.1f .. %.1f) us" % (name, blocks, len(v), S.median(v), min(v), max(v)))


if __name__ == "__main__":
    main()
