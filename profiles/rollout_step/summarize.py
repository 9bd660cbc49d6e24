"""The pairs (parent / this tree on the same world) of profiles/traffic_lookahead/measure.py --parent-lib: is this tree's median ms
per step above the parent's by more than the parent's own round-to-round spread (max - min)?

    python profiles/rollout_step/summarize.py cost.jsonl [cost_parent_first.jsonl ...]
"""
import json
import statistics as S
import sys

PAIRS = (("parent_traffic", "traffic"), ("parent_look", "look_off"))


def main():
    bad = 0
    for path in sys.argv[1:]:
        rows = [json.loads(l) for l in open(path) if l.startswith("{")]
        same = all(r["same_as_first"] for r in rows if "case" in r)
        for B in (1024, 8192):
            for old, new in PAIRS:
                a = [r["ms_per_step"] for r in rows if r.get("B") == B and r.get("case") == old]
                b = [r["ms_per_step"] for r in rows if r.get("B") == B and r.get("case") == new]
                ok = S.median(b) <= S.median(a) + (max(a) - min(a))
                bad += not ok
                print("%s B %5d %-14s %.4f (%.4f .. %.4f)  %-9s %.4f (%.4f .. %.4f)  %+.2f %% against a spread of %.2f %%: %s" %
                      (path.split("/")[-1], B, old, S.median(a), min(a), max(a), new, S.median(b), min(b), max(b),
                       100 * (S.median(b) / S.median(a) - 1), 100 * (max(a) - min(a)) / S.median(a), "inside" if ok else "ABOVE"))
        print("%s: final state equals the first case's in every case: %s" % (path.split("/")[-1], same))
        bad += not same
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
