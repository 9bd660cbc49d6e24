#!/bin/bash
# quick GPU check used while tuning: parity tests, then the single-GPU configurations and the large batch
#   /usr/local/graft/bin/gpurun --timeout 1500 -- 'bash profiles/quick.sh tag'
T=${1:-q}
OUT=${OUT:-profiles/out}          # results directory
export OUT
mkdir -p $OUT
timeout 1200 python -m pytest tests -m gpu -x -q 2>&1 | tail -15 | tee $OUT/${T}_pytest.log
for c in 2 3 4 5; do python bench.py --full --config $c --steps 10 --warmup 2 > $OUT/${T}_$c.json 2> $OUT/${T}_$c.err || tail -5 $OUT/${T}_$c.err; done
python bench.py --full --no-cpu --batch 65536 --steps 5 --warmup 1 > $OUT/${T}_big.json 2>/dev/null
python - "$T" <<'PY'
import json, os, sys
for c in ("2", "3", "4", "5", "big"):
    try:
        d = json.load(open(os.path.join(os.environ["OUT"], "%s_%s.json" % (sys.argv[1], c))))
    except Exception as e:
        print(c, "no line:", e)
        continue
    print(c, round(d["value"]), round(d["ms_per_step"], 4), round(d["roofline"]["avg_ms"], 4), d["iters"], d["status_counts"],
          d.get("max_abs_u_minus_uref"), d.get("status_agreement"))
PY
