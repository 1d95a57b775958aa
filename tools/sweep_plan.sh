#!/bin/bash
# sweep of the item lengths (L1, L2) of the level machinery on one box: bench.py --msm-plan 0,L1,L2,0,0
O=${LOG_DIR:-$(mktemp -d)}   # the bench logs (LOG_DIR, or a fresh temporary directory)
for plan in "$@"; do
  timeout -k 10 200 python bench.py --full --no-cpu-baseline --sharded-msm-log-n 0 --steps 20 --msm-plan $plan > $O/sweep_$plan.log 2>&1 || exit 1
  python - <<PY
import json
l = json.loads(open("$O/sweep_$plan.log").read().strip().splitlines()[-1])
print("plan $plan", "proofs/s %.2f" % l["value"], "latency %.2f" % l["single_proof_latency_ms"], "accum launch %.3f" % l["roofline"]["launch_ms"], flush=True)
PY
done
