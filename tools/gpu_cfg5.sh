#!/bin/bash
set -o pipefail
O=${OUT:-bench_out}; mkdir -p $O
python bench.py --full --n-public 1024 --batch-log2 12 --steps 5 --warmup 1 > $O/bench_cfg5.json 2> $O/bench_cfg5.err || { tail -20 $O/bench_cfg5.err; exit 1; }
python - $O/bench_cfg5.json <<'PY'
import json, sys
d=json.load(open(sys.argv[1]))
print("cfg5 value %.0f proofs/s  %.2f ms/step" % (d['value'], d['ms_per_step'])); print(d['roofline']); print(d['cpu_baseline'])
for k,v in list(d['kernels_ms'].items())[:6]: print("  %-22s %4d  %8.3f ms" % (k, v['launches'], v['total_ms']))
PY
bash tools/gpu_quick.sh
