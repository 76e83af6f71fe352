#!/bin/bash
# GPU box: the headline with k_gemm4 off / persistent / two-stage (PTTS_GEMM4 = 0 / 1 / 2), phases
cd "$(dirname "$0")/../../.."; out=${PTTS_OUT_DIR:-out}; mkdir -p "$out"
tag=${1:-r2g4}
for v in 0 1 2 0 1 2; do
  PTTS_GEMM4=$v timeout -k 10 300 python3 bench.py --full --no-cpu-baseline --no-b1 --no-traffic --no-two-engines --steps 8 > $out/${tag}_bench_$v.json 2> $out/${tag}_bench_$v.err || { echo "bench $v failed"; tail -5 $out/${tag}_bench_$v.err; exit 1; }
  python3 -c "import json;d=json.load(open('$out/${tag}_bench_$v.json'));print('PTTS_GEMM4=$v', d['value'],d['ms_per_step'],d['roofline']['phases_ms'])" | tee -a $out/${tag}_summary.txt
done
