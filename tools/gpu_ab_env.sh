#!/bin/bash
# GPU box: the headline (quick form) under environment settings, alternating.  usage: tools/gpu_ab_env.sh TAG "ENV1" "ENV2" [rounds]
export TMPDIR=/tmp; cd "$(dirname "$0")/.."; out=${PTTS_OUT_DIR:-out}; mkdir -p "$out"
tag=$1; e1=$2; e2=$3; n=${4:-2}
for r in $(seq 1 $n); do
  for e in "$e1" "$e2"; do
    env $e timeout -k 10 300 python3 bench.py --full --no-cpu-baseline --no-b1 --no-traffic --no-two-engines --steps 8 > $out/${tag}_ab.json 2> $out/${tag}_ab.err || { echo "$e failed"; tail -3 $out/${tag}_ab.err; exit 1; }
    python3 -c "import json;d=json.load(open('$out/${tag}_ab.json'));r=d['roofline'];print('$e', d['value'],d['ms_per_step'],r['avg_launch_us'],r.get('phases_ms'))" | tee -a $out/${tag}_ab.txt
  done
done
