#!/bin/bash
# tools/env_bench.sh "NAME=VAL ..." ... -- bench.py --full under different engine env knobs; one JSON line per
# setting under $OUT/envb (OUT: the output directory)
out=${OUT:?set OUT to the output directory}/envb; mkdir -p "$out"
i=0
for envs in "$@"; do
  i=$((i+1))
  env $envs python bench.py --steps 20 --warmup 3 --full --no-cpu-baseline --no-ablation $BENCH_ARGS 2>/dev/null > "$out"/$i.json
  python - "$envs" "$out"/$i.json <<'PY'
import json, sys
d = json.load(open(sys.argv[2]))
print(f"{sys.argv[1]:40s} ms/step {d['ms_per_step']:.4f}  frac {d['roofline']['frac']:.4f}  bad {d['parity']['mismatches_rel_1e-5']} upload {d['upload_seconds']}")
PY
done
