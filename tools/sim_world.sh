#!/bin/bash
# Rehearse, on ONE GPU, the per-rank compute of an N-way row partition (rank 0's block, no collective).
out=${1:?usage: tools/sim_world.sh <out dir>}
mkdir -p $out
for w in 2 4 8; do
  timeout -k 10 200 python bench.py --full --no-cpu-baseline --sim-world $w --steps 50 --warmup 10 > $out/sim_world_$w.json 2> $out/sim_world_$w.err
  python - "$w" "$out/sim_world_$w.json" <<'PY'
import json, sys
w = sys.argv[1]
d = json.load(open(sys.argv[2]))
print("sim-world", w, "ms_per_step", d["ms_per_step"], "plane_kernel_ms", d["roofline"]["kernel_ms_avg"],
      "frac", d["roofline"]["frac"], d["config"]["chunks"])
PY
done
