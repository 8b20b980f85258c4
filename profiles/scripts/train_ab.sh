#!/bin/bash
# A/B of the training step under the launch-structure switch SN_TRAIN_DEFER_DW (graphed ms per step + bit comparison); run on the GPU box from the repo root
out=gpurun_out/train_ab; mkdir -p $out
for dd in 0 1; do
  SN_TRAIN_DEFER_DW=$dd python profiles/scripts/train_ab_bits.py $out/bits_d${dd}.pt > $out/bits_d${dd}.log 2>&1
  SN_TRAIN_DEFER_DW=$dd python bench.py --workload train --steps 30 --warmup 10 --no-cpu-baseline > $out/train_d${dd}.json 2> $out/train_d${dd}.err
  python - <<P
import json
d=json.load(open("$out/train_d${dd}.json"))
print("defer_dw=$dd graphed ms", round(d["graphed"]["ms_per_step"],4), "eager", round(d["eager"]["ms_per_step"],3), "launches", d["launches_per_step"])
P
done
echo "== d0 vs d1"; python profiles/scripts/train_ab_bits.py --compare $out/bits_d0.pt $out/bits_d1.pt
rm -f $out/*.pt
