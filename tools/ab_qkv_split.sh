#!/bin/bash
# same-box A/B of the mid-batch q|k|v column split and the norm1 fold (from the repo root):
#   bash tools/ab_qkv_split.sh      -> $JV_OUT/ab_*.json, $JV_OUT/t1.log  (JV_OUT defaults to out/)
set -e
cd ${GRAFT_REPO_ROOT:-$(pwd)}
OUT=${JV_OUT:-out}
mkdir -p $OUT
B="--no-cpu-baseline --no-exact-range --no-profile"
python -m pytest tests/test_gpu_pipeline.py tests/test_gpu_regimes.py tests/test_gpu_dist.py -q -x -k "split_qkv or fused_block or ln_fold or regime or dist" > $OUT/t1.log 2>&1
for b in 8 4 6 10 12; do
  python bench.py --batch $b $B > $OUT/ab_b${b}_new.json 2> $OUT/err.log
  JV_NO_QKV_SPLIT=1 JV_NO_LN_FOLD=1 python bench.py --batch $b $B > $OUT/ab_b${b}_old.json 2> $OUT/err.log
done
python bench.py --batch 8 --full --no-cpu-baseline --no-exact-range > $OUT/ab_b8_prof.json 2> $OUT/err.log
