#!/bin/bash
# round artefacts, call E (after profiles/ holds this build's PMC pass): the driver's command, the C2 line, the regime sweep
cd ${GRAFT_REPO_ROOT:-$(pwd)}
OUT=${JV_OUT:-out}/final
mkdir -p $OUT
python bench.py --full > $OUT/bench2.json 2> $OUT/bench2.err || { tail -n 5 $OUT/bench2.err; exit 1; }
python bench.py --full --workload c2 --batch 8 --tokens 256 --no-exact-range > $OUT/bench_c2.json 2> $OUT/bench_c2.err || { tail -n 5 $OUT/bench_c2.err; exit 1; }
python tools/regime_sweep.py --timesteps 4 --batches 1,2,4,6,8,12,16,24,32,48,64 > $OUT/regime_sweep.txt 2> $OUT/regime_sweep.err || tail -n 5 $OUT/regime_sweep.err
tail -n 16 $OUT/regime_sweep.txt
