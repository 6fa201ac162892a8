#!/bin/bash
# round artefacts, call C: the default bench line (now with roofline.traffic from the committed PMC pass), the C2 line, the other configurations
cd ${GRAFT_REPO_ROOT:-$(pwd)}
OUT=${JV_OUT:-out}/final
mkdir -p $OUT
python bench.py --full > $OUT/bench2.json 2> $OUT/bench2.err || { tail -n 5 $OUT/bench2.err; exit 1; }
python bench.py --full --workload c2 --batch 8 --tokens 256 --no-exact-range > $OUT/bench_c2.json 2> $OUT/bench_c2.err || { tail -n 5 $OUT/bench_c2.err; exit 1; }
python tools/bench_configs.py r04
