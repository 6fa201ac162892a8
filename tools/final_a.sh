#!/bin/bash
# round artefacts, call A: the whole GPU suite on the final build, then the headline bench line
cd ${GRAFT_REPO_ROOT:-$(pwd)}
OUT=${JV_OUT:-out}/final
mkdir -p $OUT
(time timeout -k 10 1000 python -m pytest tests -m gpu -x -q) > $OUT/gputests.log 2>&1 || { tail -n 40 $OUT/gputests.log; exit 1; }
tail -n 5 $OUT/gputests.log
python bench.py --full > $OUT/bench.json 2> $OUT/bench.err || { tail -n 5 $OUT/bench.err; exit 1; }
tail -c 1500 $OUT/bench.json
