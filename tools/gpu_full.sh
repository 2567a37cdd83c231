#!/bin/bash
# The GPU suite and the whole benchmark (bench.py --full): tools/gpu_full.sh <output dir>
set -u
OUT=${1:?usage: tools/gpu_full.sh <output dir>}
mkdir -p $OUT
timeout 2400 python -m pytest tests -x -q -m gpu > $OUT/pytest.log 2>&1
echo "pytest rc=$?" > $OUT/rc.txt
timeout 900 python bench.py --full > $OUT/bench.json 2> $OUT/bench.err
echo "bench rc=$?" >> $OUT/rc.txt
cat $OUT/rc.txt; tail -n 5 $OUT/pytest.log; cut -c1-600 $OUT/bench.json; tail -n 3 $OUT/bench.err
