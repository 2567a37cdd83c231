#!/bin/bash
# The GPU suite, then bench.py --full and a few of its figures: tools/gpu_suite_and_bench.sh <output dir>
OUT=${1:?usage: tools/gpu_suite_and_bench.sh <output dir>}
mkdir -p $OUT
timeout 2400 python -m pytest tests -x -q -m gpu > $OUT/pytest.log 2>&1; echo "pytest rc=$?"; tail -n 4 $OUT/pytest.log
python bench.py --full > $OUT/bench.json 2> $OUT/bench.err; echo "bench rc=$?"
python - $OUT/bench.json <<'PY'
import json, sys
d=json.load(open(sys.argv[1]))
print(d['ms_per_step'], d['ms_per_step_same_topology'], d['value'], d['roofline']['frac'], d['roofline']['kernel_ms_per_launch'])
print(d['bootstrap_wall_clock']['seconds'], d['bootstrap_wall_clock']['refinement_s'], d['ufboot_online']['seconds_each_pass'])
print({k: (v if not isinstance(v, dict) else {a: b for a, b in v.items() if a != 'cpu_baseline'}) for k, v in d['random_start'].items()})
PY
