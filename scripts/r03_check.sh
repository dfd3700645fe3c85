#!/bin/bash
# usage (GPU box): bash scripts/r03_check.sh <tag>  -- whole GPU suite, then a short bench line
TAG=${1:-t}
python -m pytest tests -m gpu -x -q > gpurun_out/r03_${TAG}_tests.log 2>&1
echo "pytest rc=$?"; tail -15 gpurun_out/r03_${TAG}_tests.log
python bench.py --full --no-cpu-baseline --no-forward --no-per-layer 2>/dev/null | python -c "import json,sys; d=json.loads(sys.stdin.read()); print('ms_per_step', d['ms_per_step'], d.get('filter'))"
