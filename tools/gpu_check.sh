#!/bin/bash
# usage: tools/gpu_check.sh <tag> [pytest-args]   -- run GPU parity tests + rocprof'd bench on the GPU box
TAG=${1:-x}
cd /tmp && export TMPDIR=/tmp; cd $GRAFT_REPO_ROOT
python -m pytest tests -x -q -m gpu 2>&1 | tail -6
O=${CPM_CHECK_OUT:-out}   # where the kernel trace and the bench log go
rm -rf $O/prof_$TAG; mkdir -p $O
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_$TAG -- python3 bench.py --steps 50 --warmup 5 --no-cpu-baseline --full > $O/bench_$TAG.log 2>&1
grep '"metric"' $O/bench_$TAG.log | python3 -c "import sys,json; d=json.loads(sys.stdin.read()); print('value',d['value'],'ms',d['ms_per_step']); print(d['frame']['stage_ms'])" || tail -20 $O/bench_$TAG.log
python3 tools/kstats.py $O/prof_$TAG | head -14
