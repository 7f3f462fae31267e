#!/bin/bash
# Run on the GPU box (via gpurun): parity tests, bench, rocprofv3 kernel stats.  usage: tools/gpu_check.sh TAG [pytest-args]
# Logs and profiles go to $GT_OUT (default: out/ in the repository).
TAG=${1:-run}; shift
R=${GRAFT_REPO_ROOT:-$(pwd)}
O=${GT_OUT:-$R/out}
mkdir -p $O
cd $R
timeout 900 python -m pytest tests -q -m gpu --timeout 600 "$@" > $O/pytest_$TAG.log 2>&1; echo "pytest_exit=$?" >> $O/pytest_$TAG.log
tail -4 $O/pytest_$TAG.log
timeout 300 python bench.py --full --steps 300 --warmup 30 --no-cpu-baseline > $O/bench_$TAG.log 2>&1
tail -1 $O/bench_$TAG.log | python -c "import sys,json; d=json.loads(sys.stdin.read()); print('seq/s', d['value'], 'ms/step', d['ms_per_step'], 'dom', d['roofline']['kernel'], d['roofline']['achieved'], d['kernel_classes_us_per_step'])" || tail -5 $O/bench_$TAG.log
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_$TAG -- python3 $R/bench.py --full --steps 100 --warmup 10 --no-cpu-baseline > $O/benchprof_$TAG.log 2>&1
cd $R
python tools/kstats.py $(find $O/prof_$TAG -name "*kernel_stats.csv" | head -1) 131 | head -40
