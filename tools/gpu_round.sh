#!/bin/bash
# GPU-box evidence run: the whole -m gpu suite, smoke(), the driver's own bench
# command with every leg (--full), the 500-step headline with its roofline
# pass, a rocprofv3 kernel-trace --stats of the headline leg, and the stamp
# timelines.  Each GPU step has its own limit; any failure ends the session.
# Logs go under $OUT (default bench_out).
set -u
TAG=${TAG:-r05}
OUT=${OUT:-bench_out}
mkdir -p $OUT/$TAG
export PYTHONUNBUFFERED=1
timeout -k 10 900 python3 -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread -p no:cacheprovider > $OUT/$TAG/gpu_tests.log 2>&1
rc=$?; echo "pytest rc=$rc"; tail -3 $OUT/$TAG/gpu_tests.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python3 -c "import __graft_entry__ as g; g.smoke()" 2>&1 | grep -v amdgpu.ids; rc=${PIPESTATUS[0]}; [ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python3 bench.py --gpus 1 --steps 20 --warmup 5 --full > $OUT/$TAG/bench_driver.json 2> $OUT/$TAG/bench_driver.err; rc=$?; echo "driver-cmd bench rc=$rc"; [ $rc -eq 0 ] || exit $rc
python3 -c "import json;d=json.load(open('$OUT/$TAG/bench_driver.json'));print(round(d['value']/1e6,3),'M',round(d['ms_per_step']*1e3,2),'us/step',d['roofline']['kernel'],round(d['roofline']['frac'],3),d['roofline']['avg_kernel_us'])"
timeout -k 10 300 python3 bench.py --steps 500 --full --no-cpu-baseline --cache-steps -1 --converge-seconds 0 --config1-seconds -1 --config4-seconds -1 --config5-seconds -1 --drag-seconds -1 > $OUT/$TAG/bench_500.json 2>/dev/null; rc=$?; [ $rc -eq 0 ] || exit $rc
python3 -c "import json;d=json.load(open('$OUT/$TAG/bench_500.json'));print('500 steps:',round(d['value']/1e6,3),'M',round(d['ms_per_step']*1e3,2),'us/step',round(d['roofline']['frac'],3))"
cd /tmp && export TMPDIR=/tmp
R="$GRAFT_REPO_ROOT"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$R/$OUT/$TAG/prof" -o run \
  -- python3 "$R/bench.py" --full --no-cpu-baseline --cache-steps -1 --converge-seconds 0 --config1-seconds -1 --config4-seconds -1 --config5-seconds -1 --drag-seconds -1 \
  > "$R/$OUT/$TAG/prof.log" 2>&1
rc=$?; echo "prof rc=$rc"; rm -f "$R"/$OUT/$TAG/prof/*kernel_trace.csv; [ $rc -eq 0 ] || exit $rc
cd "$R"
STAMP_OUT=$PWD/tools/_stamped timeout -k 10 120 python3 tools/uni_stamps.py --no-build 2>&1 | grep -v amdgpu.ids > $OUT/$TAG/uni_stamps.txt; cat $OUT/$TAG/uni_stamps.txt
STAMP_OUT=$PWD/tools/_stamped timeout -k 10 120 python3 tools/mh_stamps.py --no-build 2>&1 | grep -v amdgpu.ids > $OUT/$TAG/mh_stamps.txt; cat $OUT/$TAG/mh_stamps.txt
