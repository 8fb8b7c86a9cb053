#!/bin/bash
# The int8 prefilter's sample bound taken from the int8 copy (option i8_sample_scan) against the exact f32 pre-scan of a strided row sample, on ONE box in
# one go:
#   1. the headline command, alternating QMX_I8_SAMPLE_SCAN=0 / 1 (five of each; the first of each also dumps its last step's lists, which must be equal)
#   2. the same command on another build of the library, twice (give the parent commit's library: option 0 is supposed to be it)
#   3. one kernel trace of the other library and one of this one, in runs of their own (tools/scan_overlap.py, tools/i8_launch_split.py)
#   4. one --full run: the timed path against the exact scan
#   5. one kernel trace of this library at --dim 1024 (where the sample kernel keeps 16 queries per block)
#   6. the size of the sample: QMX_I8_SAMPLE_ROWS = 8192 / 16384 / 32768, three alternating runs each
# Every GPU step runs under its own time limit, and the first one that fails ends the script.
# usage: [PARTS=123456] [OUT=dir] tools/exp_i8_sample_scan.sh [other_libqdrant_amd.so]     (writes $OUT/r16_i8_sample_scan_<PARTS>.txt; OUT defaults to exp_out)
set -u -o pipefail
other=${1:-}
outdir=${OUT:-$PWD/exp_out}
parts=${PARTS:-123456}
out=$outdir/r16_i8_sample_scan_$parts.txt
lib=qdrant_amd/libqdrant_amd.so
mkdir -p $outdir
: > $out
plain="--gpus 1 --steps 100 --warmup 10"
bench() {   # label, env assignment, extra bench arguments...
    local label=$1 setting=$2; shift 2
    local line
    line=$(timeout -k 10 300 env $setting python bench.py $plain "$@" 2> $outdir/r16_last.err | tail -n 1) || { echo "FAILED: $label" | tee -a $out; tail -n 5 $outdir/r16_last.err; return 1; }
    echo "$label $(echo "$line" | python3 -c "import sys, json; d = json.loads(sys.stdin.read()); print('qps', d['value'], 'ms_per_step', d['ms_per_step'])")" | tee -a $out
}
# (this build's library is set aside while the other one stands in its place, and put back on ANY way out of the script)
swap_in_other() { cp $lib $outdir/r16_this_lib.so && cp "$other" $lib; }
swap_back() { if [ -f $outdir/r16_this_lib.so ]; then cp $outdir/r16_this_lib.so $lib && rm -f $outdir/r16_this_lib.so; fi; }
trap swap_back EXIT
trace() {   # label, directory tag, extra bench arguments...
    local label=$1 tag=$2; shift 2
    rm -rf $outdir/r16_trace_$tag
    timeout -k 10 420 rocprofv3 --kernel-trace --stats --output-format csv -d $outdir/r16_trace_$tag -o t -- python bench.py $plain "$@" > $outdir/r16_traced_bench_$tag.json 2> $outdir/r16_trace_$tag.err \
        || { echo "FAILED: trace of $label" | tee -a $out; tail -n 5 $outdir/r16_trace_$tag.err; return 1; }
    local csv stats
    csv=$(find $outdir/r16_trace_$tag -name '*kernel_trace.csv' | head -1)
    stats=$(find $outdir/r16_trace_$tag -name '*kernel_stats.csv' | head -1)
    echo "$label (traced run: $(tail -n 1 $outdir/r16_traced_bench_$tag.json | cut -c1-120))" | tee -a $out
    python3 tools/scan_overlap.py "$csv" | tee -a $out
    python3 tools/i8_launch_split.py "$csv" 10000000 ${TRACE_DIM:-768} 16 | tee -a $out
    [ -n "$stats" ] && head -n 20 "$stats" > $outdir/r16_kernel_stats_$tag.csv
    rm -rf $outdir/r16_trace_$tag
}
if [[ $parts == *1* ]]; then
echo "# 1. python bench.py $plain, alternating" | tee -a $out
for i in 1 2 3 4 5; do
    for v in 0 1; do
        extra=""
        [ $i -eq 1 ] && extra="--dump-outputs $outdir/r16_dump_$v"
        bench "QMX_I8_SAMPLE_SCAN=$v run $i" QMX_I8_SAMPLE_SCAN=$v $extra || exit 1
    done
done
for f in ids scores counts; do
    python3 -c "import sys, numpy as np; sys.exit(0 if np.array_equal(np.load('$outdir/r16_dump_0/$f.npy'), np.load('$outdir/r16_dump_1/$f.npy')) else 1)" \
        && echo "dump $f.npy: np.array_equal with 0 and 1" | tee -a $out || { echo "dump $f.npy DIFFERS" | tee -a $out; exit 1; }
done
rm -rf $outdir/r16_dump_0 $outdir/r16_dump_1
fi
if [[ $parts == *2* ]] && [ -n "$other" ]; then
    echo "# 2. the other library (the parent commit's build)" | tee -a $out
    swap_in_other || exit 1
    for i in 1 2; do bench "other library run $i" QMX_I8_SAMPLE_SCAN=0 || exit 1; done
    swap_back || exit 1
fi
if [[ $parts == *3* ]]; then
echo "# 3. rocprofv3 --kernel-trace --stats -- python bench.py $plain" | tee -a $out
export TMPDIR=/tmp
if [ -n "$other" ]; then
    swap_in_other || exit 1
    trace "other library" other
    rc=$?
    swap_back || exit 1
    [ $rc -eq 0 ] || exit 1
fi
trace "this library" this || exit 1
fi
if [[ $parts == *4* ]]; then
echo "# 4. --full: the timed path against the exact scan" | tee -a $out
# (the headline leg, its check against the exact scan of the whole block and the robustness legs; not the other configurations, sweeps and CPU baseline)
line=$(timeout -k 10 900 python bench.py --full --steps 100 --warmup 10 --configs= --no-sweep --no-cpu --no-other-copy-point --fanout-rows 0 --no-hbm-point \
       --details $outdir/r16_full_details.json 2> $outdir/r16_last.err | tail -n 1) || { echo "FAILED: --full" | tee -a $out; tail -n 5 $outdir/r16_last.err; exit 1; }
echo "$line" | python3 -c "import sys, json; d = json.loads(sys.stdin.read()); print('full run: qps', d['value'], 'checks', d.get('checks'), 'recall_at_10', d.get('recall_at_10', d.get('checks', {}).get('recall_at_10')))" | tee -a $out
python3 -c "
import json
d = json.load(open('$outdir/r16_full_details.json'))
def walk(x, path=''):
    if isinstance(x, dict):
        for k, v in x.items():
            if isinstance(v, (dict, list)): walk(v, path + '/' + k)
            elif 'equal' in k or 'recall' in k or 'fallback' in k: print('  ', path + '/' + k, '=', v)
    elif isinstance(x, list):
        for i, v in enumerate(x): walk(v, path + '/%d' % i)
walk(d)
" | tee -a $out
fi
if [[ $parts == *5* ]]; then
echo "# 5. rocprofv3 --kernel-trace --stats -- python bench.py $plain --dim 1024" | tee -a $out
export TMPDIR=/tmp
TRACE_DIM=1024 trace "this library, --dim 1024" dim1024 --dim 1024 || exit 1
fi
if [[ $parts == *6* ]]; then
echo "# 6. the sample's size, alternating" | tee -a $out
for i in 1 2 3; do
    for rows in 8192 16384 32768; do
        bench "QMX_I8_SAMPLE_ROWS=$rows run $i" QMX_I8_SAMPLE_ROWS=$rows || exit 1
    done
done
fi
