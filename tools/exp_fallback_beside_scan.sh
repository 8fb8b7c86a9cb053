#!/bin/bash
# The conditional exact pass of the int8 prefilter as one launch that fits beside a resident scan block (option fallback_beside_scan) against the former
# 16-query pass and 64-query passes, on ONE box in one go:
#   1. the headline command, alternating QMX_FALLBACK_BESIDE_SCAN=0 / 1 (five of each; the first of each also dumps its last step's lists, which must be equal)
#   2. the same command on another build of the library, twice (give the parent commit's library: option 0 is supposed to be it)
#   3. one kernel trace of the other library and one of this one, in runs of their own (tools/scan_overlap.py)
#   4. one --full run without the side legs: the timed path against the exact scan and the robustness legs - and, with another library given, the same run
#      on it: the leg in which every query overflows (student5 / int8_copy) is where the new form pays, both figures are printed
#   5. one kernel trace of this library at --dim 1024, where the former passes must still be what runs
# Every GPU step runs under its own time limit, and the first one that fails ends the script.
# usage: [PARTS=12345] [OTHER_AROUND=1] [OUT=dir] tools/exp_fallback_beside_scan.sh [other_libqdrant_amd.so]     (writes $OUT/r17_fallback_beside_scan_<PARTS>.txt; OUT defaults to exp_out)
set -u -o pipefail
other=${1:-}
outdir=${OUT:-$PWD/exp_out}
parts=${PARTS:-12345}
out=$outdir/r17_fallback_beside_scan_$parts.txt
lib=qdrant_amd/libqdrant_amd.so
mkdir -p $outdir
: > $out
plain="--gpus 1 --steps 100 --warmup 10"
bench() {   # label, env assignment, extra bench arguments...
    local label=$1 setting=$2; shift 2
    local line
    line=$(timeout -k 10 300 env $setting python bench.py $plain "$@" 2> $outdir/r17_last.err | tail -n 1) || { echo "FAILED: $label" | tee -a $out; tail -n 5 $outdir/r17_last.err; return 1; }
    echo "$label $(echo "$line" | python3 -c "import sys, json; d = json.loads(sys.stdin.read()); print('qps', d['value'], 'ms_per_step', d['ms_per_step'])")" | tee -a $out
}
# (this build's library is set aside while the other one stands in its place, and put back on ANY way out of the script)
swap_in_other() { cp $lib $outdir/r17_this_lib.so && cp "$other" $lib; }
swap_back() { if [ -f $outdir/r17_this_lib.so ]; then cp $outdir/r17_this_lib.so $lib && rm -f $outdir/r17_this_lib.so; fi; }
trap swap_back EXIT
trace() {   # label, directory tag, extra bench arguments...
    local label=$1 tag=$2; shift 2
    rm -rf $outdir/r17_trace_$tag
    timeout -k 10 420 rocprofv3 --kernel-trace --stats --output-format csv -d $outdir/r17_trace_$tag -o t -- python bench.py $plain "$@" > $outdir/r17_traced_bench_$tag.json 2> $outdir/r17_trace_$tag.err \
        || { echo "FAILED: trace of $label" | tee -a $out; tail -n 5 $outdir/r17_trace_$tag.err; return 1; }
    local csv stats
    csv=$(find $outdir/r17_trace_$tag -name '*kernel_trace.csv' | head -1)
    stats=$(find $outdir/r17_trace_$tag -name '*kernel_stats.csv' | head -1)
    echo "$label (traced run: $(tail -n 1 $outdir/r17_traced_bench_$tag.json | cut -c1-120))" | tee -a $out
    python3 tools/scan_overlap.py "$csv" | tee -a $out
    # which instantiations of the chain-major scan ran, and how often
    python3 -c "
import csv, collections, sys
n = collections.Counter(r['Kernel_Name'].split('(')[0] for r in csv.DictReader(open(sys.argv[1])) if 'scan_f32_mfma16_kernel' in r['Kernel_Name'])
for k, v in sorted(n.items()): print('   ', v, 'x', k)
" "$csv" | tee -a $out
    [ -n "$stats" ] && head -n 24 "$stats" > $outdir/r17_kernel_stats_$tag.csv
    rm -rf $outdir/r17_trace_$tag
}
full() {   # label, details tag
    local label=$1 tag=$2 line
    # (the headline leg, its check against the exact scan of the whole block and the robustness legs; not the other configurations, sweeps and CPU baseline)
    line=$(timeout -k 10 900 python bench.py --full --steps 100 --warmup 10 --configs= --no-sweep --no-cpu --no-other-copy-point --fanout-rows 0 --no-hbm-point \
           --details $outdir/r17_full_details_$tag.json 2> $outdir/r17_last.err | tail -n 1) || { echo "FAILED: --full, $label" | tee -a $out; tail -n 5 $outdir/r17_last.err; return 1; }
    echo "$line" | python3 -c "import sys, json; d = json.loads(sys.stdin.read()); print('$label: --full run: qps', d['value'], 'checks', d.get('checks'), 'recall_at_10', d.get('recall_at_10', d.get('checks', {}).get('recall_at_10')))" | tee -a $out
    python3 -c "
import json
d = json.load(open('$outdir/r17_full_details_$tag.json'))
def walk(x, path=''):
    if isinstance(x, dict):
        for k, v in x.items():
            if isinstance(v, (dict, list)): walk(v, path + '/' + k)
            elif 'equal' in k or 'recall' in k or 'fallback' in k: print('  ', path + '/' + k, '=', v)
    elif isinstance(x, list):
        for i, v in enumerate(x): walk(v, path + '/%d' % i)
walk(d)
leg = d.get('robustness', {}).get('student5', {}).get('int8_copy', {})
print('   student5 / int8_copy ($label): qps', leg.get('qps'), 'ms_per_step', leg.get('ms_per_step'), 'fallback_queries_per_batch', leg.get('fallback_queries_per_batch'))
" | tee -a $out
}
other_run() {   # run number
    swap_in_other || return 1
    bench "other library run $1" QMX_FALLBACK_BESIDE_SCAN=0
    local rc=$?
    swap_back || return 1
    return $rc
}
# (OTHER_AROUND=1: the other library's two runs stand before and behind the alternating runs, not both behind them - a box that drifts over a call
#  then shows it in their difference)
if [[ $parts == *2* ]] && [ -n "$other" ] && [ "${OTHER_AROUND:-0}" = 1 ]; then
    echo "# 2. the other library (the parent commit's build): one run before part 1, one behind it" | tee -a $out
    other_run 1 || exit 1
fi
if [[ $parts == *1* ]]; then
echo "# 1. python bench.py $plain, alternating" | tee -a $out
for i in 1 2 3 4 5; do
    for v in 0 1; do
        extra=""
        [ $i -eq 1 ] && extra="--dump-outputs $outdir/r17_dump_$v"
        bench "QMX_FALLBACK_BESIDE_SCAN=$v run $i" QMX_FALLBACK_BESIDE_SCAN=$v $extra || exit 1
    done
done
for f in ids scores counts; do
    python3 -c "import sys, numpy as np; sys.exit(0 if np.array_equal(np.load('$outdir/r17_dump_0/$f.npy'), np.load('$outdir/r17_dump_1/$f.npy')) else 1)" \
        && echo "dump $f.npy: np.array_equal with 0 and 1" | tee -a $out || { echo "dump $f.npy DIFFERS" | tee -a $out; exit 1; }
done
rm -rf $outdir/r17_dump_0 $outdir/r17_dump_1
fi
if [[ $parts == *2* ]] && [ -n "$other" ]; then
    if [ "${OTHER_AROUND:-0}" = 1 ]; then
        other_run 2 || exit 1
    else
        echo "# 2. the other library (the parent commit's build)" | tee -a $out
        for i in 1 2; do other_run $i || exit 1; done
    fi
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
echo "# 4. --full: the timed path against the exact scan, the robustness legs" | tee -a $out
full "this library" this || exit 1
if [ -n "$other" ]; then
    swap_in_other || exit 1
    full "other library" other
    rc=$?
    swap_back || exit 1
    [ $rc -eq 0 ] || exit 1
fi
fi
if [[ $parts == *5* ]]; then
echo "# 5. rocprofv3 --kernel-trace --stats -- python bench.py $plain --dim 1024" | tee -a $out
export TMPDIR=/tmp
trace "this library, --dim 1024" dim1024 --dim 1024 || exit 1
fi
