#!/bin/bash
# The dense epilogue of the int8 prefilter's first launch (option i8_dense_epilogue) against the one epilogue for both launches, on ONE box in one go:
#   1. the headline command, alternating QMX_I8_DENSE_EPILOGUE=0 / 1 (five of each; the first of each also dumps its last step's lists, which must be equal)
#   2. the same command on another build of the library, twice (give the parent commit's library: option 0 is supposed to be it)
#   3. the first launch's stride (QMX_I8_SAMPLE_STRIDE = 8 / 16 / 32), three runs each
#   4. one kernel trace per option value, in runs of their own: the two launches' mean durations (tools/i8_launch_split.py)
#   5. one --full run: the timed path against the exact scan
# Every GPU step runs under its own time limit, and the first one that fails ends the script.
# usage: [PARTS=12345] [OUT=dir] tools/exp_i8_dense_epilogue.sh [other_libqdrant_amd.so]     (writes $OUT/r14_i8_dense_epilogue_<PARTS>.txt; OUT defaults to exp_out)
set -u -o pipefail
other=${1:-}
outdir=${OUT:-$PWD/exp_out}
parts=${PARTS:-12345}
out=$outdir/r14_i8_dense_epilogue_$parts.txt
lib=qdrant_amd/libqdrant_amd.so
mkdir -p $outdir
: > $out
plain="--gpus 1 --steps 100 --warmup 10"
bench() {   # label, env assignment, extra bench arguments...
    local label=$1 setting=$2; shift 2
    local line
    line=$(timeout -k 10 300 env $setting python bench.py $plain "$@" 2> $outdir/r14_last.err | tail -n 1) || { echo "FAILED: $label" | tee -a $out; tail -n 5 $outdir/r14_last.err; exit 1; }
    echo "$label $(echo "$line" | python3 -c "import sys, json; d = json.loads(sys.stdin.read()); print('qps', d['value'], 'ms_per_step', d['ms_per_step'])")" | tee -a $out
}
if [[ $parts == *1* ]]; then
echo "# 1. python bench.py $plain, alternating" | tee -a $out
for i in 1 2 3 4 5; do
    for v in 0 1; do
        extra=""
        [ $i -eq 1 ] && extra="--dump-outputs $outdir/r14_dump_$v"
        bench "QMX_I8_DENSE_EPILOGUE=$v run $i" QMX_I8_DENSE_EPILOGUE=$v $extra
    done
done
for f in ids scores counts; do
    cmp $outdir/r14_dump_0/$f.npy $outdir/r14_dump_1/$f.npy && echo "dump $f.npy: identical with 0 and 1" | tee -a $out || { echo "dump $f.npy DIFFERS" | tee -a $out; exit 1; }
done
fi
if [[ $parts == *2* ]] && [ -n "$other" ]; then
    echo "# 2. the other library ($other)" | tee -a $out
    cp $lib $outdir/r14_this_lib.so && cp "$other" $lib || exit 1
    for i in 1 2; do bench "other library run $i" QMX_I8_DENSE_EPILOGUE=0; done
    cp $outdir/r14_this_lib.so $lib && rm -f $outdir/r14_this_lib.so || exit 1
fi
if [[ $parts == *3* ]]; then
echo "# 3. the first launch's stride (dense epilogue)" | tee -a $out
for i in 1 2 3; do
    for st in 8 16 32; do bench "QMX_I8_SAMPLE_STRIDE=$st run $i" QMX_I8_SAMPLE_STRIDE=$st; done
done
fi
if [[ $parts == *4* ]]; then
echo "# 4. rocprofv3 --kernel-trace --stats -- python bench.py $plain" | tee -a $out
export TMPDIR=/tmp
for v in 0 1; do
    rm -rf $outdir/r14_trace_$v
    timeout -k 10 420 env QMX_I8_DENSE_EPILOGUE=$v rocprofv3 --kernel-trace --stats --output-format csv -d $outdir/r14_trace_$v -o t -- python bench.py $plain > $outdir/r14_traced_bench_$v.json 2> $outdir/r14_trace_$v.err \
        || { echo "FAILED: trace $v" | tee -a $out; tail -n 5 $outdir/r14_trace_$v.err; exit 1; }
    csv=$(find $outdir/r14_trace_$v -name '*kernel_trace.csv' | head -1)
    stats=$(find $outdir/r14_trace_$v -name '*kernel_stats.csv' | head -1)
    echo "QMX_I8_DENSE_EPILOGUE=$v (traced run: $(tail -n 1 $outdir/r14_traced_bench_$v.json | cut -c1-120))" | tee -a $out
    python3 tools/i8_launch_split.py "$csv" | tee -a $out
    [ -n "$stats" ] && head -n 12 "$stats" > $outdir/r14_kernel_stats_$v.csv
    rm -rf $outdir/r14_trace_$v
done
fi
if [[ $parts == *5* ]]; then
echo "# 5. --full: the timed path against the exact scan" | tee -a $out
line=$(timeout -k 10 500 python bench.py --full --steps 100 --warmup 10 --configs= --no-sweep --no-robustness --no-cpu --no-other-copy-point --fanout-rows 0 --no-hbm-point \
       --details $outdir/r14_full_details.json 2> $outdir/r14_last.err | tail -n 1) || { echo "FAILED: --full" | tee -a $out; tail -n 5 $outdir/r14_last.err; exit 1; }
echo "$line" | python3 -c "import sys, json; d = json.loads(sys.stdin.read()); print('full run: qps', d['value'], 'checks', d.get('checks'), 'recall_at_10', d.get('recall_at_10', d.get('checks', {}).get('recall_at_10')))" | tee -a $out
fi
