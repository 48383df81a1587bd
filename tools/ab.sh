#!/bin/bash
# A/B of builds of the library on ONE box (box-to-box variance is larger than most kernel changes):
# ab_libs/<V>.so are copied over the in-tree library in turn, bench runs interleaved.  usage: tools/ab.sh "A B C" [rounds]
# Prints the pipelined rate and the kernels' own durations (HIP events, one batch at a time: the steadier number).
# AB_OUT=<dir>: every run's JSON line is kept there as <V>_<round>.json (the side legs of --full are read from those).
# Stops at the first run that fails: nothing more is started on a GPU that a run may have left in a bad state.
set -o pipefail
VARS=${1:-"A B"}
ROUNDS=${2:-3}
[ -n "$AB_OUT" ] && mkdir -p "$AB_OUT"
for i in $(seq $ROUNDS); do
  for v in $VARS; do
    cp ab_libs/$v.so vofod_amd/csrc/libvofod_hip.so || exit 1
    timeout -k 10 200 python bench.py --full --steps 40 --warmup 8 --cpu-baseline-scans 0 --host-input-steps 0 2>/dev/null | tee ${AB_OUT:+$AB_OUT/${v}_$i.json} | python -c "import json,sys; d=json.loads(sys.stdin.read()); k=d['kernels']; print('$v', round(d['value']), round(d['ms_per_step'],3), {n.split('<')[0]: round(x['avg_us'],1) for n,x in k.items() if n.startswith(('k_key1','k_frame_lds'))})" || exit 1
  done
done
