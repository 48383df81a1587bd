#!/bin/bash
# GPU parity suite under every switch that turns a fast path off (README "Environment switches"); one line per run.
# Usage on the GPU box: bash tools/run_fallback_matrix.sh [quick|core]   (quick: the switches of the batched fast path only;
# core: every switch, but only the parity / KAT / close-first / tail-edges files - two minutes per switch instead of five)
# MATRIX_EXTRA="SETTING ...": further settings, one run each behind the list's - for a switch that keeps every batch on its
# kernels and only changes what a kernel does (the lean emission's, the lean ranks' and the lean count's, README "Environment switches"): the route assertions of the
# tests hold the list below to the switches that move a batch to other kernels
set -o pipefail
ALL=("" VOFOD_CLOSE_FIRST=0 VOFOD_DEVICE_TAIL=0 VOFOD_SLABS=0 VOFOD_SLAB_EMIT=0 VOFOD_BRICK_LDS=0 VOFOD_DILATE=0 VOFOD_CCL=voxel "VOFOD_CLOSE_FIRST=0 VOFOD_DEVICE_TAIL=0" VOFOD_EXPLORE=host)
QUICK=(VOFOD_CLOSE_FIRST=0 VOFOD_DEVICE_TAIL=0 VOFOD_BRICK_LDS=0 VOFOD_CCL=voxel)
if [ "$1" = quick ]; then SW=("${QUICK[@]}"); else SW=("${ALL[@]}"); fi
for x in $MATRIX_EXTRA; do SW+=("$x"); done
TESTS=tests
if [ "$1" = core ]; then TESTS="tests/test_gpu_parity.py tests/test_gpu_kat.py tests/test_gpu_close_first.py tests/test_gpu_close_first_edges.py tests/test_gpu_tail_edges.py tests/test_gpu_lean_emit.py tests/test_gpu_lean_ranks.py tests/test_gpu_lean_count.py tests/test_gpu_detection_points.py"; fi
# optional: first switch and number of switches (run_fallback_matrix.sh core 4 4: the fifth to the eighth), to take the matrix in parts
FIRST=${2:-0}
COUNT=${3:-${#SW[@]}}
for sw in "${SW[@]:$FIRST:$COUNT}"; do
  printf "%-36s " "${sw:-default}"
  env $sw timeout -k 10 900 python -m pytest $TESTS -x -q -m gpu 2>&1 | grep -E "^FAILED|passed|failed|error" | tail -3 | tr "\n" " "
  rc=${PIPESTATUS[0]}
  echo
  # a run that was killed (time limit, abort, segmentation fault) may have left the GPU in a bad state: nothing more is started on it
  if [ "$rc" -ge 124 ]; then echo "run ended with status $rc: stopping here"; exit "$rc"; fi
done
