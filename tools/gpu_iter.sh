#!/bin/bash
# one gpurun call of the optimisation loop: GPU parity suite (fail fast), phase stamps of the frame kernel, bench line
TAG=${1:-x}
O=${OUT:-out}; mkdir -p $O  # (results directory)
timeout -k 10 800 python -m pytest tests -q -m gpu -x --durations=3 > $O/${TAG}_test.log 2>&1; tail -6 $O/${TAG}_test.log
VOFOD_LDS_PROF=1 timeout -k 10 300 python bench.py --full --steps 2 --warmup 1 --cpu-baseline-scans 0 --no-profile-pass > $O/${TAG}_prof.json 2> $O/${TAG}_prof.err; grep k_frame $O/${TAG}_prof.err | tail -4
timeout -k 10 300 python bench.py --full --cpu-baseline-scans 0 > $O/${TAG}_bench.json 2> $O/${TAG}_bench.err
python -c "
import json;d=json.load(open('$O/${TAG}_bench.json'));print(round(d['value']),round(d['ms_per_step'],3)); print({k:round(v['avg_us'],1) for k,v in d['kernels'].items()})"
