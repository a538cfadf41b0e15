#!/bin/bash
# usage: tools/round_numbers.sh <full record .json> <bench line .json>
python bench.py --full --full-json "${1:?full record path}" > "${2:?bench line path}" 2> "$2.err"
echo "bench rc=$?"
wc -c "$2"
export SLAMPP_HIP_DEV=1
SETTLE_MS=30 REPS=5 python3 tools/cold_path.py c1 c2 c3 venice band c5 uniform 1kx1m 2>/dev/null > gpurun_out/r06_cold_path.txt
cat gpurun_out/r06_cold_path.txt
REPS=9 python3 tools/time_dropin.py c3 venice > gpurun_out/r06_dropin.txt 2>&1
cat gpurun_out/r06_dropin.txt
