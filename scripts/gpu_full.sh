#!/bin/bash
# full GPU suite (one process), then the config-2 bench line (--full: roofline and host_api included)
# logs go to $OUT (default bench_out/)
set -o pipefail
OUT=${OUT:-bench_out}
mkdir -p $OUT
timeout -k 10 1000 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > $OUT/full_gpu.log 2>&1 || { tail -40 $OUT/full_gpu.log; exit 1; }
tail -2 $OUT/full_gpu.log
timeout -k 10 400 python -u bench.py --steps 20 --warmup 3 --full > $OUT/bench_c2.log 2>&1 || { tail -20 $OUT/bench_c2.log; exit 2; }
tail -1 $OUT/bench_c2.log | python3 -c "import json,sys; r=json.loads(sys.stdin.read()); print(r['ms_per_step'], r['roofline']['frac'], r.get('host_api'))"
