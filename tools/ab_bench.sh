#!/bin/bash
# A/B on ONE GPU box (box-to-box spread is +-3 %): alternate bench.py runs of the product library and of the
# variant libraries given as arguments (paths, loaded through SSX_HIP_LIB_OVERRIDE), three rounds each.
# usage: [BENCH_ARGS="--scene plane-srgb ..."] tools/ab_bench.sh [variant.so ...]   -> prints value / ms_per_step / kernel_ms per run
# Every run has a time limit of its own (AB_TIMEOUT seconds, default 300), and the script stops at the first run that fails or is killed at its limit.
export SSX_DEBUG_ENV=1 # the master switch of the A/B environment variables (README)
set -o pipefail
R=$(pwd)
T="timeout -k 10 ${AB_TIMEOUT:-300}"
P='import json,sys; d=json.loads(sys.stdin.read()); print(sys.argv[1], d["value"], d["ms_per_step"], d["roofline"]["kernel_ms"], d["roofline"]["stage_ms"], d["roofline"]["scratch_bytes"])'
for round in 1 2 3; do
	$T python $R/bench.py --steps 10 --warmup 2 --quick $BENCH_ARGS 2>/dev/null | python -c "$P" product || exit 1
	for V in "$@"; do
		SSX_HIP_LIB_OVERRIDE=$R/$V $T python $R/bench.py --steps 10 --warmup 2 --quick $BENCH_ARGS 2>/dev/null | python -c "$P" $V || exit 1
	done
done
