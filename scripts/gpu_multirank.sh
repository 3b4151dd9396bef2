#!/bin/bash
# Multi-rank rehearsal on one GPU (gloo; the driver runs the real N-GPU RCCL scaling).
set -u
OUT=${OMLDM_OUT:-out}  # where this script leaves its records
mkdir -p $OUT
export HSA_ENABLE_IPC_MODE_LEGACY=0
timeout -k 10 300 python -m pytest tests/test_multirank_gpu.py -m gpu -q -x > $OUT/pytest_multirank.log 2>&1 || { tail -30 $OUT/pytest_multirank.log; exit 2; }
tail -1 $OUT/pytest_multirank.log
OMLDM_DIST_BACKEND=gloo timeout -k 10 300 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29650 bench.py --gpus 2 --full --steps 10 --warmup 2 --latency-samples 50 > $OUT/bench_2rank.log 2>&1 || { tail -30 $OUT/bench_2rank.log; exit 3; }
tail -1 $OUT/bench_2rank.log
