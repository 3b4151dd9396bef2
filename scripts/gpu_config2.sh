#!/bin/bash
# BASELINE config 2 (logistic regression, bf16 model, 2^20 hashed features): pinned-host
# stream and HBM-resident ingest.
set -u
R=${GRAFT_REPO_ROOT:-$PWD}
OUT=${OMLDM_OUT:-$R/out}  # where this script leaves its records
mkdir -p $OUT
cd $R
timeout -k 10 240 python bench.py --full --learner LogisticRegression --steps 200 --warmup 20 > $OUT/cfg2_pinned.json 2> $OUT/cfg2_pinned.err || { tail -20 $OUT/cfg2_pinned.err; exit 3; }
timeout -k 10 240 python bench.py --full --learner LogisticRegression --ingest device --steps 200 --warmup 20 > $OUT/cfg2_device.json 2> $OUT/cfg2_device.err || { tail -20 $OUT/cfg2_device.err; exit 3; }
cat $OUT/cfg2_pinned.json $OUT/cfg2_device.json
