#!/bin/bash
# bench.py A/B: each argument is a tag of extra bench flags (commas for spaces).
set -e
OUT=${OMLDM_OUT:-out}  # where this script leaves its records
mkdir -p $OUT/r5
for tag in "$@"; do
  name=$(echo "$tag" | tr '=,-' '___')
  timeout -k 10 300 python bench.py --full --steps 5 --warmup 2 $(echo "$tag" | tr ',' ' ') > $OUT/r5/bab_${name}.json 2> $OUT/r5/bab_${name}.err
done
