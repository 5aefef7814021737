#!/bin/bash
# same-box A/B of the two FAST kernels of the whole path (development aid)
O=${1:-out/ab}
mkdir -p $O
for rep in 1 2; do
for impl in 3 4; do
  for mode in "" "--full-work"; do
    ORBX_FAST_IMPL=$impl timeout -k 10 200 python bench.py --full --only-timed --no-cpu-baseline $mode > $O/ab.json 2> $O/ab.err
    python -c "
import json; d=json.load(open('$O/ab.json')); print('impl', $impl, '$mode', round(d['value']), d['roofline_kernels_ms'])"
  done
done
done
