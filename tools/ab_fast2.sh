#!/bin/bash
# same-box A/B of the two FAST kernels of the whole path, production shape (pipelined) and one batch at a time
O=${1:-out/ab}
mkdir -p $O
for rep in 1 2; do
for impl in 3 4; do
  ORBX_FAST_IMPL=$impl timeout -k 10 200 python bench.py --full --only-timed --no-cpu-baseline > $O/ab.json 2> $O/ab.err
  python -c "
import json; d=json.load(open('$O/ab.json')); print('impl', $impl, 'one batch at a time', round(d['value']), d['roofline_kernels_ms'])"
  ORBX_FAST_IMPL=$impl timeout -k 10 300 python bench.py --full --no-cpu-baseline --strong-frames 0 > $O/ab.json 2> $O/ab.err
  python -c "
import json; d=json.load(open('$O/ab.json')); print('impl', $impl, 'pipelined', round(d['value']), round(d['value_full_work']), round(d['value_sustained']), round(d['fps_with_d2h']))"
  ORBX_FAST_IMPL=$impl timeout -k 10 300 python bench.py --full --no-cpu-baseline --strong-frames 0 --batch 256 > $O/ab.json 2> $O/ab.err
  python -c "
import json; d=json.load(open('$O/ab.json')); print('impl', $impl, 'pipelined 256', round(d['value']), round(d['value_full_work']), round(d['value_sustained']), round(d['fps_with_d2h']))"
done
done
