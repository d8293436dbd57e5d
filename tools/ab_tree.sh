#!/bin/bash
# same-box A/B of two whole trees: this one (new) against a built copy of another commit under tools/ab/parent (old), alternating,
# as tools/ab_lib.sh alternates two libraries - for changes after which the old library no longer loads under the new binding
# (a new C-ABI entry point).  REPS (default 3) runs each; prints ms_per_step, roofline fraction, act_up / act_down / grad us.
cd "$(dirname "$0")/.." || exit 1          # the repository root, wherever the script is called from
line() { python -c "import sys,json; d=json.loads(sys.stdin.read()); k=d['roofline']['kernels']; print('$1', d['ms_per_step'], d['roofline']['frac'], k['act_up']['avg_us'], k['act_down']['avg_us'], k['grad']['avg_us'])"; }
for rep in $(seq ${REPS:-3}); do
  for v in old new; do
    if [ $v = old ]; then d=tools/ab/parent; else d=.; fi
    (cd $d && timeout 200 python bench.py --full --no-others --no-cpu 2>/dev/null | tail -1 | line "$v 2000") || exit 1
  done
done
