#!/bin/bash
# the CKKS linear operations, one pz_glwe_combine_batched call each (tools/bench_ckks_linear.py, configs[4] shapes): one JSON line per op
# on stdout, e.g.  tools/bench_lines_ckks.sh > profiles/rNN_ckks_linear_lines.jsonl
for op in add add_unequal sub neg rescale add_pt; do
    timeout -k 10 600 python tools/bench_ckks_linear.py --op $op || exit $?
done
