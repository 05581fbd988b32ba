#!/bin/bash
# A/B of two builds of the library on one box: tools/ab_lib.sh <tag> ; libmcq_alt.so beside libmcq_hip.so
O=${AB_OUT:-ab_out}; mkdir -p $O
for rep in 1 2 3; do
python bench.py --full --steps 10 --warmup 3 --no-secondary > $O/ab_main_$rep.json 2>/dev/null
MCQ_ALLOW_LIB_PATH=1 MCQ_LIB_PATH=$PWD/quantization_amd/lib/libmcq_alt.so python bench.py --full --steps 10 --warmup 3 --no-secondary > $O/ab_alt_$rep.json 2>/dev/null
done
