#!/bin/bash
# Timing ablations of the fused transposed conv + blur launch (csrc/tconv_blur.hip) on the two top up-sampling layers at 32 samples.  Experiment builds first:
#   for v in 0 1 2 4 3; do tools/build_exp.sh tb$v "-DMGF_TB_ABL=$v" tconv_blur.hip; done
# MGF_TB_ABL: 1 no blur and no stores, 2 no halo columns (32 owned lanes), 4 the blur without its global stores (bits add; results are wrong, times are not).
# Same box:  bash tools/tconv_blur_abl.sh OUT
D=${1:-tb_abl_out}; mkdir -p $D
for v in 0 4 1 2 3 0; do
  echo "== MGF_TB_ABL=$v" | tee -a $D/abl.txt
  MGF_LIB_PATH=$PWD/exp_build/libmgf_tb$v.so timeout -k 10 120 python tools/tconv_blur_micro.py 32 20 2>$D/tb$v.err | grep -v "^    " | tee -a $D/abl.txt || exit 1
done
