#!/bin/bash
# Profiling tool (not product): cost-ablation builds of libquadenv.so for tools/learner_bench.py --
# quad_ppo_grad without the L2 MFMAs, without the weight-gradient MFMAs (dW2, dW3), without
# dh1 + dW1. Output: tools/_build/lrn_*.so (run learner_bench.py with QUADENV_LIB=<so>).
# Each variant is the product build (csrc/Makefile, its flags) with one -D, in its own object directory.
set -e
cd "$(dirname "$0")/../uav_reinforcement_learning_control_amd/csrc"
B=../../tools/_build
for v in NOL2 NODW NODH1; do
  make -s -j8 OUT=$B/lrn_$v/libquadenv.so DEFS=-DQD_LRN_$v
  cp $B/lrn_$v/libquadenv.so $B/lrn_$v.so
done
