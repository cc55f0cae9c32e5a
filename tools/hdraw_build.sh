#!/bin/bash
# Profiling tool (not product): k_step_h's helper reset-draw cost ablations -> tools/_build/hd_HDRAW0.so
# (the reset row from a cheap hash instead of the 4 Philox blocks) and hd_HROW0.so (no reset row);
# ("A+B" builds both ablations); A/B with tools/lib_ab.py N tools/_build/hd_HDRAW0.so tools/_build/hd_HROW0.so
# Each variant is the product build (csrc/Makefile, its flags) with its -D flags, in its own object directory.
set -e
cd "$(dirname "$0")/../uav_reinforcement_learning_control_amd/csrc"
B=../../tools/_build
for v in ${VARIANTS:-HDRAW0 HROW0}; do
  make -s -j8 OUT=$B/hd_$v/libquadenv.so DEFS="-DQD_ABL_$(echo $v | sed "s/+/ -DQD_ABL_/g")"
  cp $B/hd_$v/libquadenv.so $B/hd_$v.so
done
