#!/bin/bash
# Profiling tool (not product): cost-ablation builds of libquadenv.so for tools/rollout_variants.py --
# k_rollout without the env step, without the MLPs, without the critic, without the obs-copy rows
# (NOOBSCOPY). (The round-4 alternatives PK0 / ALP0 were dropped from the product source in round 6.)
# Output: tools/_build/roll_*.so
# Each variant is the product build (csrc/Makefile, its flags) with one -D, in its own object directory.
set -e
cd "$(dirname "$0")/../uav_reinforcement_learning_control_amd/csrc"
B=../../tools/_build
for v in NOENV NOMLP NOCRITIC NOOBSCOPY; do
  make -s -j8 OUT=$B/roll_$v/libquadenv.so DEFS=-DQD_ROLL_$v
  cp $B/roll_$v/libquadenv.so $B/roll_$v.so
done
