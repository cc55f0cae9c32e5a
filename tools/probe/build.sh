#!/bin/bash
# Profiling tool (not product): libquadenv.so built with -DQD_PROBE (k_step_h records per-wave
# s_memtime phase stamps into the target_info buffer) -> tools/_build/probe.so
# (the product build, csrc/Makefile, with the extra -D flags, in its own object directory)
set -e
cd "$(dirname "$0")/../../uav_reinforcement_learning_control_amd/csrc"
B=../../tools/_build
make -s -j8 OUT=$B/probe/libquadenv.so DEFS="-DQD_PROBE ${EXTRA:-}"
cp $B/probe/libquadenv.so $B/probe.so
