#!/bin/bash
# Profiling tool (not product): libquadenv.so with extra -D flags -> tools/_build/var_<name>.so
# (the product build, csrc/Makefile, with those flags, in its own object directory).
# Usage: build_variant.sh name "-DFOO=1 -DBAR" [name2 "flags2" ...]
set -e
cd "$(dirname "$0")/../../uav_reinforcement_learning_control_amd/csrc"
B=../../tools/_build
while [ $# -ge 2 ]; do
  name=$1; flags=$2; shift 2
  make -s -j8 OUT=$B/var_$name/libquadenv.so DEFS="$flags"
  cp $B/var_$name/libquadenv.so $B/var_$name.so
done
