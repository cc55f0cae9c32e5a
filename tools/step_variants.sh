#!/bin/bash
# Profiling tool (not product): build cost-ablation variants of libquadenv.so for
# tools/step_variants.py -- the physics run twice / skipped, the observation (scipy Euler) skipped,
# the auto-reset branch compiled out (k_step_h), the SLP vectorizer on. Output: tools/_build/abl_*.so
# The -D variants are the product build (csrc/Makefile, its flags) with one -D, each in its own object directory.
set -e
cd "$(dirname "$0")/../uav_reinforcement_learning_control_amd/csrc"
make -s
B=../../tools/_build
for v in PHYS2 NOPHYS NOOBS NORESET; do
  make -s -j8 OUT=$B/abl_$v/libquadenv.so DEFS=-DQD_ABL_$v
  cp $B/abl_$v/libquadenv.so $B/abl_$v.so
done
# the product source WITH the SLP vectorizer (v_pk_* f32 packing; csrc/Makefile turns it off): its own compile
# line, the other objects from the in-tree build
mkdir -p $B/obj
F="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-function -ffp-contract=on -mllvm -amdgpu-kernarg-preload-count=16"
O=../_lib/obj
/opt/rocm/bin/hipcc $F -I$O -c -o $B/obj/quadenv_SLP.o quadenv.hip
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $B/abl_SLP.so \
  $B/obj/quadenv_SLP.o $O/policy.o $O/rollout.o $O/learner.o $O/learner_x3.o
