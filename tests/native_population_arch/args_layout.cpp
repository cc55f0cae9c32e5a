// TEST INFRASTRUCTURE ONLY: prints the host layout of lrna::Args (csrc/learner_arch.h), the entry of the general
// learner's population gradient table (csrc/population.h), for tests/test_population_arch_cpu.py to pin.
#include <cstddef>
#include <cstdio>

#include "../../uav_reinforcement_learning_control_amd/csrc/learner_arch.h"

using quadenv::lrna::Args;

int main() {
  std::printf("sizeof %zu\n", sizeof(Args));
#define OFF(f) std::printf(#f " %zu\n", offsetof(Args, f))
  OFF(g);
  OFF(g.idx);
  OFF(g.adv_part);
  OFF(g.batch);
  OFF(gr);
  OFF(stats);
  OFF(x);
  OFF(h1);
  OFF(dh2);
  OFF(dh1);
  OFF(sp);
  OFF(pb);
  OFF(h1w);
  OFF(rps);
  OFF(ent_coef);
  return 0;
}
