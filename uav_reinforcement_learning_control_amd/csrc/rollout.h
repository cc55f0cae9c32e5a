// rollout.h -- the fused rollout kernel's arguments (rollout.hip), shared with the population tables (population.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "env_tiles.h"

namespace quadenv {

struct RollArgs {  // QuadRollout, flattened
  float* obs_copy;
  float* actions;
  float* log_prob;
  float* value;
  float* starts;
  float* rewards;
  float* last_obs;
  float* last_start;
  float* ep_ret;
  float* ep_len;
  double* stats;
  uint32_t rows;
  uint32_t t0;
  int32_t steps;
  int32_t deterministic;
  uint64_t seed;
  float gamma;
};

}  // namespace quadenv
