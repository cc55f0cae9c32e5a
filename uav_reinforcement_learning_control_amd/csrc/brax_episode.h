// brax_episode.h -- host-side entries of the Brax-profile policy's launches (brax_actor.hip), called by
// quad_brax_episode and quad_brax_unroll (quadenv.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/quadenv.h"
#include "env_tiles.h"
#include "policy_episode.h"  // ActorNet

namespace quadenv {

// QUAD_OK and *out, or QUAD_EINVAL with a message for an arch outside the family
int brax_net_of(const QuadBraxActorArch* a, ActorNet* out);
struct BraxEpisodeArgs {  // QuadBraxRun, flattened (trace_envs 0 when no trace is requested)
  int32_t max_steps, trace_envs, deterministic;
  uint32_t noise_step0;
  uint64_t seed;
  QuadBraxMetrics metrics;
  float *trace_actions, *trace_obs, *trace_pos, *trace_target;
};
// k_brax_episode<env_kind, mb> over all envs of kp, 64-env blocks of two one-tile waves
hipError_t launch_brax_episode(const KConsts<float>* kc, const KParams& kp, int env_kind, const ActorNet& net,
                               const float* packed, const BraxEpisodeArgs& a, hipStream_t s);

struct BraxUnrollArgs {  // QuadBraxUnroll, flattened
  float *obs, *raw, *log_prob, *reward, *discount, *truncation, *next_obs, *ep_ret;
  double* stats;
  int32_t steps, unroll_length;
  uint32_t noise_step0;
  uint64_t seed;
};
// k_brax_unroll<env_kind, mb> (brax_unroll.hip) over all envs of kp, the episode kernel's block shape
hipError_t launch_brax_unroll(const KConsts<float>* kc, const KParams& kp, int env_kind, const ActorNet& net,
                              const float* packed, const BraxUnrollArgs& a, hipStream_t s);

}  // namespace quadenv
