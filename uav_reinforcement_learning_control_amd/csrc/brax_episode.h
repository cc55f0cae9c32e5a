// brax_episode.h -- the flattened arguments of the Brax-profile policy's fused launches and the launchers their
// per-(kind, MB) objects export to quad_brax_episode / quad_brax_unroll (brax_actor.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/quadenv.h"
#include "env_tiles.h"
#include "policy_episode.h"  // ActorNet

namespace quadenv {

struct BraxEpisodeArgs {  // QuadBraxRun, flattened (trace_envs 0 when no trace is requested)
  int32_t max_steps, trace_envs, deterministic;
  uint32_t noise_step0;
  uint64_t seed;
  QuadBraxMetrics metrics;
  float *trace_actions, *trace_obs, *trace_pos, *trace_target;
};
struct BraxUnrollArgs {  // QuadBraxUnroll, flattened
  float *obs, *raw, *log_prob, *reward, *discount, *truncation, *next_obs, *ep_ret;
  double* stats;
  int32_t steps, unroll_length;
  uint32_t noise_step0;
  uint64_t seed;
};

// one (kind, MB) object's instantiation, defined and explicitly instantiated in that object: k_brax_episode
// (brax_actor.hip) and k_brax_unroll (brax_unroll.hip) over all envs of kp, 64-env blocks of two one-tile waves
template <int BKIND, int MB>
hipError_t launch_brax_inst(const KConsts<float>* kc, const KParams& kp, const ActorNet& net, const float* packed,
                            const BraxEpisodeArgs& a, hipStream_t s);
template <int BKIND, int MB>
hipError_t launch_brax_unroll_inst(const KConsts<float>* kc, const KParams& kp, const ActorNet& net, const float* packed,
                                   const BraxUnrollArgs& a, hipStream_t s);

}  // namespace quadenv
