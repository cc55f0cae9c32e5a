// policy_episode.h -- the fused policy episode's arguments (policy_episode.hip) and what crosses between its
// three objects, to the general actor's entry points (actor_arch.hip) and to the population (population.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/quadenv.h"
#include "env_tiles.h"

namespace quadenv {

struct EstArgs {  // QuadVelEst, flattened
  const double* alpha;
  double alpha_all, max_dt;
  double* state;
};

struct EpisodeArgs {  // QuadPolicyRun, flattened
  int32_t max_steps, trace_envs;
  EstArgs est;
  double est_dt;
  float *trace_actions, *trace_state12, *trace_obs, *trace_vel_est;
  QuadPidMetrics metrics;
  double* vel_err_sq;
};

// The population form (population.h, quad_pop_episode): k_policy_episode's arguments per member, env-observation
// mode; block (b, k) is block b of member active[k]'s episodes. kc: the constant block every member shares.
struct PopEpisodeEntry {
  KParams kp;
  const float* packed;
  EpisodeArgs a;
};
hipError_t launch_pop_policy_episode(const KConsts<float>* kc, const PopEpisodeEntry* tab, const int32_t* active,
                                     int count, int n, int env_kind, bool ctbr, bool spec, hipStream_t s);

// the block shape of both fused policy launches for n envs: tiles per wave (1 / 2), envs per block (64 / 256)
void episode_block_shape(int32_t n, int& nt, int& eb);

// k_policy_waypoints<ctbr, ., spec, obs_mode> over all envs of kp (hover kind)
hipError_t launch_policy_waypoints(const KConsts<float>* kc, const KParams& kp, bool ctbr, bool spec, int obs_mode,
                                   const float* packed, const EpisodeArgs& a, const QuadWaypointRun& wr,
                                   hipStream_t s);

// a checked QuadActorArch or QuadBraxActorArch (actor_core.h net_of): H1 / 32, H2 / 32 (2, 4 or 8), QUAD_ACTFN_*
struct ActorNet {
  int nb1, mb, actfn;
};

}  // namespace quadenv
