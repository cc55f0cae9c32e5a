// policy_episode.h -- host-side entries of the deployed-observation law and the fused policy episode
// (policy_episode.hip), called by quad_deploy_obs and quad_policy_episode.
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

// k_deploy_obs over n rows (the observation bounds are the handle's constant block kc)
hipError_t launch_deploy_obs(const KConsts<float>* kc, const EstArgs& est, const float* state12, const float* target3,
                             double timestamp, int32_t n, float* obs, float* vel_est, hipStream_t s);

// k_policy_episode<env_kind, ctbr, ., spec, obs_mode> over all envs of kp; the block shape is chosen here
hipError_t launch_policy_episode(const KConsts<float>* kc, const KParams& kp, int env_kind, bool ctbr, bool spec,
                                 int obs_mode, const float* packed, const EpisodeArgs& a, hipStream_t s);

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

// ---- the general actor's forms (actor_arch.hip; quad_actor_episode / quad_actor_waypoints): the same closed loop
// with actor_arch.h's forward, in 64-env blocks of two one-tile waves, the constant block read from memory
struct ActorNet {  // a checked QuadActorArch or QuadBraxActorArch: H1 / 32, H2 / 32 (2, 4 or 8), QUAD_ACTFN_*
  int nb1, mb, actfn;
};
// QUAD_OK and *out, or QUAD_EINVAL with a message for an arch outside the family
int actor_net_of(const QuadActorArch* a, ActorNet* out);
hipError_t launch_actor_episode(const KConsts<float>* kc, const KParams& kp, int env_kind, bool ctbr, int obs_mode,
                                const ActorNet& net, const float* packed, const EpisodeArgs& a, hipStream_t s);
hipError_t launch_actor_waypoints(const KConsts<float>* kc, const KParams& kp, bool ctbr, int obs_mode,
                                  const ActorNet& net, const float* packed, const EpisodeArgs& a,
                                  const QuadWaypointRun& wr, hipStream_t s);

}  // namespace quadenv
