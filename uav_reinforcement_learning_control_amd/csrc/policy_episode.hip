// policy_episode.hip -- the trained policy's whole-episode evaluation in ONE launch
// (quad_policy_episode), and the deployed observation law alone (quad_deploy_obs).
//
// Kernels
//   k_deploy_obs, k_deploy_obs_rows            vel_est_update + deploy_obs (quad_deploy.h) over [n,12]: one timestamp,
//                                              or one timestamp and one code (skip / update / empty first) per row
//                                              states, caller-owned [8][n] estimator block
//   k_policy_episode<KIND, CTBR, NT, SPEC, MODE, EB>
//                                              the fused closed loop: k_rollout's block shape and
//                                              env-to-lane mapping (rollout.hip) with k_ctrl_episode's
//                                              freeze-at-done loop (ctrl.hip) -- actor only,
//                                              deterministic, no auto-reset, no buffer rows
//
// Per step: observation (the env's, or the deployed one: MODE) -> X^T fragments -> actor MLP on MFMA ->
// clip(mean) -> env_step -> pid_acc_step -> estimator update -> estimator error -> traces. Each env's
// state, estimator, metric accumulators and observation stay in registers for the whole episode; the
// packed actor is staged into LDS once. One store at the end.
//
// The loop itself (episode_body) lives in policy_episode_body.h with the forward as a template parameter, so the
// general actor's kernels (actor_arch.hip) compile the same body; Net128Forward below is this file's forward.
//
// Two rules hold this kernel together:
//   * A frozen env's lane keeps feeding its column of the wave's MFMA tile(s): every MFMA and
//     permlane32_swap (fragments, net_forward) runs with the full wave outside any per-lane branch; only
//     the per-lane updates sit under `if (run)`.
//   * A wave leaves the loop when none of its lanes runs, and the waves of a block leave at different
//     steps, so after the staging barriers the loop holds no block-wide barrier.
//
// k_policy_waypoints is the same body with the waypoint tracker (quad_waypoints.h) after every committed step
// (WP): hover kind, the tracker's status ends an env's run, the deployed observation is rebuilt with the
// target the tracker has just written (quad_policy_waypoints).
//
// This file is compiled once per env kind (-DPE_KIND=0 hover / 1 trajectory) and once more for the hover
// kind's waypoint instantiations (-DPE_KIND=2): the three objects build in parallel, each with its own
// instantiations. The hover object (PE_KIND=0) also holds the family's host code: the block-shape rule, the
// argument checks and the C entry points quad_deploy_obs, quad_policy_episode and quad_policy_waypoints.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <string>

#include "../../include/quadenv.h"
#include "dispatch.h"
#include "env_tiles.h"
#include "handle.h"
#include "kconsts_default.h"
#include "policy_episode.h"
#include "policy_episode_body.h"
#include "policy_net.h"
#include "population.h"
#include "quad_deploy.h"
#include "quad_physics.h"
#include "quad_pid.h"
#include "quad_waypoints.h"

#ifndef PE_KIND
#error "compile with -DPE_KIND=0 (hover), 1 (trajectory) or 2 (hover, waypoint laps)"
#endif
#define PE_WP (PE_KIND == 2)

namespace quadenv {

#if !PE_WP
// one env kind's instantiations (this translation unit's)
template <int KIND>
hipError_t launch_episode_kind(const KConsts<float>* kc, const KParams& kp, bool ctbr, bool spec, int obs_mode,
                               int nt, int eb, const float* packed, const EpisodeArgs& a, hipStream_t s);
template <int KIND>
hipError_t launch_pop_episode_kind(const KConsts<float>* kc, const PopEpisodeEntry* tab, const int32_t* active,
                                   int count, int n, bool ctbr, bool spec, int nt, int eb, hipStream_t s);
#if PE_KIND == 0
template <>
hipError_t launch_pop_episode_kind<QUAD_ENV_TRAJ>(const KConsts<float>* kc, const PopEpisodeEntry* tab,
                                                  const int32_t* active, int count, int n, bool ctbr, bool spec,
                                                  int nt, int eb, hipStream_t s);
template <>  // the trajectory kind's: the other object of this file
hipError_t launch_episode_kind<QUAD_ENV_TRAJ>(const KConsts<float>* kc, const KParams& kp, bool ctbr, bool spec,
                                              int obs_mode, int nt, int eb, const float* packed, const EpisodeArgs& a,
                                              hipStream_t s);
#endif
#endif

namespace {

// the 12-128-128-4 ReLU actor of policy_net.h as episode_body's forward (policy_episode_body.h): the packed image
// in LDS with the actor's W2 pieces, net_forward<ACT, NT>'s bits, k_policy_act's deterministic sample
template <int NT>
struct Net128Forward {
  const float* __restrict__ packed;
  float sd[ACT];
  template <int BLK>
  __device__ __forceinline__ void stage() {
    extern __shared__ float lds[];
    stage_lds<BLK>(lds, packed);
    stage_pieces<BLK>(lds, packed);  // the actor's W2 pieces; the critic's image rides along and is never evaluated
    const float* log_std = packed + LDS_F;
#pragma unroll
    for (int k = 0; k < ACT; k++) sd[k] = expf(log_std[k]);
  }
  __device__ __forceinline__ void operator()(const float (&ob)[12], float (&act)[ACT]) const {
    extern __shared__ float lds[];
    const bool h = (threadIdx.x & 32) != 0;
    float xb[NT][8], mean[NT][ACT];
    fragments<NT>(ob, xb);
    {
      P3 xp[NT];
#pragma unroll
      for (int j = 0; j < NT; j++) xp[j] = split8(xb[j]);
      const NetOff o = net_off(0, packed, 0);
      Pipe<NT> st;
      pipe_start<NT, true>(lds, o, xp, st);  // net_forward<ACT, NT> with the W2 pieces from LDS: the same bits
      net_core<ACT, NT, false, 0, true>(lds, o, o, xp, st, mean);
    }
#pragma unroll
    for (int k = 0; k < ACT; k++) {
      const float mk = (NT == 2 && h) ? mean[NT - 1][k] : mean[0][k];
      act[k] = mk + sd[k] * 0.f;  // k_policy_act's sample with deterministic = 1 (z = 0)
    }
  }
};


// SPEC: the handle's constant block is the reference default (kconsts_default.h): immediates
template <int KIND, bool CTBR, int NT, bool SPEC, int MODE, int EB>
__global__ __launch_bounds__(EB * 2 / NT) void k_policy_episode(const KConsts<float>* __restrict__ kc, KParams p,
                                                                const float* __restrict__ packed, EpisodeArgs a) {
  p.kc = kc;  // noalias: constant-block loads stay scalar after the stores (see KParams)
  Net128Forward<NT> fw{packed};
  if constexpr (SPEC) {
    constexpr KConsts<float> K = kdef_block<KIND, CTBR>();
    episode_body<KIND, CTBR, NT, MODE, EB, false>(K, p, fw, a, nullptr);
  } else {
    episode_body<KIND, CTBR, NT, MODE, EB, false>(*kc, p, fw, a, nullptr);
  }
}

#if !PE_WP
// The population form (quad_pop_episode); the member's entry is read through pop::const_entry (population.h).
template <int KIND, bool CTBR, int NT, bool SPEC, int EB>
__global__ __launch_bounds__(EB * 2 / NT) void k_pop_policy_episode(const KConsts<float>* __restrict__ kc,
                                                                    const PopEpisodeEntry* __restrict__ tab,
                                                                    const int32_t* __restrict__ active) {
#if defined(__HIP_DEVICE_COMPILE__)  // (pop::const_entry, population.h)
  const auto& en = pop::const_entry(tab, active[blockIdx.y]);
  KParams p = en.kp;
  p.kc = kc;
  const EpisodeArgs a = en.a;
  const float* __restrict__ packed = en.packed;
  Net128Forward<NT> fw{packed};
  if constexpr (SPEC) {
    constexpr KConsts<float> K = kdef_block<KIND, CTBR>();
    episode_body<KIND, CTBR, NT, QUAD_OBS_ENV, EB, false>(K, p, fw, a, nullptr);
  } else {
    episode_body<KIND, CTBR, NT, QUAD_OBS_ENV, EB, false>(*kc, p, fw, a, nullptr);
  }
#endif
}

template <int KIND, bool CTBR, int NT, bool SPEC, int EB>
hipError_t launch_pop(const KConsts<float>* kc, const PopEpisodeEntry* tab, const int32_t* active, int count, int n,
                      hipStream_t s) {
  return launch_lds<&k_pop_policy_episode<KIND, CTBR, NT, SPEC, EB>>(dim3((n + EB - 1) / EB, count), dim3(EB * 2 / NT),
                                                                     LDS_F * int(sizeof(float)), s, kc, tab, active);
}
#endif

#if PE_WP
// the WP form of k_policy_episode: hover kind only (a switch overwrites the target register), the tracker's
// tables and rows in a kernel argument of its own so k_policy_episode's arguments stay as they are
template <bool CTBR, int NT, bool SPEC, int MODE, int EB>
__global__ __launch_bounds__(EB * 2 / NT) void k_policy_waypoints(const KConsts<float>* __restrict__ kc, KParams p,
                                                                  const float* __restrict__ packed, EpisodeArgs a,
                                                                  QuadWaypointRun wr) {
  p.kc = kc;
  Net128Forward<NT> fw{packed};
  if constexpr (SPEC) {
    constexpr KConsts<float> K = kdef_block<QUAD_ENV_HOVER, CTBR>();
    episode_body<QUAD_ENV_HOVER, CTBR, NT, MODE, EB, true>(K, p, fw, a, &wr);
  } else {
    episode_body<QUAD_ENV_HOVER, CTBR, NT, MODE, EB, true>(*kc, p, fw, a, &wr);
  }
}

template <bool CTBR, int NT, bool SPEC, int MODE, int EB>
hipError_t launch_wp(const KConsts<float>* kc, const KParams& kp, const float* packed, const EpisodeArgs& a,
                     const QuadWaypointRun& wr, hipStream_t s) {
  return launch_lds<&k_policy_waypoints<CTBR, NT, SPEC, MODE, EB>>(dim3((kp.n + EB - 1) / EB), dim3(EB * 2 / NT),
                                                                   LDS_F * int(sizeof(float)), s, kc, kp, packed, a, wr);
}
#else
template <int KIND, bool CTBR, int NT, bool SPEC, int MODE, int EB>
hipError_t launch(const KConsts<float>* kc, const KParams& kp, const float* packed, const EpisodeArgs& a,
                  hipStream_t s) {
  return launch_lds<&k_policy_episode<KIND, CTBR, NT, SPEC, MODE, EB>>(dim3((kp.n + EB - 1) / EB), dim3(EB * 2 / NT),
                                                                       LDS_F * int(sizeof(float)), s, kc, kp, packed, a);
}
#endif

#if PE_KIND == 0
constexpr int DEPLOY_BLOCK = 256;

// one row of quad_deploy_obs / quad_deploy_obs_rows; code: 0 skip, 1 update, 2 empty the estimator first
__device__ __forceinline__ void deploy_row(const KConsts<float>* __restrict__ kc, const EstArgs& est,
                                           const float* __restrict__ state12, const float* __restrict__ target3,
                                           double timestamp, int code, int i, int32_t n, float* __restrict__ obs,
                                           float* __restrict__ vel_est) {
  if (code == 0) return;
  float s[12], tg[3];
#pragma unroll
  for (int j = 0; j < 12; j++) s[j] = state12[size_t(i) * 12 + j];
#pragma unroll
  for (int j = 0; j < 3; j++) tg[j] = target3[size_t(i) * 3 + j];
  double st[EST_NSTATE], vel[3];
#pragma unroll
  for (int j = 0; j < EST_NSTATE; j++) st[j] = code == 2 ? 0.0 : est.state[size_t(j) * size_t(n) + size_t(i)];
  vel_est_update(est.alpha ? est.alpha[i] : est.alpha_all, est.max_dt, s, timestamp, st, vel);
#pragma unroll
  for (int j = 0; j < EST_NSTATE; j++) est.state[size_t(j) * size_t(n) + size_t(i)] = st[j];
  float o[12];
  deploy_obs(kc->obs_lo, kc->obs_span, kc->obs_rspan, s, tg, vel, o);
#pragma unroll
  for (int j = 0; j < 12; j++) obs[size_t(i) * 12 + j] = o[j];
  if (vel_est) {
#pragma unroll
    for (int j = 0; j < 3; j++) vel_est[size_t(i) * 3 + j] = float(vel[j]);
  }
}

__global__ __launch_bounds__(DEPLOY_BLOCK) void k_deploy_obs(const KConsts<float>* __restrict__ kc, EstArgs est,
                                                             const float* __restrict__ state12,
                                                             const float* __restrict__ target3, double timestamp,
                                                             int32_t n, float* __restrict__ obs,
                                                             float* __restrict__ vel_est) {
  const int i = blockIdx.x * DEPLOY_BLOCK + threadIdx.x;
  if (i >= n) return;
  deploy_row(kc, est, state12, target3, timestamp, 1, i, n, obs, vel_est);
}

__global__ __launch_bounds__(DEPLOY_BLOCK) void k_deploy_obs_rows(const KConsts<float>* __restrict__ kc, EstArgs est,
                                                                  const float* __restrict__ state12,
                                                                  const float* __restrict__ target3,
                                                                  const double* __restrict__ timestamps,
                                                                  const uint8_t* __restrict__ rows, int32_t n,
                                                                  float* __restrict__ obs, float* __restrict__ vel_est) {
  const int i = blockIdx.x * DEPLOY_BLOCK + threadIdx.x;
  if (i >= n) return;
  deploy_row(kc, est, state12, target3, timestamps[i], rows ? int(rows[i]) : 1, i, n, obs, vel_est);
}
#endif

}  // namespace

#if PE_WP
// quad_policy_waypoints' launch: quad_policy_episode's block-shape rule (below, in the hover object)
hipError_t launch_policy_waypoints(const KConsts<float>* kc, const KParams& kp, bool ctbr, bool spec, int obs_mode,
                                   const float* packed, const EpisodeArgs& a, const QuadWaypointRun& wr,
                                   hipStream_t s) {
  int nt, eb;
  episode_block_shape(kp.n, nt, eb);
  return with_bool(ctbr, [&](auto cb) {
    return with_bool(spec, [&](auto sp) {
      return with_bool(obs_mode == QUAD_OBS_DEPLOYED, [&](auto dm) {
        constexpr bool CB = decltype(cb)::value, SP = decltype(sp)::value;
        constexpr int MD = decltype(dm)::value ? QUAD_OBS_DEPLOYED : QUAD_OBS_ENV;
        if (nt == 1) return launch_wp<CB, 1, SP, MD, 64>(kc, kp, packed, a, wr, s);
        return eb == 64 ? launch_wp<CB, 2, SP, MD, 64>(kc, kp, packed, a, wr, s)
                        : launch_wp<CB, 2, SP, MD, 256>(kc, kp, packed, a, wr, s);
      });
    });
  });
}
#else
template <>
hipError_t launch_episode_kind<PE_KIND>(const KConsts<float>* kc, const KParams& kp, bool ctbr, bool spec, int obs_mode,
                                        int nt, int eb, const float* packed, const EpisodeArgs& a, hipStream_t s) {
  return with_bool(ctbr, [&](auto cb) {
    return with_bool(spec, [&](auto sp) {
      return with_bool(obs_mode == QUAD_OBS_DEPLOYED, [&](auto dm) {
        constexpr int KD = PE_KIND;
        constexpr bool CB = decltype(cb)::value, SP = decltype(sp)::value;
        constexpr int MD = decltype(dm)::value ? QUAD_OBS_DEPLOYED : QUAD_OBS_ENV;
        // one-tile waves only in 64-env blocks: eight of them per 256-env block would share a SIMD in pairs,
        // 256 registers each, and spill (650-860 bytes of scratch per lane)
        if (nt == 1) return launch<KD, CB, 1, SP, MD, 64>(kc, kp, packed, a, s);
        return eb == 64 ? launch<KD, CB, 2, SP, MD, 64>(kc, kp, packed, a, s)
                        : launch<KD, CB, 2, SP, MD, 256>(kc, kp, packed, a, s);
      });
    });
  });
}
#endif

#if !PE_WP
template <>
hipError_t launch_pop_episode_kind<PE_KIND>(const KConsts<float>* kc, const PopEpisodeEntry* tab, const int32_t* active,
                                            int count, int n, bool ctbr, bool spec, int nt, int eb, hipStream_t s) {
  return with_bool(ctbr, [&](auto cb) {
    return with_bool(spec, [&](auto sp) {
      constexpr int KD = PE_KIND;
      constexpr bool CB = decltype(cb)::value, SP = decltype(sp)::value;
      if (nt == 1) return launch_pop<KD, CB, 1, SP, 64>(kc, tab, active, count, n, s);  // (launch_episode_kind's rule)
      return eb == 64 ? launch_pop<KD, CB, 2, SP, 64>(kc, tab, active, count, n, s)
                      : launch_pop<KD, CB, 2, SP, 256>(kc, tab, active, count, n, s);
    });
  });
}
#endif

#if PE_KIND == 0
// The block shape: an evaluation batch (5 .. ~1,000 envs) in 64-env blocks of two one-tile waves (NT = 1),
// so it spreads over 4x the CUs of k_rollout's shape and each wave's MFMA chain is one tile long; from
// EPISODE_WIDE_N envs k_rollout's 256-env blocks of two-tile waves (the measurements: DESIGN 16). Every form
// computes the same bits. QUADENV_ROLLOUT_NT = 1 / 2 and QUADENV_EPISODE_BLOCK = 64 / 256 pin them (A/B, tests);
// NT = 1 always takes 64-env blocks (launch_episode_kind).
constexpr int EPISODE_WIDE_N = 16384;
void episode_block_shape(int32_t n, int& nt, int& eb) {
  const bool wide = n > EPISODE_WIDE_N;
  const char* v = std::getenv("QUADENV_ROLLOUT_NT");
  nt = v && std::atoi(v) == 1 ? 1 : (v && std::atoi(v) == 2 ? 2 : (wide ? 2 : 1));
  const char* b = std::getenv("QUADENV_EPISODE_BLOCK");
  eb = b && std::atoi(b) == 64 ? 64 : (b && std::atoi(b) == 256 ? 256 : (wide ? 256 : 64));
}
hipError_t launch_pop_policy_episode(const KConsts<float>* kc, const PopEpisodeEntry* tab, const int32_t* active,
                                     int count, int n, int env_kind, bool ctbr, bool spec, hipStream_t s) {
  int nt, eb;
  episode_block_shape(n, nt, eb);
  return env_kind == QUAD_ENV_TRAJ
             ? launch_pop_episode_kind<QUAD_ENV_TRAJ>(kc, tab, active, count, n, ctbr, spec, nt, eb, s)
             : launch_pop_episode_kind<QUAD_ENV_HOVER>(kc, tab, active, count, n, ctbr, spec, nt, eb, s);
}

// quad_policy_episode's argument checks and its flattened arguments (also quad_actor_episode's and
// quad_pop_attach_eval's)
int pop::episode_args(const QuadHandle* h, const float* packed, const QuadPolicyRun* r, EpisodeArgs* out,
                      const char* who) {
  if (!h || !packed || !r) return fail(QUAD_EINVAL, "handle/packed/run is NULL");
  if (h->cfg.env_kind != QUAD_ENV_HOVER && h->cfg.env_kind != QUAD_ENV_TRAJ)
    return fail(QUAD_EINVAL, std::string(who) + ": env_kind must be HOVER or TRAJ");
  return policy_run_args(h, packed, r, false, out, who);
}

// quad_policy_waypoints' argument checks and its flattened arguments (also quad_actor_waypoints')
int waypoints_args(const QuadHandle* h, const float* packed, const QuadPolicyRun* r, const QuadWaypointRun* wr,
                   EpisodeArgs* out, const char* who) {
  if (!h || !packed || !r || !wr) return fail(QUAD_EINVAL, "handle/packed/run/waypoints is NULL");
  if (int rc = check_waypoint_run(h, who, wr)) return rc;
  return policy_run_args(h, packed, r, wr->trace_reward || wr->trace_wp_idx, out, who);
}
#endif

}  // namespace quadenv

#if PE_KIND == 0
using namespace quadenv;

extern "C" {

// quad_deploy_obs' and quad_deploy_obs_rows' argument checks
static int deploy_obs_args(const QuadHandle* h, const QuadVelEst* est, const float* state12, const float* target3,
                           int32_t n, const float* obs, const char* who) {
  const std::string w(who);
  if (!h || !est) return fail(QUAD_EINVAL, "handle/est is NULL");
  if (h->cfg.env_kind != QUAD_ENV_HOVER && h->cfg.env_kind != QUAD_ENV_TRAJ)
    return fail(QUAD_EINVAL, w + ": env_kind must be HOVER or TRAJ");
  if (int rc = check_est(est, who)) return rc;
  if (!est->state) return fail(QUAD_EINVAL, w + ": the estimator state block is required");
  if (!state12 || !target3 || !obs) return fail(QUAD_EINVAL, w + ": state12, target3 and obs are required");
  if (n < 1) return fail(QUAD_EINVAL, w + ": n must be >= 1");
  return QUAD_OK;
}

int quad_deploy_obs(QuadHandle* h, const QuadVelEst* est, const float* state12, const float* target3,
                    double timestamp, int32_t n, float* obs, float* vel_est, void* stream) {
  if (int rc = deploy_obs_args(h, est, state12, target3, n, obs, "quad_deploy_obs")) return rc;
  DeviceGuard g(h->device);
  hipLaunchKernelGGL(k_deploy_obs, dim3((n + DEPLOY_BLOCK - 1) / DEPLOY_BLOCK), dim3(DEPLOY_BLOCK), 0,
                     static_cast<hipStream_t>(stream), h->kdev, EstArgs{est->alpha, est->alpha_all, est->max_dt, est->state},
                     state12, target3, timestamp, n, obs, vel_est);
  HIP_TRY(hipGetLastError());
  return QUAD_OK;
}

int quad_deploy_obs_rows(QuadHandle* h, const QuadVelEst* est, const float* state12, const float* target3,
                         const double* timestamps, const uint8_t* rows, int32_t n, float* obs, float* vel_est,
                         void* stream) {
  if (int rc = deploy_obs_args(h, est, state12, target3, n, obs, "quad_deploy_obs_rows")) return rc;
  if (!timestamps) return fail(QUAD_EINVAL, "quad_deploy_obs_rows: timestamps is required");
  DeviceGuard g(h->device);
  hipLaunchKernelGGL(k_deploy_obs_rows, dim3((n + DEPLOY_BLOCK - 1) / DEPLOY_BLOCK), dim3(DEPLOY_BLOCK), 0,
                     static_cast<hipStream_t>(stream), h->kdev, EstArgs{est->alpha, est->alpha_all, est->max_dt, est->state},
                     state12, target3, timestamps, rows, n, obs, vel_est);
  HIP_TRY(hipGetLastError());
  return QUAD_OK;
}

int quad_policy_episode(QuadHandle* h, const float* packed, const QuadPolicyRun* r, void* stream) {
  EpisodeArgs a{};
  if (int rc = pop::episode_args(h, packed, r, &a)) return rc;
  DeviceGuard g(h->device);
  int nt, eb;
  episode_block_shape(h->n, nt, eb);
  const bool ctbr = h->cfg.wrapper == QUAD_WRAP_CTBR;
  hipStream_t s = static_cast<hipStream_t>(stream);
  HIP_TRY(h->cfg.env_kind == QUAD_ENV_TRAJ
              ? launch_episode_kind<QUAD_ENV_TRAJ>(h->kdev, h->kp, ctbr, h->spec, r->obs_mode, nt, eb, packed, a, s)
              : launch_episode_kind<QUAD_ENV_HOVER>(h->kdev, h->kp, ctbr, h->spec, r->obs_mode, nt, eb, packed, a, s));
  return QUAD_OK;
}

int quad_policy_waypoints(QuadHandle* h, const float* packed, const QuadPolicyRun* r, const QuadWaypointRun* wr,
                          void* stream) {
  EpisodeArgs a{};
  if (int rc = waypoints_args(h, packed, r, wr, &a, "quad_policy_waypoints")) return rc;
  DeviceGuard g(h->device);
  HIP_TRY(launch_policy_waypoints(h->kdev, h->kp, h->cfg.wrapper == QUAD_WRAP_CTBR, h->spec, r->obs_mode, packed, a, *wr,
                                  static_cast<hipStream_t>(stream)));
  return QUAD_OK;
}

}  // extern "C"
#endif
