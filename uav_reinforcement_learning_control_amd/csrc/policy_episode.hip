// policy_episode.hip -- the trained policy's whole-episode evaluation in ONE launch
// (quad_policy_episode), and the deployed observation law alone (quad_deploy_obs).
//
// Kernels
//   k_deploy_obs                               vel_est_update + deploy_obs (quad_deploy.h) over [n,12]
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
// instantiations.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>

#include "../../include/quadenv.h"
#include "dispatch.h"
#include "env_tiles.h"
#include "kconsts_default.h"
#include "policy_episode.h"
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

// k_pid_episode's store (pid.hip), for the same QuadPidMetrics layout
__device__ __forceinline__ void store_metrics(const QuadPidMetrics& o, int i, const PidAcc& m, int32_t status) {
  o.steps[i] = m.steps;
  o.status[i] = status;
  o.total_reward[i] = m.total_reward;
  o.pos_err_sum[i] = m.pe_sum;
  o.pos_err_sq[i] = m.pe_sq;
  o.pos_err_max[i] = m.pe_max;
  o.yaw_rate_abs_sum[i] = m.yr_abs_sum;
  o.yaw_rate_sum[i] = m.yr_sum;
  o.yaw_rate_sq[i] = m.yr_sq;
  o.yaw_rate_abs_max[i] = m.yr_abs_max;
  o.yaw_rate_sign_changes[i] = m.sign_changes;
  o.yaw_rate_delta_sum[i] = m.yr_delta;
}

__device__ __forceinline__ void store_row12(float* base, uint32_t row, const float v[12]) {
#pragma unroll
  for (int j = 0; j < 3; j++)
    sto(reinterpret_cast<float4*>(base), 48u * row + 16u * j, make_float4(v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]));
}

// NT = 2: wave w of a block owns envs 64w .. 64w + 63 = its two MFMA tiles. NT = 1: wave w owns the 32
// envs 32w .. 32w + 31; lanes l and l + 32 both carry env l & 31 (the same bits), the lower half stores.
// EB: envs per block (256: k_rollout's shape; 64: one or two waves, for evaluation-sized batches).
// the metric status of a tracker status: lap -> QUAD_PID_LAP, terminated / truncated -> their codes
__device__ __forceinline__ int32_t metric_status_of(int32_t tracker_status) {
  return tracker_status == 1 ? QUAD_PID_LAP
                             : (tracker_status == 2 ? QUAD_PID_TERMINATED
                                                    : (tracker_status == 3 ? QUAD_PID_TRUNCATED : QUAD_PID_RUNNING));
}

// WP: the waypoint tracker runs after every committed step and ends the env's run (wr: the kernel's
// QuadWaypointRun; never read otherwise)
template <int KIND, bool CTBR, int NT, int MODE, int EB, bool WP>
__device__ __forceinline__ void episode_body(const KConsts<float>& K, const KParams& p, const float* __restrict__ packed,
                                             const EpisodeArgs& a, const QuadWaypointRun* wr) {
  constexpr int BLK = EB * 2 / NT;
  extern __shared__ float lds[];
  const int w = threadIdx.x >> 6;
  const bool h = (threadIdx.x & 32) != 0;
  const int i_raw = blockIdx.x * EB + (NT == 2 ? int(threadIdx.x) : w * 32 + int(threadIdx.x & 31));
  const bool ok = i_raw < p.n;
  const bool owner = ok && (NT == 2 || !h);  // the lane that stores this env's outputs
  // lanes past the last env shadow it (in-range loads, MFMA columns of their own) and store nothing
  const int i = ok ? i_raw : p.n - 1;
  const size_t n = size_t(p.n);

  // ---- setup, once: env, actor image, first observation, first estimator sample
  EnvRegs<float> e;
  load_env(p, i, e, CTBR);
  const uint32_t ep = Tiles(p).ldu(F_EP, env_off(uint32_t(i)));
  const double alpha = a.est.alpha ? a.est.alpha[i] : a.est.alpha_all;
  double est[EST_NSTATE];
#pragma unroll
  for (int j = 0; j < EST_NSTATE; j++) est[j] = a.est.state ? a.est.state[size_t(j) * n + size_t(i)] : 0.0;
  stage_lds<BLK>(lds, packed);
  stage_pieces<BLK>(lds, packed);  // the actor's W2 pieces; the critic's image rides along and is never evaluated
  const float* log_std = packed + LDS_F;
  float sd[ACT];
#pragma unroll
  for (int k = 0; k < ACT; k++) sd[k] = expf(log_std[k]);
  float ob[12], s12[12], ti[9];
  observe(K, e, ob, s12);  // what quad_observe reports
  target_info_of<KIND>(K, p, i, e, ep, ti);
  double vel[3];
  WpTrack tk = {};
  const double* wp = nullptr;
  int cnt = 1;
  int32_t status = QUAD_PID_RUNNING;
  bool run = true;
  if constexpr (WP) {
    tk = load_track(wr->s, i);
    const int ws = wr->w.set_of ? wr->w.set_of[i] : 0;
    cnt = wr->w.counts[ws];
    wp = wr->w.points + size_t(ws) * wr->w.max_points * 3;
    run = tk.status == 0;  // finished in an earlier run: no step, env, estimator and tracker as they are
    status = metric_status_of(tk.status);
    // a resumed run: the estimator already holds this instant's sample (a second one, dt = 0, would restart it)
    const double ts = double(e.step) * a.est_dt;
    if (run && !(est[7] != 0.0 && est[3] == ts)) {
      vel_est_update(alpha, a.est.max_dt, s12, ts, est, vel);
    } else {
#pragma unroll
      for (int j = 0; j < 3; j++) vel[j] = est[4 + j];
    }
  } else {
    vel_est_update(alpha, a.est.max_dt, s12, double(e.step) * a.est_dt, est, vel);
  }
  if (MODE == QUAD_OBS_DEPLOYED) deploy_obs(K.obs_lo, K.obs_span, K.obs_rspan, s12, e.target, vel, ob);

  PidAcc m;
  double verr = 0.0;
  const uint32_t M = uint32_t(a.trace_envs);
  const bool traced = owner && uint32_t(i) < M;
  for (int t = 0; t < a.max_steps; t++) {
    if (!__any(run)) break;  // wave-uniform: the whole wave leaves together
    // ---- policy: the actor on the wave's tile(s), full wave (frozen lanes feed their columns too)
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
    float ac[ACT];
#pragma unroll
    for (int k = 0; k < ACT; k++) {
      const float mk = (NT == 2 && h) ? mean[NT - 1][k] : mean[0][k];
      const float act = mk + sd[k] * 0.f;  // k_policy_act's sample with deterministic = 1 (z = 0)
      ac[k] = fminf(fmaxf(act, -1.f), 1.f);
    }
    // ---- env step on a copy; a frozen env keeps its state
    EnvRegs<float> en = e;
    StepRes r;
    env_step<float, CTBR>(K, en, ac, r);
    if (run) {
      if (traced) {
        const uint32_t row = uint32_t(t) * M + uint32_t(i);  // < 2^32 / 48: checked by quad_policy_episode
        if (a.trace_actions) sto(reinterpret_cast<float4*>(a.trace_actions), 16u * row, make_float4(ac[0], ac[1], ac[2], ac[3]));
        if (a.trace_obs) store_row12(a.trace_obs, row, ob);
      }
      const float tgt[3] = {ti[0], ti[1], ti[2]};  // the target read before the step
      e = en;
#pragma unroll
      for (int j = 0; j < 12; j++) { s12[j] = r.state12[j]; ob[j] = r.obs[j]; }
      int flown = 0;
      if constexpr (WP) {  // the env's observation above keeps the target the step was flown with
        flown = tk.wp_idx;
        float nt[3];
        if (wp_update(wp, cnt, wr->w.reach_radius, s12, r.reward, r.term, r.trunc, tk, nt)) {
#pragma unroll
          for (int j = 0; j < 3; j++) e.target[j] = nt[j];
        }
      }
      target_info_of<KIND>(K, p, i, e, ep, ti);
      pid_acc_step(m, s12, tgt, r.reward);
      vel_est_update(alpha, a.est.max_dt, s12, double(e.step) * a.est_dt, est, vel);
      {  // |v_est - v_true|^2 of the post-step sample, summed over the axes in order, float64
#pragma clang fp contract(off)
        const double d0 = vel[0] - double(s12[6]), d1 = vel[1] - double(s12[7]), d2 = vel[2] - double(s12[8]);
        verr += (d0 * d0 + d1 * d1) + d2 * d2;
      }
      if (MODE == QUAD_OBS_DEPLOYED) deploy_obs(K.obs_lo, K.obs_span, K.obs_rspan, s12, e.target, vel, ob);
      if (traced) {
        const uint32_t row = uint32_t(t) * M + uint32_t(i);
        if (a.trace_state12) store_row12(a.trace_state12, row, s12);
        if (a.trace_vel_est) {
#pragma unroll
          for (int j = 0; j < 3; j++) sto(a.trace_vel_est, 12u * row + 4u * j, float(vel[j]));
        }
        if constexpr (WP) {
          if (wr->trace_reward) sto(wr->trace_reward, 4u * row, r.reward);
          if (wr->trace_wp_idx) sto(wr->trace_wp_idx, 4u * row, int32_t(flown));
        }
      }
      if constexpr (WP) {
        if (tk.status != 0) {
          status = metric_status_of(tk.status);
          run = false;
        }
      } else if (r.term || r.trunc) {
        status = r.term ? QUAD_PID_TERMINATED : QUAD_PID_TRUNCATED;
        run = false;
      }
    }
  }

  if (owner) {
    store_env(p, i, e, CTBR);
    if (a.est.state) {
#pragma unroll
      for (int j = 0; j < EST_NSTATE; j++) a.est.state[size_t(j) * n + size_t(i)] = est[j];
    }
    store_metrics(a.metrics, i, m, status);
    if (a.vel_err_sq) a.vel_err_sq[i] = verr;
    if constexpr (WP) store_track(wr->s, i, tk);
  }
}

// SPEC: the handle's constant block is the reference default (kconsts_default.h): immediates
template <int KIND, bool CTBR, int NT, bool SPEC, int MODE, int EB>
__global__ __launch_bounds__(EB * 2 / NT) void k_policy_episode(const KConsts<float>* __restrict__ kc, KParams p,
                                                                const float* __restrict__ packed, EpisodeArgs a) {
  p.kc = kc;  // noalias: constant-block loads stay scalar after the stores (see KParams)
  if constexpr (SPEC) {
    constexpr KConsts<float> K = kdef_block<KIND, CTBR>();
    episode_body<KIND, CTBR, NT, MODE, EB, false>(K, p, packed, a, nullptr);
  } else {
    episode_body<KIND, CTBR, NT, MODE, EB, false>(*kc, p, packed, a, nullptr);
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
  if constexpr (SPEC) {
    constexpr KConsts<float> K = kdef_block<KIND, CTBR>();
    episode_body<KIND, CTBR, NT, QUAD_OBS_ENV, EB, false>(K, p, packed, a, nullptr);
  } else {
    episode_body<KIND, CTBR, NT, QUAD_OBS_ENV, EB, false>(*kc, p, packed, a, nullptr);
  }
#endif
}

template <int KIND, bool CTBR, int NT, bool SPEC, int EB>
hipError_t launch_pop(const KConsts<float>* kc, const PopEpisodeEntry* tab, const int32_t* active, int count, int n,
                      hipStream_t s) {
  static bool opted[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  const int bytes = LDS_F * int(sizeof(float));
  if (!opted[dev]) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_pop_policy_episode<KIND, CTBR, NT, SPEC, EB>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) return e;
    opted[dev] = true;
  }
  hipLaunchKernelGGL((k_pop_policy_episode<KIND, CTBR, NT, SPEC, EB>), dim3((n + EB - 1) / EB, count),
                     dim3(EB * 2 / NT), bytes, s, kc, tab, active);
  return hipGetLastError();
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
  if constexpr (SPEC) {
    constexpr KConsts<float> K = kdef_block<QUAD_ENV_HOVER, CTBR>();
    episode_body<QUAD_ENV_HOVER, CTBR, NT, MODE, EB, true>(K, p, packed, a, &wr);
  } else {
    episode_body<QUAD_ENV_HOVER, CTBR, NT, MODE, EB, true>(*kc, p, packed, a, &wr);
  }
}

template <bool CTBR, int NT, bool SPEC, int MODE, int EB>
hipError_t launch_wp(const KConsts<float>* kc, const KParams& kp, const float* packed, const EpisodeArgs& a,
                     const QuadWaypointRun& wr, hipStream_t s) {
  static bool opted[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  const int bytes = LDS_F * int(sizeof(float));
  if (!opted[dev]) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_policy_waypoints<CTBR, NT, SPEC, MODE, EB>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) return e;
    opted[dev] = true;
  }
  hipLaunchKernelGGL((k_policy_waypoints<CTBR, NT, SPEC, MODE, EB>), dim3((kp.n + EB - 1) / EB), dim3(EB * 2 / NT),
                     bytes, s, kc, kp, packed, a, wr);
  return hipGetLastError();
}
#else
template <int KIND, bool CTBR, int NT, bool SPEC, int MODE, int EB>
hipError_t launch(const KConsts<float>* kc, const KParams& kp, const float* packed, const EpisodeArgs& a,
                  hipStream_t s) {
  static bool opted[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  const int bytes = LDS_F * int(sizeof(float));
  if (!opted[dev]) {
    const hipError_t e = hipFuncSetAttribute(
        reinterpret_cast<const void*>(&k_policy_episode<KIND, CTBR, NT, SPEC, MODE, EB>),
        hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) return e;
    opted[dev] = true;
  }
  hipLaunchKernelGGL((k_policy_episode<KIND, CTBR, NT, SPEC, MODE, EB>), dim3((kp.n + EB - 1) / EB),
                     dim3(EB * 2 / NT), bytes, s, kc, kp, packed, a);
  return hipGetLastError();
}
#endif

#if PE_KIND == 0
constexpr int DEPLOY_BLOCK = 256;

__global__ __launch_bounds__(DEPLOY_BLOCK) void k_deploy_obs(const KConsts<float>* __restrict__ kc, EstArgs est,
                                                             const float* __restrict__ state12,
                                                             const float* __restrict__ target3, double timestamp,
                                                             int32_t n, float* __restrict__ obs,
                                                             float* __restrict__ vel_est) {
  const int i = blockIdx.x * DEPLOY_BLOCK + threadIdx.x;
  if (i >= n) return;
  float s[12], tg[3];
#pragma unroll
  for (int j = 0; j < 12; j++) s[j] = state12[size_t(i) * 12 + j];
#pragma unroll
  for (int j = 0; j < 3; j++) tg[j] = target3[size_t(i) * 3 + j];
  double st[EST_NSTATE], vel[3];
#pragma unroll
  for (int j = 0; j < EST_NSTATE; j++) st[j] = est.state[size_t(j) * size_t(n) + size_t(i)];
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
#endif

}  // namespace

#if PE_WP
// quad_policy_waypoints' launch: launch_policy_episode's block-shape rule (below, in the hover object)
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
hipError_t launch_deploy_obs(const KConsts<float>* kc, const EstArgs& est, const float* state12, const float* target3,
                             double timestamp, int32_t n, float* obs, float* vel_est, hipStream_t s) {
  hipLaunchKernelGGL(k_deploy_obs, dim3((n + DEPLOY_BLOCK - 1) / DEPLOY_BLOCK), dim3(DEPLOY_BLOCK), 0, s, kc, est,
                     state12, target3, timestamp, n, obs, vel_est);
  return hipGetLastError();
}

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
hipError_t launch_policy_episode(const KConsts<float>* kc, const KParams& kp, int env_kind, bool ctbr, bool spec,
                                 int obs_mode, const float* packed, const EpisodeArgs& a, hipStream_t s) {
  int nt, eb;
  episode_block_shape(kp.n, nt, eb);
  return env_kind == QUAD_ENV_TRAJ
             ? launch_episode_kind<QUAD_ENV_TRAJ>(kc, kp, ctbr, spec, obs_mode, nt, eb, packed, a, s)
             : launch_episode_kind<QUAD_ENV_HOVER>(kc, kp, ctbr, spec, obs_mode, nt, eb, packed, a, s);
}
hipError_t launch_pop_policy_episode(const KConsts<float>* kc, const PopEpisodeEntry* tab, const int32_t* active,
                                     int count, int n, int env_kind, bool ctbr, bool spec, hipStream_t s) {
  int nt, eb;
  episode_block_shape(n, nt, eb);
  return env_kind == QUAD_ENV_TRAJ
             ? launch_pop_episode_kind<QUAD_ENV_TRAJ>(kc, tab, active, count, n, ctbr, spec, nt, eb, s)
             : launch_pop_episode_kind<QUAD_ENV_HOVER>(kc, tab, active, count, n, ctbr, spec, nt, eb, s);
}
#endif

}  // namespace quadenv
