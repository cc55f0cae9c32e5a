// policy_episode_body.h -- the fused closed loop of the policy-episode kernels (device only): k_policy_episode /
// k_policy_waypoints (policy_episode.hip, the 12-128-128-4 ReLU actor of policy_net.h) and k_actor_episode /
// k_actor_waypoints (actor_arch.hip, the general actor of actor_arch.h) compile the same body with their own
// forward. The forward is a functor FWD:
//   fw.template stage<BLK>()   once, by the whole block: the net's image into LDS (ends with a barrier)
//   fw(ob, act)                per step, full wave: ob[12] of this lane's env -> act[4], the unclipped action
//                              of this lane's env (every MFMA and lane exchange outside any per-lane branch)
// The two rules of policy_episode.hip's header hold for every forward.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/quadenv.h"
#include "env_tiles.h"
#include "policy_episode.h"
#include "policy_net.h"
#include "quad_deploy.h"
#include "quad_physics.h"
#include "quad_pid.h"
#include "quad_waypoints.h"

namespace quadenv {

// The metric store and the tracker's status codes are the controller kernels' (store_metrics, metric_status_of:
// quad_pid.h).

__device__ __forceinline__ void store_row12(float* base, uint32_t row, const float v[12]) {
#pragma unroll
  for (int j = 0; j < 3; j++)
    sto(reinterpret_cast<float4*>(base), 48u * row + 16u * j, make_float4(v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]));
}

// NT = 2: wave w of a block owns envs 64w .. 64w + 63 = its two MFMA tiles. NT = 1: wave w owns the 32
// envs 32w .. 32w + 31; lanes l and l + 32 both carry env l & 31 (the same bits), the lower half stores.
// EB: envs per block (256: k_rollout's shape; 64: one or two waves, for evaluation-sized batches).
// WP: the waypoint tracker runs after every committed step and ends the env's run (wr: the kernel's
// QuadWaypointRun; never read otherwise)
template <int KIND, bool CTBR, int NT, int MODE, int EB, bool WP, typename FWD>
__device__ __forceinline__ void episode_body(const KConsts<float>& K, const KParams& p, FWD& fw, const EpisodeArgs& a,
                                             const QuadWaypointRun* wr) {
  constexpr int BLK = EB * 2 / NT;
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
  fw.template stage<BLK>();
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
    float act[ACT], ac[ACT];
    fw(ob, act);
#pragma unroll
    for (int k = 0; k < ACT; k++) ac[k] = fminf(fmaxf(act[k], -1.f), 1.f);
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

}  // namespace quadenv
