// ctrl.hip -- the controller family on gfx950 (the laws: quad_ctrl.h; the PID ids call quad_pid.h).
//
// Kernels
//   k_ctrl_act<LAW>                 the law alone over [n,12] states and [n,9] targets, caller-owned state block
//   k_ctrl_episode<KIND, LAW, SPEC> the fused closed loop in k_pid_episode's shape (pid.hip): one thread per
//                                   env in 64-thread blocks, env loaded once, (law -> env_step) up to
//                                   max_steps times with the env, the eight controller states, the
//                                   parameter set and the metric accumulators in registers, one store
//   k_ctrl_waypoints<LAW, SPEC>     the same body with the waypoint tracker (quad_waypoints.h) after every
//                                   step: hover kind, (law -> env_step -> tracker) until the tracker's
//                                   status leaves 0 (quad_ctrl_waypoints)
//
// The law is a template argument, so each instantiation keeps only its own law's parameters and state
// rows live: the SMC rows 6-7 of the state block are loaded and stored by the SMC instantiation alone.
#include <hip/hip_runtime.h>

#include "../../include/quadenv.h"
#include "ctrl.h"
#include "dispatch.h"
#include "env_tiles.h"
#include "kconsts_default.h"
#include "quad_ctrl.h"
#include "quad_physics.h"
#include "quad_waypoints.h"

using namespace quadenv;

namespace {

constexpr int ACT_BLOCK = 256;
constexpr int EP_BLOCK = 64;

// the state-block rows a law reads and writes: the six integrators, and for SMC v_yaw and des_wz_prev
template <int LAW>
constexpr int rows_of() { return LAW == QUAD_CTRL_SMC ? CTRL_NSTATE : 6; }

template <int LAW>
__global__ __launch_bounds__(ACT_BLOCK) void k_ctrl_act(PidPlant plant, const QuadCtrlParams* __restrict__ params,
                                                        int32_t n_sets, const int32_t* __restrict__ set_of,
                                                        const float* __restrict__ state12,
                                                        const float* __restrict__ target9, int32_t n,
                                                        double* __restrict__ state, float4* __restrict__ actions,
                                                        double* __restrict__ diag) {
  const int i = blockIdx.x * ACT_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int set = set_of ? set_of[i] : 0;
  if (set < 0 || set >= n_sets) {  // never index the table
    actions[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    return;
  }
  const QuadCtrlParams C = params[set];
  float s[12], t[9];
#pragma unroll
  for (int j = 0; j < 12; j++) s[j] = state12[size_t(i) * 12 + j];
#pragma unroll
  for (int j = 0; j < 9; j++) t[j] = target9[size_t(i) * 9 + j];
  constexpr int ROWS = rows_of<LAW>();
  double cs[CTRL_NSTATE] = {};
#pragma unroll
  for (int j = 0; j < ROWS; j++) cs[j] = state[size_t(j) * size_t(n) + size_t(i)];
  float a[4];
  double d[CTRL_NDIAG];
  ctrl_law<LAW>(C, plant, s, t, cs, a, d);
#pragma unroll
  for (int j = 0; j < ROWS; j++) state[size_t(j) * size_t(n) + size_t(i)] = cs[j];
  actions[i] = make_float4(a[0], a[1], a[2], a[3]);
  if (diag) {
#pragma unroll
    for (int j = 0; j < CTRL_NDIAG; j++) diag[size_t(i) * CTRL_NDIAG + j] = d[j];
  }
}

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

// the metric status of a tracker status: lap -> QUAD_PID_LAP, terminated / truncated -> their codes
__device__ __forceinline__ int32_t metric_status_of(int32_t tracker_status) {
  return tracker_status == 1 ? QUAD_PID_LAP
                             : (tracker_status == 2 ? QUAD_PID_TERMINATED
                                                    : (tracker_status == 3 ? QUAD_PID_TRUNCATED : QUAD_PID_RUNNING));
}

// WP: the waypoint tracker runs after every step and ends the env's run (wr: the kernel's QuadWaypointRun;
// never read otherwise)
template <int KIND, int LAW, bool WP>
__device__ __forceinline__ void ctrl_episode_body(const KConsts<float>& K, const KParams& p, const PidPlant& plant,
                                                  const QuadCtrlRun& r, const QuadWaypointRun* wr) {
  const int i = blockIdx.x * EP_BLOCK + threadIdx.x;
  if (i >= p.n) return;
  PidAcc m;
  const int set = r.set_of ? r.set_of[i] : 0;
  if (set < 0 || set >= r.n_sets) {  // never index the table; the env takes no step
    store_metrics(r.metrics, i, m, QUAD_PID_INVALID);
    return;
  }
  const QuadCtrlParams C = r.params[set];
  WpTrack tk = {};
  const double* wp = nullptr;
  int cnt = 1;
  if constexpr (WP) {
    tk = load_track(wr->s, i);
    if (tk.status != 0) {  // finished in an earlier run: no step, env and tracker as they are
      store_metrics(r.metrics, i, m, metric_status_of(tk.status));
      return;
    }
    const int ws = wr->w.set_of ? wr->w.set_of[i] : 0;
    cnt = wr->w.counts[ws];
    wp = wr->w.points + size_t(ws) * wr->w.max_points * 3;
  }
  EnvRegs<float> e;
  load_env(p, i, e, false);
  const uint32_t ep = Tiles(p).ldu(F_EP, env_off(uint32_t(i)));
  float obs[12], s12[12], ti[9];
  observe(K, e, obs, s12);  // what quad_observe reports
  target_info_of<KIND>(K, p, i, e, ep, ti);
  constexpr int ROWS = rows_of<LAW>();
  double cs[CTRL_NSTATE] = {};
#pragma unroll
  for (int j = 0; j < ROWS; j++) cs[j] = r.state ? r.state[size_t(j) * size_t(p.n) + size_t(i)] : 0.0;
  const uint32_t M = uint32_t(r.trace_envs);
  const bool traced = uint32_t(i) < M;
  int32_t status = QUAD_PID_RUNNING;
  for (int t = 0; t < r.max_steps; t++) {
    float a[4];
    ctrl_law<LAW>(C, plant, s12, ti, cs, a, nullptr);
    const float tgt[3] = {ti[0], ti[1], ti[2]};  // the target read before the step
    StepRes sr;
    env_step<float, false>(K, e, a, sr);
#pragma unroll
    for (int j = 0; j < 12; j++) s12[j] = sr.state12[j];
    int flown = 0;
    if constexpr (WP) {
      flown = tk.wp_idx;
      float nt[3];
      if (wp_update(wp, cnt, wr->w.reach_radius, s12, sr.reward, sr.term, sr.trunc, tk, nt)) {
#pragma unroll
        for (int j = 0; j < 3; j++) e.target[j] = nt[j];
      }
    }
    target_info_of<KIND>(K, p, i, e, ep, ti);
    pid_acc_step(m, s12, tgt, sr.reward);
    if (traced) {
      const uint32_t row = uint32_t(t) * M + uint32_t(i);  // < 2^32 / 48: checked by quad_ctrl_episode
      if (r.trace_actions) sto(reinterpret_cast<float4*>(r.trace_actions), 16u * row, make_float4(a[0], a[1], a[2], a[3]));
      if (r.trace_state12) {
#pragma unroll
        for (int j = 0; j < 3; j++)
          sto(reinterpret_cast<float4*>(r.trace_state12), 48u * row + 16u * j,
              make_float4(s12[4 * j], s12[4 * j + 1], s12[4 * j + 2], s12[4 * j + 3]));
      }
      if constexpr (WP) {
        if (wr->trace_reward) sto(wr->trace_reward, 4u * row, sr.reward);
        if (wr->trace_wp_idx) sto(wr->trace_wp_idx, 4u * row, int32_t(flown));
      }
    }
    if constexpr (WP) {
      if (tk.status != 0) {
        status = metric_status_of(tk.status);
        break;
      }
    } else if (sr.term || sr.trunc) {
      status = sr.term ? QUAD_PID_TERMINATED : QUAD_PID_TRUNCATED;
      break;
    }
  }
  store_env(p, i, e, false);
  if (r.state) {
#pragma unroll
    for (int j = 0; j < ROWS; j++) r.state[size_t(j) * size_t(p.n) + size_t(i)] = cs[j];
  }
  store_metrics(r.metrics, i, m, status);
  if constexpr (WP) store_track(wr->s, i, tk);
}

template <int KIND, int LAW, bool SPEC>
__global__ __launch_bounds__(EP_BLOCK) void k_ctrl_episode(const KConsts<float>* __restrict__ kc, KParams p,
                                                           PidPlant plant, QuadCtrlRun r) {
  p.kc = kc;  // noalias: constant-block loads stay scalar after the stores (see KParams)
  if constexpr (SPEC) {
    constexpr KConsts<float> K = kdef_block<KIND, false>();
    ctrl_episode_body<KIND, LAW, false>(K, p, plant, r, nullptr);
  } else {
    ctrl_episode_body<KIND, LAW, false>(*kc, p, plant, r, nullptr);
  }
}

// the WP form of k_ctrl_episode: hover kind only (a switch overwrites the target register), the tracker's
// tables and rows in a kernel argument of its own so k_ctrl_episode's arguments stay as they are
template <int LAW, bool SPEC>
__global__ __launch_bounds__(EP_BLOCK) void k_ctrl_waypoints(const KConsts<float>* __restrict__ kc, KParams p,
                                                             PidPlant plant, QuadCtrlRun r, QuadWaypointRun wr) {
  p.kc = kc;
  if constexpr (SPEC) {
    constexpr KConsts<float> K = kdef_block<QUAD_ENV_HOVER, false>();
    ctrl_episode_body<QUAD_ENV_HOVER, LAW, true>(K, p, plant, r, &wr);
  } else {
    ctrl_episode_body<QUAD_ENV_HOVER, LAW, true>(*kc, p, plant, r, &wr);
  }
}

// f(law): law = std::integral_constant<int, QUAD_CTRL_*>; the caller has checked the range
template <class F>
void with_law(int law, F&& f) {
  switch (law) {
    case QUAD_CTRL_PID_YAW: f(std::integral_constant<int, QUAD_CTRL_PID_YAW>{}); break;
    case QUAD_CTRL_PID_WORLD: f(std::integral_constant<int, QUAD_CTRL_PID_WORLD>{}); break;
    case QUAD_CTRL_SE3: f(std::integral_constant<int, QUAD_CTRL_SE3>{}); break;
    case QUAD_CTRL_SMC: f(std::integral_constant<int, QUAD_CTRL_SMC>{}); break;
    default: f(std::integral_constant<int, QUAD_CTRL_LQR>{}); break;
  }
}

}  // namespace

namespace quadenv {

hipError_t launch_ctrl_act(const PidPlant& plant, const QuadCtrlParams* params, int32_t n_sets, const int32_t* set_of,
                           int32_t law, const float* state12, const float* target9, int32_t n, double* state,
                           float* actions, double* diag, hipStream_t s) {
  const dim3 grid((n + ACT_BLOCK - 1) / ACT_BLOCK), blk(ACT_BLOCK);
  with_law(law, [&](auto lw) {
    hipLaunchKernelGGL(k_ctrl_act<decltype(lw)::value>, grid, blk, 0, s, plant, params, n_sets, set_of, state12,
                       target9, n, state, reinterpret_cast<float4*>(actions), diag);
  });
  return hipGetLastError();
}

hipError_t launch_ctrl_episode(const KConsts<float>* kc, const KParams& kp, int env_kind, bool spec,
                               const PidPlant& plant, const QuadCtrlRun& r, hipStream_t s) {
  const dim3 grid((kp.n + EP_BLOCK - 1) / EP_BLOCK), blk(EP_BLOCK);
  with_law(r.law, [&](auto lw) {
    with_kind(env_kind == QUAD_ENV_TRAJ, spec, [&](auto kind, auto sp) {
      hipLaunchKernelGGL((k_ctrl_episode<decltype(kind)::value, decltype(lw)::value, decltype(sp)::value>), grid, blk,
                         0, s, kc, kp, plant, r);
    });
  });
  return hipGetLastError();
}

hipError_t launch_ctrl_waypoints(const KConsts<float>* kc, const KParams& kp, bool spec, const PidPlant& plant,
                                 const QuadCtrlRun& r, const QuadWaypointRun& wr, hipStream_t s) {
  const dim3 grid((kp.n + EP_BLOCK - 1) / EP_BLOCK), blk(EP_BLOCK);
  with_law(r.law, [&](auto lw) {
    with_bool(spec, [&](auto sp) {
      hipLaunchKernelGGL((k_ctrl_waypoints<decltype(lw)::value, decltype(sp)::value>), grid, blk, 0, s, kc, kp, plant,
                         r, wr);
    });
  });
  return hipGetLastError();
}

}  // namespace quadenv
