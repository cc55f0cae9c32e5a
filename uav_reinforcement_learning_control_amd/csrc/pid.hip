// pid.hip -- the cascaded PID baseline on gfx950 (the law: quad_pid.h).
//
// Kernels
//   k_pid_act        the law alone over [n,12] states and [n,9] targets, caller-owned integrators
//   k_pid_episode    the fused closed loop: one thread per env, state loaded once, (law -> env_step)
//                    up to max_steps times in registers, metrics and state stored once
//   k_target_info    info["target" / "target_vel" / "target_acc"] for the envs' current step count
//
// k_pid_episode runs 64-thread blocks at every size: 65,536 envs are 1,024 waves, one per SIMD of the
// 256 CUs, and below that a wider block would only leave CUs empty; above it the launch is
// throughput-bound on the same per-wave chain and the block size does not enter. One wave per SIMD
// may hold all 512 VGPRs, so the env state, the six float64 integrators, the gain set (22 doubles,
// per lane: set_of is lane-varying) and the metric accumulators stay in registers across the loop.
// A wave leaves the loop when its last lane has finished, which is why callers lay batches out
// candidate-major (a wave's 64 lanes share a gain set and tend to finish together).
#include <hip/hip_runtime.h>

#include "../../include/quadenv.h"
#include "dispatch.h"
#include "env_tiles.h"
#include "kconsts_default.h"
#include "pid.h"
#include "quad_physics.h"
#include "quad_pid.h"

using namespace quadenv;

namespace {

constexpr int ACT_BLOCK = 256;
constexpr int EP_BLOCK = 64;

template <int MODE>
__global__ __launch_bounds__(ACT_BLOCK) void k_pid_act(PidPlant plant, const QuadPidGains* __restrict__ gains,
                                                       int32_t n_sets, const int32_t* __restrict__ set_of,
                                                       const float* __restrict__ state12,
                                                       const float* __restrict__ target9, int32_t n,
                                                       double* __restrict__ integ, float4* __restrict__ actions,
                                                       double* __restrict__ diag) {
  const int i = blockIdx.x * ACT_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int set = set_of ? set_of[i] : 0;
  if (set < 0 || set >= n_sets) {  // never index the table
    actions[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    return;
  }
  const QuadPidGains G = gains[set];
  float s[12], t[9];
#pragma unroll
  for (int j = 0; j < 12; j++) s[j] = state12[size_t(i) * 12 + j];
#pragma unroll
  for (int j = 0; j < 9; j++) t[j] = target9[size_t(i) * 9 + j];
  double in[6];
#pragma unroll
  for (int j = 0; j < 6; j++) in[j] = integ[size_t(j) * size_t(n) + size_t(i)];
  float a[4];
  double d[6];
  pid_law<MODE>(G, plant, s, t, in, a, d);
#pragma unroll
  for (int j = 0; j < 6; j++) integ[size_t(j) * size_t(n) + size_t(i)] = in[j];
  actions[i] = make_float4(a[0], a[1], a[2], a[3]);
  if (diag) {
#pragma unroll
    for (int j = 0; j < 6; j++) diag[size_t(i) * 6 + j] = d[j];
  }
}

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

template <int KIND, int MODE>
__device__ __forceinline__ void pid_episode_body(const KConsts<float>& K, const KParams& p, const PidPlant& plant,
                                                 const QuadPidRun& r) {
  const int i = blockIdx.x * EP_BLOCK + threadIdx.x;
  if (i >= p.n) return;
  PidAcc m;
  const int set = r.set_of ? r.set_of[i] : 0;
  if (set < 0 || set >= r.n_sets) {  // never index the table; the env takes no step
    store_metrics(r.metrics, i, m, QUAD_PID_INVALID);
    return;
  }
  const QuadPidGains G = r.gains[set];
  EnvRegs<float> e;
  load_env(p, i, e, false);
  const uint32_t ep = Tiles(p).ldu(F_EP, env_off(uint32_t(i)));
  float obs[12], s12[12], ti[9];
  observe(K, e, obs, s12);  // what quad_observe reports
  target_info_of<KIND>(K, p, i, e, ep, ti);
  double integ[6];
#pragma unroll
  for (int j = 0; j < 6; j++) integ[j] = r.integ ? r.integ[size_t(j) * size_t(p.n) + size_t(i)] : 0.0;
  const uint32_t M = uint32_t(r.trace_envs);
  const bool traced = uint32_t(i) < M;
  int32_t status = QUAD_PID_RUNNING;
  for (int t = 0; t < r.max_steps; t++) {
    float a[4];
    pid_law<MODE>(G, plant, s12, ti, integ, a, nullptr);
    const float tgt[3] = {ti[0], ti[1], ti[2]};  // the target read before the step
    StepRes sr;
    env_step<float, false>(K, e, a, sr);
#pragma unroll
    for (int j = 0; j < 12; j++) s12[j] = sr.state12[j];
    target_info_of<KIND>(K, p, i, e, ep, ti);
    pid_acc_step(m, s12, tgt, sr.reward);
    if (traced) {
      const uint32_t row = uint32_t(t) * M + uint32_t(i);  // < 2^32 / 48: checked by quad_pid_episode
      if (r.trace_actions) sto(reinterpret_cast<float4*>(r.trace_actions), 16u * row, make_float4(a[0], a[1], a[2], a[3]));
      if (r.trace_state12) {
#pragma unroll
        for (int j = 0; j < 3; j++)
          sto(reinterpret_cast<float4*>(r.trace_state12), 48u * row + 16u * j,
              make_float4(s12[4 * j], s12[4 * j + 1], s12[4 * j + 2], s12[4 * j + 3]));
      }
    }
    if (sr.term || sr.trunc) {
      status = sr.term ? QUAD_PID_TERMINATED : QUAD_PID_TRUNCATED;
      break;
    }
  }
  store_env(p, i, e, false);
  if (r.integ) {
#pragma unroll
    for (int j = 0; j < 6; j++) r.integ[size_t(j) * size_t(p.n) + size_t(i)] = integ[j];
  }
  store_metrics(r.metrics, i, m, status);
}

template <int KIND, int MODE, bool SPEC>
__global__ __launch_bounds__(EP_BLOCK) void k_pid_episode(const KConsts<float>* __restrict__ kc, KParams p,
                                                          PidPlant plant, QuadPidRun r) {
  p.kc = kc;  // noalias: constant-block loads stay scalar after the stores (see KParams)
  if constexpr (SPEC) {
    constexpr KConsts<float> K = kdef_block<KIND, false>();
    pid_episode_body<KIND, MODE>(K, p, plant, r);
  } else {
    pid_episode_body<KIND, MODE>(*kc, p, plant, r);
  }
}

template <int KIND>
__global__ __launch_bounds__(ACT_BLOCK) void k_target_info(const KConsts<float>* __restrict__ kc, KParams p,
                                                           float* __restrict__ out) {
  p.kc = kc;
  const int i = blockIdx.x * ACT_BLOCK + threadIdx.x;
  if (i >= p.n) return;
  EnvRegs<float> e;
  load_env(p, i, e, false);
  const uint32_t ep = Tiles(p).ldu(F_EP, env_off(uint32_t(i)));
  float o[9];
  target_info_of<KIND>(*kc, p, i, e, ep, o);
#pragma unroll
  for (int j = 0; j < 9; j++) out[size_t(i) * 9 + j] = o[j];
}

}  // namespace

namespace quadenv {

hipError_t launch_pid_act(const PidPlant& plant, const QuadPidGains* gains, int32_t n_sets, const int32_t* set_of,
                          int32_t mode, const float* state12, const float* target9, int32_t n, double* integ,
                          float* actions, double* diag, hipStream_t s) {
  const dim3 grid((n + ACT_BLOCK - 1) / ACT_BLOCK), blk(ACT_BLOCK);
  with_bool(mode == QUAD_PID_WORLD_FRAME, [&](auto world) {
    constexpr int MODE = decltype(world)::value ? QUAD_PID_WORLD_FRAME : QUAD_PID_YAW_FRAME;
    hipLaunchKernelGGL(k_pid_act<MODE>, grid, blk, 0, s, plant, gains, n_sets, set_of, state12, target9, n, integ,
                       reinterpret_cast<float4*>(actions), diag);
  });
  return hipGetLastError();
}

hipError_t launch_pid_episode(const KConsts<float>* kc, const KParams& kp, int env_kind, bool spec,
                              const PidPlant& plant, const QuadPidRun& r, hipStream_t s) {
  const dim3 grid((kp.n + EP_BLOCK - 1) / EP_BLOCK), blk(EP_BLOCK);
  with_kind(env_kind == QUAD_ENV_TRAJ, r.mode == QUAD_PID_WORLD_FRAME, [&](auto kind, auto world) {
    with_bool(spec, [&](auto sp) {
      constexpr int MODE = decltype(world)::value ? QUAD_PID_WORLD_FRAME : QUAD_PID_YAW_FRAME;
      hipLaunchKernelGGL((k_pid_episode<decltype(kind)::value, MODE, decltype(sp)::value>), grid, blk, 0, s, kc, kp,
                         plant, r);
    });
  });
  return hipGetLastError();
}

hipError_t launch_target_info(const KConsts<float>* kc, const KParams& kp, int env_kind, float* target_info,
                              hipStream_t s) {
  const dim3 grid((kp.n + ACT_BLOCK - 1) / ACT_BLOCK), blk(ACT_BLOCK);
  with_bool(env_kind == QUAD_ENV_TRAJ, [&](auto tr) {
    constexpr int KIND = decltype(tr)::value ? QUAD_ENV_TRAJ : QUAD_ENV_HOVER;
    hipLaunchKernelGGL(k_target_info<KIND>, grid, blk, 0, s, kc, kp, target_info);
  });
  return hipGetLastError();
}

}  // namespace quadenv
