// ctrl.hip -- the controller kernels on gfx950 and their C entry points: the cascaded PID baseline (quad_pid_*)
// and the controller family (quad_ctrl_*) are one kernel family (the laws: quad_pid.h, quad_ctrl.h); quad_target_info.
//
// Kernels
//   k_ctrl_act<ROW, LAW>                 the law alone over [n,12] states and [n,9] targets, caller-owned state block
//   k_ctrl_episode<ROW, KIND, LAW, SPEC> the fused closed loop: one thread per env, env loaded once, (law ->
//                                        env_step) up to max_steps times in registers, metrics and state stored once
//   k_ctrl_waypoints<LAW, SPEC>          the same body with the waypoint tracker (quad_waypoints.h) after every
//                                        step: hover kind, (law -> env_step -> tracker) until the tracker's
//                                        status leaves 0 (quad_ctrl_waypoints)
//   k_target_info<KIND>                  info["target" / "target_vel" / "target_acc"] for the envs' current step count
//
// ROW is the table's row type and fixes, at compile time, the row load, the law call and the diag width:
//   QuadPidGains    22 doubles; pid_law on the row itself; diag [n,6]          (quad_pid_act, quad_pid_episode)
//   QuadCtrlParams  33 doubles; ctrl_law<LAW>;             diag [n,CTRL_NDIAG] (quad_ctrl_*)
// so quad_pid_episode and quad_ctrl_episode with a PID law run the same body on the same law and give the
// same bits. The law is a template argument too, so each instantiation keeps only its own law's parameters
// and state rows live: the SMC rows 6-7 of the state block are loaded and stored by the SMC instantiation alone.
//
// The episode kernels run 64-thread blocks at every size: 65,536 envs are 1,024 waves, one per SIMD of the
// 256 CUs, and below that a wider block would only leave CUs empty; above it the launch is
// throughput-bound on the same per-wave chain and the block size does not enter. One wave per SIMD
// may hold all 512 VGPRs, so the env state, the controller states, the parameter set (per lane: set_of is
// lane-varying) and the metric accumulators stay in registers across the loop.
// A wave leaves the loop when its last lane has finished, which is why callers lay batches out
// candidate-major (a wave's 64 lanes share a parameter set and tend to finish together).
#include <hip/hip_runtime.h>

#include "../../include/quadenv.h"
#include "dispatch.h"
#include "env_tiles.h"
#include "handle.h"
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

// a gain row carries the two PID laws (LAW = the mode), calls pid_law on itself and reports pid_law's six diag columns
template <class ROW>
constexpr bool PID_ROW = std::is_same<ROW, QuadPidGains>::value;

template <class ROW, int LAW>
__global__ __launch_bounds__(ACT_BLOCK) void k_ctrl_act(PidPlant plant, const ROW* __restrict__ rows, int32_t n_sets,
                                                        const int32_t* __restrict__ set_of,
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
  const ROW C = rows[set];
  float s[12], t[9];
#pragma unroll
  for (int j = 0; j < 12; j++) s[j] = state12[size_t(i) * 12 + j];
#pragma unroll
  for (int j = 0; j < 9; j++) t[j] = target9[size_t(i) * 9 + j];
  constexpr int ROWS = rows_of<LAW>(), NDIAG = PID_ROW<ROW> ? 6 : CTRL_NDIAG;
  double cs[CTRL_NSTATE] = {};
#pragma unroll
  for (int j = 0; j < ROWS; j++) cs[j] = state[size_t(j) * size_t(n) + size_t(i)];
  float a[4];
  double d[NDIAG];
  if constexpr (PID_ROW<ROW>) {
    pid_law<LAW>(C, plant, s, t, cs, a, d);
  } else {
    ctrl_law<LAW>(C, plant, s, t, cs, a, d);
  }
#pragma unroll
  for (int j = 0; j < ROWS; j++) state[size_t(j) * size_t(n) + size_t(i)] = cs[j];
  actions[i] = make_float4(a[0], a[1], a[2], a[3]);
  if (diag) {
#pragma unroll
    for (int j = 0; j < NDIAG; j++) diag[size_t(i) * NDIAG + j] = d[j];
  }
}

// QuadPidRun / QuadCtrlRun as the kernels take it: the two have one layout, field for field, and differ in the
// table's row type (law: the mode of a QuadPidRun; the host dispatches on it)
template <class ROW>
struct Run {
  const ROW* rows;
  const int32_t* set_of;
  int32_t n_sets, law, max_steps, trace_envs;
  double* state;
  float *trace_actions, *trace_state12;
  QuadPidMetrics metrics;
};
Run<QuadPidGains> run_of(const QuadPidRun& r) {
  return {r.gains, r.set_of, r.n_sets, r.mode, r.max_steps, r.trace_envs, r.integ, r.trace_actions, r.trace_state12,
          r.metrics};
}
Run<QuadCtrlParams> run_of(const QuadCtrlRun& r) {
  return {r.params, r.set_of, r.n_sets, r.law, r.max_steps, r.trace_envs, r.state, r.trace_actions, r.trace_state12,
          r.metrics};
}

// WP: the waypoint tracker runs after every step and ends the env's run (wr: the kernel's QuadWaypointRun;
// never read otherwise)
template <class ROW, int KIND, int LAW, bool WP>
__device__ __forceinline__ void ctrl_episode_body(const KConsts<float>& K, const KParams& p, const PidPlant& plant,
                                                  const Run<ROW>& r, const QuadWaypointRun* wr) {
  const int i = blockIdx.x * EP_BLOCK + threadIdx.x;
  if (i >= p.n) return;
  PidAcc m;
  const int set = r.set_of ? r.set_of[i] : 0;
  if (set < 0 || set >= r.n_sets) {  // never index the table; the env takes no step
    store_metrics(r.metrics, i, m, QUAD_PID_INVALID);
    return;
  }
  const ROW C = r.rows[set];
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
    if constexpr (PID_ROW<ROW>) {
      pid_law<LAW>(C, plant, s12, ti, cs, a, nullptr);
    } else {
      ctrl_law<LAW>(C, plant, s12, ti, cs, a, nullptr);
    }
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
      const uint32_t row = uint32_t(t) * M + uint32_t(i);  // < 2^32 / 48: checked by the entry point
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

template <class ROW, int KIND, int LAW, bool SPEC>
__global__ __launch_bounds__(EP_BLOCK) void k_ctrl_episode(const KConsts<float>* __restrict__ kc, KParams p,
                                                           PidPlant plant, Run<ROW> r) {
  p.kc = kc;  // noalias: constant-block loads stay scalar after the stores (see KParams)
  if constexpr (SPEC) {
    constexpr KConsts<float> K = kdef_block<KIND, false>();
    ctrl_episode_body<ROW, KIND, LAW, false>(K, p, plant, r, nullptr);
  } else {
    ctrl_episode_body<ROW, KIND, LAW, false>(*kc, p, plant, r, nullptr);
  }
}

// the WP form of k_ctrl_episode: hover kind only (a switch overwrites the target register), QuadCtrlParams
// rows only, the tracker's tables and rows in a kernel argument of its own
template <int LAW, bool SPEC>
__global__ __launch_bounds__(EP_BLOCK) void k_ctrl_waypoints(const KConsts<float>* __restrict__ kc, KParams p,
                                                             PidPlant plant, Run<QuadCtrlParams> r,
                                                             QuadWaypointRun wr) {
  p.kc = kc;
  if constexpr (SPEC) {
    constexpr KConsts<float> K = kdef_block<QUAD_ENV_HOVER, false>();
    ctrl_episode_body<QuadCtrlParams, QUAD_ENV_HOVER, LAW, true>(K, p, plant, r, &wr);
  } else {
    ctrl_episode_body<QuadCtrlParams, QUAD_ENV_HOVER, LAW, true>(*kc, p, plant, r, &wr);
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

// f(law): law = std::integral_constant<int, id>, over the ids a ROW table carries (QuadPidGains: the two PID
// modes = the two PID law ids; QuadCtrlParams: every QUAD_CTRL_*); the caller has checked the range
template <class ROW, class F>
void with_law(int law, F&& f) {
  if constexpr (!PID_ROW<ROW>) {
    switch (law) {
      case QUAD_CTRL_SE3: return f(std::integral_constant<int, QUAD_CTRL_SE3>{});
      case QUAD_CTRL_SMC: return f(std::integral_constant<int, QUAD_CTRL_SMC>{});
      case QUAD_CTRL_LQR: return f(std::integral_constant<int, QUAD_CTRL_LQR>{});
      default: break;
    }
  }
  static_assert(QUAD_CTRL_PID_YAW == QUAD_PID_YAW_FRAME && QUAD_CTRL_PID_WORLD == QUAD_PID_WORLD_FRAME, "PID ids");
  if (law == QUAD_CTRL_PID_WORLD) return f(std::integral_constant<int, QUAD_CTRL_PID_WORLD>{});
  return f(std::integral_constant<int, QUAD_CTRL_PID_YAW>{});
}

template <class ROW>
hipError_t launch_act(const PidPlant& plant, const ROW* rows, int32_t n_sets, const int32_t* set_of, int32_t law,
                      const float* state12, const float* target9, int32_t n, double* state, float* actions,
                      double* diag, hipStream_t s) {
  const dim3 grid((n + ACT_BLOCK - 1) / ACT_BLOCK), blk(ACT_BLOCK);
  with_law<ROW>(law, [&](auto lw) {
    hipLaunchKernelGGL((k_ctrl_act<ROW, decltype(lw)::value>), grid, blk, 0, s, plant, rows, n_sets, set_of, state12,
                       target9, n, state, reinterpret_cast<float4*>(actions), diag);
  });
  return hipGetLastError();
}

template <class ROW>
hipError_t launch_episode(const KConsts<float>* kc, const KParams& kp, int env_kind, bool spec, const PidPlant& plant,
                          const Run<ROW>& r, hipStream_t s) {
  const dim3 grid((kp.n + EP_BLOCK - 1) / EP_BLOCK), blk(EP_BLOCK);
  with_law<ROW>(r.law, [&](auto lw) {
    with_kind(env_kind == QUAD_ENV_TRAJ, spec, [&](auto kind, auto sp) {
      hipLaunchKernelGGL((k_ctrl_episode<ROW, decltype(kind)::value, decltype(lw)::value, decltype(sp)::value>), grid,
                         blk, 0, s, kc, kp, plant, r);
    });
  });
  return hipGetLastError();
}

}  // namespace

constexpr LawIds PID_MODES{QUAD_PID_YAW_FRAME, QUAD_PID_WORLD_FRAME, "mode", "gains"};
constexpr LawIds CTRL_LAWS{QUAD_CTRL_PID_YAW, QUAD_CTRL_LQR, "law", "params"};

extern "C" {

// ---- cascaded PID baseline (QuadPidGains rows)
int quad_pid_default_gains(QuadPidGains* g) {
  if (!g) return fail(QUAD_EINVAL, "gains is NULL");
  pid_default_gains_fill(g);
  return QUAD_OK;
}

int quad_pid_act(QuadHandle* h, const QuadPidGains* gains, int32_t n_sets, const int32_t* set_of, int32_t mode,
                 const float* state12, const float* target9, int32_t n, double* integ, float* actions,
                 double* diag, void* stream) {
  if (!h) return fail(QUAD_EINVAL, "handle is NULL");
  if (int rc = check_law_table(h, "quad_pid_act", PID_MODES, mode, n_sets, gains)) return rc;
  if (int rc = check_act_rows("quad_pid_act", state12, target9, integ, "integ", actions, n)) return rc;
  DeviceGuard g(h->device);
  HIP_TRY(launch_act(make_pid_plant(h->cfg), gains, n_sets, set_of, mode, state12, target9, n, integ, actions, diag,
                     static_cast<hipStream_t>(stream)));
  return QUAD_OK;
}

// ---- controller family (QuadCtrlParams rows); quad_pid_*'s rules with a law id in place of the mode
int quad_ctrl_default_params(QuadCtrlParams* p) {
  if (!p) return fail(QUAD_EINVAL, "params is NULL");
  ctrl_default_params_fill(p);
  return QUAD_OK;
}

int quad_ctrl_act(QuadHandle* h, const QuadCtrlParams* params, int32_t n_sets, const int32_t* set_of, int32_t law,
                  const float* state12, const float* target9, int32_t n, double* state, float* actions,
                  double* diag, void* stream) {
  if (!h) return fail(QUAD_EINVAL, "handle is NULL");
  if (int rc = check_law_table(h, "quad_ctrl_act", CTRL_LAWS, law, n_sets, params)) return rc;
  if (int rc = check_act_rows("quad_ctrl_act", state12, target9, state, "state", actions, n)) return rc;
  DeviceGuard g(h->device);
  HIP_TRY(launch_act(make_pid_plant(h->cfg), params, n_sets, set_of, law, state12, target9, n, state, actions, diag,
                     static_cast<hipStream_t>(stream)));
  return QUAD_OK;
}

// ---- the fused episodes of both row types (k_ctrl_episode)
int quad_pid_episode(QuadHandle* h, const QuadPidRun* r, void* stream) {
  if (!h || !r) return fail(QUAD_EINVAL, "handle/run is NULL");
  if (int rc = check_law_table(h, "quad_pid_episode", PID_MODES, r->mode, r->n_sets, r->gains)) return rc;
  const bool any_trace = r->trace_actions || r->trace_state12;
  if (int rc = check_run("quad_pid_episode", h->n, r->max_steps, r->trace_envs, r->metrics,
                         reinterpret_cast<uintptr_t>(r->trace_actions) | reinterpret_cast<uintptr_t>(r->trace_state12),
                         any_trace, "traces"))
    return rc;
  DeviceGuard g(h->device);
  QuadPidRun run = *r;
  if (!any_trace) run.trace_envs = 0;
  HIP_TRY(launch_episode(h->kdev, h->kp, h->cfg.env_kind, h->spec, make_pid_plant(h->cfg), run_of(run),
                         static_cast<hipStream_t>(stream)));
  return QUAD_OK;
}

int quad_ctrl_episode(QuadHandle* h, const QuadCtrlRun* r, void* stream) {
  if (!h || !r) return fail(QUAD_EINVAL, "handle/run is NULL");
  if (int rc = check_law_table(h, "quad_ctrl_episode", CTRL_LAWS, r->law, r->n_sets, r->params)) return rc;
  const bool any_trace = r->trace_actions || r->trace_state12;
  if (int rc = check_run("quad_ctrl_episode", h->n, r->max_steps, r->trace_envs, r->metrics,
                         reinterpret_cast<uintptr_t>(r->trace_actions) | reinterpret_cast<uintptr_t>(r->trace_state12),
                         any_trace, "traces"))
    return rc;
  DeviceGuard g(h->device);
  QuadCtrlRun run = *r;
  if (!any_trace) run.trace_envs = 0;
  HIP_TRY(launch_episode(h->kdev, h->kp, h->cfg.env_kind, h->spec, make_pid_plant(h->cfg), run_of(run),
                         static_cast<hipStream_t>(stream)));
  return QUAD_OK;
}

// ---- waypoint laps in one launch (k_ctrl_waypoints)
int quad_ctrl_waypoints(QuadHandle* h, const QuadCtrlRun* r, const QuadWaypointRun* wr, void* stream) {
  if (!h || !r || !wr) return fail(QUAD_EINVAL, "handle/run/waypoints is NULL");
  if (int rc = check_waypoint_run(h, "quad_ctrl_waypoints", wr)) return rc;
  if (int rc = check_law_table(h, "quad_ctrl_waypoints", CTRL_LAWS, r->law, r->n_sets, r->params)) return rc;
  const bool any_trace = r->trace_actions || r->trace_state12 || wr->trace_reward || wr->trace_wp_idx;
  if (int rc = check_run("quad_ctrl_waypoints", h->n, r->max_steps, r->trace_envs, r->metrics,
                         reinterpret_cast<uintptr_t>(r->trace_actions) | reinterpret_cast<uintptr_t>(r->trace_state12),
                         any_trace, "traces"))
    return rc;
  DeviceGuard g(h->device);
  Run<QuadCtrlParams> run = run_of(*r);
  if (!any_trace) run.trace_envs = 0;
  const dim3 grid((h->n + EP_BLOCK - 1) / EP_BLOCK), blk(EP_BLOCK);
  with_law<QuadCtrlParams>(run.law, [&](auto lw) {
    with_bool(h->spec, [&](auto sp) {
      hipLaunchKernelGGL((k_ctrl_waypoints<decltype(lw)::value, decltype(sp)::value>), grid, blk, 0,
                         static_cast<hipStream_t>(stream), h->kdev, h->kp, make_pid_plant(h->cfg), run, *wr);
    });
  });
  HIP_TRY(hipGetLastError());
  return QUAD_OK;
}

int quad_target_info(QuadHandle* h, float* target_info, void* stream) {
  if (!h || !target_info) return fail(QUAD_EINVAL, "handle/target_info is NULL");
  if (h->cfg.env_kind != QUAD_ENV_HOVER && h->cfg.env_kind != QUAD_ENV_TRAJ)
    return fail(QUAD_EINVAL, "quad_target_info: env_kind must be HOVER or TRAJ");
  DeviceGuard g(h->device);
  const dim3 grid((h->n + ACT_BLOCK - 1) / ACT_BLOCK), blk(ACT_BLOCK);
  with_bool(h->cfg.env_kind == QUAD_ENV_TRAJ, [&](auto tr) {
    constexpr int KIND = decltype(tr)::value ? QUAD_ENV_TRAJ : QUAD_ENV_HOVER;
    hipLaunchKernelGGL(k_target_info<KIND>, grid, blk, 0, static_cast<hipStream_t>(stream), h->kdev, h->kp, target_info);
  });
  HIP_TRY(hipGetLastError());
  return QUAD_OK;
}

}  // extern "C"
