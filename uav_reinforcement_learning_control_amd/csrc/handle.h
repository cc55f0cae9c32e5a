// handle.h -- the env handle and the argument checks that several kernel families' C entry points share (host
// only). Every file that holds entry points includes it; the checks are defined once, in quadenv.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/quadenv.h"
#include "env_tiles.h"
#include "policy_episode.h"  // EpisodeArgs

struct QuadHandle {
  QuadCfg cfg;
  quadenv::PhysConstsD pd;
  quadenv::KParams kp;
  int device;
  int n;
  float* tiles = nullptr;     // env state (layout at the top of quadenv.hip)
  size_t tile_bytes = 0;
  uint32_t* stage = nullptr;  // [NFT][n] staging for host-side get/set_state, allocated on first use
  quadenv::KConsts<float> kh;                 // host copy of the constant block
  quadenv::KConsts<float>* kdev = nullptr;    // device copy the kernels read (scalar loads, K$-resident)
  bool spec = false;                 // kh == a reference default block: k_step_h's SPEC form
  int hblock = 0;                    // envs per k_step_h block: 0 = by size (h_wide: 256 between H_SMALL and 2M, else 64)
  int hd = -1;                       // k_step_hd for the 64-env nt launches: -1 = by size (hd_form), 0 / 1
  int nt = -1;                       // k_step_h's state cache policy: -1 = by size (nt_state), 0 / 1
};

namespace quadenv {

// one last-error slot per thread for the whole library (quad_last_error)
int set_error(int code, const char* msg);
int fail(int code, const std::string& msg);
int hip_fail(hipError_t e, const char* what);  // QUAD_EHIP, "what: hipGetErrorString(e)"

#define HIP_TRY(expr)                                  \
  do {                                                 \
    hipError_t e__ = (expr);                           \
    if (e__ != hipSuccess) return hip_fail(e__, #expr); \
  } while (0)

struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) (void)hipSetDevice(dev);
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// wrapper kinds: the RelPosActWrapper output stage (obs7) and the CTBR action path
inline bool wrap_relpos(int32_t w) { return w == QUAD_WRAP_RELPOS || w == QUAD_WRAP_CTBR_RELPOS; }
inline bool wrap_ctbr(int32_t w) { return w == QUAD_WRAP_CTBR || w == QUAD_WRAP_CTBR_RELPOS; }

// ---- what the fused runs and the controller calls check alike; who: the entry point the messages name
int check_est(const QuadVelEst* e, const char* who);

// The common fields of a run (QuadPidRun, QuadCtrlRun, QuadPolicyRun), in this order: max_steps, the twelve
// metrics arrays, trace_envs' range, a policy run's estimator (est and est_dt; NULL for a controller run) and,
// with a trace requested, the 32-bit bound on the trace rows' byte offsets and the 16-byte alignment of
// `aligned`: the OR of the pointers the kernels store 16 bytes at a time, which align_what names.
int check_run(const char* who, int32_t n, int32_t max_steps, int32_t trace_envs, const QuadPidMetrics& m,
              uintptr_t aligned, bool any_trace, const char* align_what, const QuadVelEst* est = nullptr,
              double est_dt = 1.0);

// what quad_pid_* (ids: the modes) and quad_ctrl_* (ids: the laws) ask of the handle and of the table
struct LawIds {
  int32_t lo, hi;            // the valid ids
  const char *what, *table;  // the words the messages print
};
int check_law_table(const QuadHandle* h, const char* who, const LawIds& ids, int32_t id, int32_t n_sets,
                    const void* table);

// the rows of quad_pid_act / quad_ctrl_act; state_name: "integ" / "state"
int check_act_rows(const char* who, const float* state12, const float* target9, const double* state,
                   const char* state_name, const float* actions, int32_t n);

// what both lap calls ask of the handle and of the tracker; the wrapper is the caller's to check
int check_waypoint_run(const QuadHandle* h, const char* who, const QuadWaypointRun* wr);

// What quad_policy_episode / quad_policy_waypoints and their quad_actor_* forms ask of the wrapper, the run and
// the image, after the entry point's own handle checks, and the flattened arguments. who: the entry point the
// messages name (the message is built only on failure); lap_traces: the lap call's own traces are requested.
int policy_run_args(const QuadHandle* h, const float* packed, const QuadPolicyRun* r, bool lap_traces,
                    EpisodeArgs* out, const char* who);

// The whole argument check and the flattened arguments of quad_policy_episode (and quad_actor_episode,
// quad_pop_attach_eval) and of quad_policy_waypoints (and quad_actor_waypoints); policy_episode.hip
namespace pop {
int episode_args(const QuadHandle* h, const float* packed, const QuadPolicyRun* r, EpisodeArgs* out,
                 const char* who = "quad_policy_episode");
}
int waypoints_args(const QuadHandle* h, const float* packed, const QuadPolicyRun* r, const QuadWaypointRun* wr,
                   EpisodeArgs* out, const char* who);

}  // namespace quadenv
