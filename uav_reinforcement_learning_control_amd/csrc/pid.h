// pid.h -- host-side entries of the PID kernels (pid.hip), called by quad_pid_act / quad_pid_episode /
// quad_target_info (quadenv.hip), the way quad_rollout reaches rollout.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "env_tiles.h"
#include "quad_pid.h"

namespace quadenv {

// k_pid_act over n rows
hipError_t launch_pid_act(const PidPlant& plant, const QuadPidGains* gains, int32_t n_sets, const int32_t* set_of,
                          int32_t mode, const float* state12, const float* target9, int32_t n, double* integ,
                          float* actions, double* diag, hipStream_t s);

// k_pid_episode<env_kind, mode, spec> over all envs of kp
hipError_t launch_pid_episode(const KConsts<float>* kc, const KParams& kp, int env_kind, bool spec,
                              const PidPlant& plant, const QuadPidRun& r, hipStream_t s);

// k_target_info<env_kind> over all envs of kp
hipError_t launch_target_info(const KConsts<float>* kc, const KParams& kp, int env_kind, float* target_info,
                              hipStream_t s);

}  // namespace quadenv
