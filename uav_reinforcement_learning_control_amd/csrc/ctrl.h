// ctrl.h -- host-side entries of the controller kernels (ctrl.hip), called by quad_pid_act / quad_pid_episode /
// quad_target_info and quad_ctrl_act / quad_ctrl_episode / quad_ctrl_waypoints (quadenv.hip), the way
// quad_rollout reaches rollout.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "env_tiles.h"
#include "quad_ctrl.h"

namespace quadenv {

// k_ctrl_act<QuadPidGains, mode> over n rows: integ [6][n], diag [n,6]
hipError_t launch_pid_act(const PidPlant& plant, const QuadPidGains* gains, int32_t n_sets, const int32_t* set_of,
                          int32_t mode, const float* state12, const float* target9, int32_t n, double* integ,
                          float* actions, double* diag, hipStream_t s);

// k_ctrl_act<QuadCtrlParams, law> over n rows: state [8][n], diag [n,7]
hipError_t launch_ctrl_act(const PidPlant& plant, const QuadCtrlParams* params, int32_t n_sets, const int32_t* set_of,
                           int32_t law, const float* state12, const float* target9, int32_t n, double* state,
                           float* actions, double* diag, hipStream_t s);

// k_ctrl_episode<row type, env_kind, mode or law, spec> over all envs of kp
hipError_t launch_pid_episode(const KConsts<float>* kc, const KParams& kp, int env_kind, bool spec,
                              const PidPlant& plant, const QuadPidRun& r, hipStream_t s);
hipError_t launch_ctrl_episode(const KConsts<float>* kc, const KParams& kp, int env_kind, bool spec,
                               const PidPlant& plant, const QuadCtrlRun& r, hipStream_t s);

// k_ctrl_waypoints<law, spec> over all envs of kp (hover kind)
hipError_t launch_ctrl_waypoints(const KConsts<float>* kc, const KParams& kp, bool spec, const PidPlant& plant,
                                 const QuadCtrlRun& r, const QuadWaypointRun& wr, hipStream_t s);

// k_target_info<env_kind> over all envs of kp
hipError_t launch_target_info(const KConsts<float>* kc, const KParams& kp, int env_kind, float* target_info,
                              hipStream_t s);

}  // namespace quadenv
