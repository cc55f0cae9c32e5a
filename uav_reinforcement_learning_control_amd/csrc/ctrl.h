// ctrl.h -- host-side entries of the controller-family kernels (ctrl.hip), called by quad_ctrl_act /
// quad_ctrl_episode (quadenv.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "env_tiles.h"
#include "quad_ctrl.h"

namespace quadenv {

// k_ctrl_act<law> over n rows
hipError_t launch_ctrl_act(const PidPlant& plant, const QuadCtrlParams* params, int32_t n_sets, const int32_t* set_of,
                           int32_t law, const float* state12, const float* target9, int32_t n, double* state,
                           float* actions, double* diag, hipStream_t s);

// k_ctrl_episode<env_kind, law, spec> over all envs of kp
hipError_t launch_ctrl_episode(const KConsts<float>* kc, const KParams& kp, int env_kind, bool spec,
                               const PidPlant& plant, const QuadCtrlRun& r, hipStream_t s);

// k_ctrl_waypoints<law, spec> over all envs of kp (hover kind)
hipError_t launch_ctrl_waypoints(const KConsts<float>* kc, const KParams& kp, bool spec, const PidPlant& plant,
                                 const QuadCtrlRun& r, const QuadWaypointRun& wr, hipStream_t s);

}  // namespace quadenv
