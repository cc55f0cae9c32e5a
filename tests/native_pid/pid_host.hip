// TEST INFRASTRUCTURE ONLY: the product's control law (csrc/quad_pid.h) instantiated on the host
// behind a C interface, so the CPU suite checks the very function the kernels inline.
#include "../../include/quadenv.h"
#include "../../uav_reinforcement_learning_control_amd/csrc/quad_model.h"
#include "../../uav_reinforcement_learning_control_amd/csrc/quad_pid.h"

using namespace quadenv;

extern "C" {

void host_pid_default_gains(QuadPidGains* g) { pid_default_gains_fill(g); }

// n calls with one gain set, the integrators (integ[6]) carried from call to call.
// state12 [n,12], target9 [n,9] -> actions [n,4], diag [n,6], integ_out [n,6] (after each call)
int host_pid_calls(const QuadCfg* cfg, const QuadPidGains* g, int mode, const float* state12, const float* target9,
                   int n, double* integ, float* actions, double* diag, double* integ_out) {
  if (mode != QUAD_PID_YAW_FRAME && mode != QUAD_PID_WORLD_FRAME) return -1;
  const PidPlant P = make_pid_plant(*cfg);
  for (int i = 0; i < n; i++) {
    if (mode == QUAD_PID_WORLD_FRAME)
      pid_law<QUAD_PID_WORLD_FRAME>(*g, P, state12 + 12 * i, target9 + 9 * i, integ, actions + 4 * i, diag + 6 * i);
    else
      pid_law<QUAD_PID_YAW_FRAME>(*g, P, state12 + 12 * i, target9 + 9 * i, integ, actions + 4 * i, diag + 6 * i);
    for (int j = 0; j < 6; j++) integ_out[6 * i + j] = integ[j];
  }
  return 0;
}

}  // extern "C"
