// quad_deploy.h -- the observation the reference's deployed policy sees (ros2_ws policy_node.py), as
// __host__ __device__ functions.
//
//   vel_est_update   one VelocityEstimator.update(position, timestamp)   state_estimator.py:27-57
//   deploy_obs       one build_observation(...)                           observation_builder.py:32-58
//
// The node does not hand the policy the env's observation: the linear velocity is a first-order low-pass
// on finite differences of the mocap position, and the normalised vector is clipped to [-1, 1]. The
// estimator runs in float64 on the float32 position words (the node's float64 arrays), in the reference's
// operation order and without contraction; the builder is the env's own float32 normalisation
// (norm_obs1) followed by np.clip. k_deploy_obs and k_policy_episode (policy_episode.hip) and the host
// shim (tests/native_deploy) instantiate these two functions.
#pragma once

#include "quad_physics.h"

namespace quadenv {

constexpr int EST_NSTATE = 8;  // prev_pos 3, prev_time, velocity 3, has_prev (0 / 1)

// st: the estimator's state (read and updated); vel: the velocity update() returns
QD_HD void vel_est_update(double alpha, double max_dt, const float pos[3], double timestamp, double st[EST_NSTATE],
                          double vel[3]) {
#pragma clang fp contract(off)
  const double p[3] = {double(pos[0]), double(pos[1]), double(pos[2])};
  const double dt = timestamp - st[3];
  // no previous sample, or an invalid dt (a NaN dt fails both compares and is used, as in Python)
  const bool restart = !(st[7] != 0.0) || dt <= 0.0 || dt > max_dt;
  const double one_m = 1.0 - alpha;
#pragma unroll
  for (int j = 0; j < 3; j++) {
    const double raw = (p[j] - st[j]) / dt;
    const double v = alpha * st[4 + j] + one_m * raw;
    st[4 + j] = restart ? 0.0 : v;
    st[j] = p[j];
    vel[j] = st[4 + j];
  }
  st[3] = timestamp;
  st[7] = 1.0;
}

// s12: the QuadState vector (position, attitude, linear and angular velocity); vel: the estimator's
// velocity, which replaces s12[6:9]; lo / span / rspan: the handle's observation bounds (KConsts)
QD_HD void deploy_obs(const float lo[12], const float span[12], const float rspan[12], const float s12[12],
                      const float target[3], const double vel[3], float obs[12]) {
#pragma unroll
  for (int i = 0; i < 12; i++) {
    const float x = i < 3 ? sub32(target[i], s12[i]) : (i >= 6 && i < 9 ? float(vel[i - 6]) : s12[i]);
    const float y = norm_obs1(x, lo[i], span[i], rspan[i]);
    // norm_obs1's constant division turns an infinite 2 (x - lo) into NaN; NumPy's quotient stays infinite
    // and the clip lands it on +-1 (the env never normalises such a state: it has terminated)
    const float v = (y != y && x == x) ? (x > 0.f ? 1.0f : -1.0f) : y;
    obs[i] = clipn(v, -1.0f, 1.0f);
  }
}

}  // namespace quadenv
