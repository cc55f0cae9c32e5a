// quad_waypoints.h -- the waypoint-lap bookkeeping of the reference's evaluate_trajectory
// (evaluate.py:487-497 start, :539-590 per step), as __host__ __device__ functions.
//
//   wp_begin    the start: position = waypoint 0, target = waypoint 1 % n, tracker zeroed
//   wp_update   one pass of the loop body after env.step: reward, step count, switch within
//               reach_radius, lap, terminated, truncated
//
// The distance is np.linalg.norm(drone_pos - current_target) on a float32 position and a float64
// waypoint: float64 differences, squares summed in axis order, one sqrt, without contraction.
// k_waypoints_begin / k_waypoints_update (quadenv.hip), the fused lap kernels (ctrl.hip,
// policy_episode.hip) and the host shim (tests/native_waypoints) instantiate these two functions.
#pragma once

#include <cmath>
#include <cstdint>

#include "../../include/quadenv.h"
#include "quad_physics.h"

namespace quadenv {

// one env's row of QuadWaypointState. status: 0 running, 1 lap completed, 2 terminated, 3 truncated
struct WpTrack {
  int32_t wp_idx, reached, laps, steps, status;
  double total_reward;
};

// row i of the caller's tracker arrays
QD_HD WpTrack load_track(const QuadWaypointState& s, int i) {
  return WpTrack{s.wp_idx[i], s.reached[i], s.laps[i], s.steps[i], s.status[i], s.total_reward[i]};
}
QD_HD void store_track(const QuadWaypointState& s, int i, const WpTrack& t) {
  s.wp_idx[i] = t.wp_idx;
  s.reached[i] = t.reached;
  s.laps[i] = t.laps;
  s.steps[i] = t.steps;
  s.status[i] = t.status;
  s.total_reward[i] = t.total_reward;
}

// wp: the env's set [cnt][3], cnt >= 1. pos0: the start position, tgt: the first target, both
// waypoints[k].astype(np.float32)
QD_HD void wp_begin(const double* wp, int cnt, WpTrack& t, float pos0[3], float tgt[3]) {
  const int nxt = 1 % cnt;
#pragma unroll
  for (int j = 0; j < 3; j++) {
    pos0[j] = float(wp[j]);
    tgt[j] = float(wp[3 * nxt + j]);
  }
  t.wp_idx = nxt;
  t.reached = 0;
  t.laps = 0;
  t.steps = 0;
  t.status = 0;
  t.total_reward = 0.0;
}

// One step of a running env (t.status == 0; the caller skips the others). pos: the step's
// state12[0:3]. Returns true when the env target is to be overwritten with tgt (a switch that does
// not end the lap); the lap wins over terminated, which wins over truncated.
QD_HD bool wp_update(const double* wp, int cnt, float reach_radius, const float pos[3], float reward, bool term,
                     bool trunc, WpTrack& t, float tgt[3]) {
#pragma clang fp contract(off)
  t.total_reward += double(reward);
  t.steps += 1;
  int k = t.wp_idx;
  double d2 = 0.0;
#pragma unroll
  for (int j = 0; j < 3; j++) {
    const double d = double(pos[j]) - wp[3 * k + j];
    d2 += d * d;
  }
  int status = 0;
  bool sw = false;
  if (sqrt(d2) < double(reach_radius)) {
    t.reached += 1;
    k = (k + 1) % cnt;
    t.wp_idx = k;
    if (k == 0) {
      t.laps += 1;
      status = 1;
    } else {
      sw = true;
#pragma unroll
      for (int j = 0; j < 3; j++) tgt[j] = float(wp[3 * k + j]);
    }
  }
  if (status == 0 && term) status = 2;
  else if (status == 0 && trunc) status = 3;
  t.status = status;
  return sw;
}

}  // namespace quadenv
