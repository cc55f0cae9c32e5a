// quad_pid.h -- the reference's cascaded PID control law as a __host__ __device__ function.
//
// One call of CascadedPIDController.compute:
//   QUAD_PID_YAW_FRAME    pid_controller.py:99-191
//   QUAD_PID_WORLD_FRAME  pid_controller_world_frame.py:179-283
// in float64 on the float32 state and target words, cast to float32 and clipped to [-1, 1] at the
// end like the reference (np.array(..., dtype=np.float32), np.clip). The operation order is the
// reference's; np.clip / Python's max / min keep their NaN behaviour (clipn and the selects below).
// k_ctrl_act and k_ctrl_episode (ctrl.hip) and the host shim (tests/native_pid) instantiate this one
// function, so under -ffp-contract=on the two kernels compute the same bits.
#pragma once

#include "quad_physics.h"

namespace quadenv {

// The plant constants of the law the handle's QuadCfg holds (drone_config.py's names in comments);
// MASS travels with the gain set.
struct PidPlant {
  double g;           // G = -gravity[2]
  double dt;          // DT = timestep
  double max_thrust;  // MAX_TOTAL_THRUST = 4 max_motor_thrust
  double max_torque;  // MAX_TORQUE
  double arm;         // ARM_LENGTH
  double inertia[3];  // IXX, IYY, IZZ
};
inline PidPlant make_pid_plant(const QuadCfg& c) {
  return PidPlant{-c.gravity[2], c.timestep, 4.0 * c.max_motor_thrust, c.max_torque, c.arm_length,
                  {c.inertia[0], c.inertia[1], c.inertia[2]}};
}
// pid_gains.json (the reference's committed values) and drone_config.py MASS
inline void pid_default_gains_fill(QuadPidGains* g) {
  g->kp_xy = 4.0; g->kd_xy = 3.5; g->ki_xy = 0.25;
  g->kp_z = 6.0; g->kd_z = 6.5; g->ki_z = 0.8;
  g->kp_att = 180.0; g->kd_att = 26.0;
  g->kp_yaw = 80.0; g->kd_yaw = 30.0;
  g->ki_rate_torque = 0.025; g->rate_int_max = 0.01;
  g->axy_max = 4.5; g->az_min = -5.0; g->az_max = 12.0; g->tilt_max = 0.25;
  g->z_int_max = 2.0; g->xy_int_max = 0.4;
  g->torque_motor_frac = 0.7; g->torque_abs_max = 0.05; g->yaw_torque_scale = 0.6;
  g->mass = 0.2227;
}

// integ: xy integral 2, z integral, rate-torque integral 3 (read and updated). diag (nullptr to
// skip): des_rate 3, des_att 3.
template <int MODE>
QD_HD void pid_law(const QuadPidGains& G, const PidPlant& P, const float s[12], const float t[9], double integ[6],
                   float act[4], double* diag) {
  constexpr bool WORLD = MODE == QUAD_PID_WORLD_FRAME;
  const double PI = 3.14159265358979323846;
  const double pos[3] = {double(s[0]), double(s[1]), double(s[2])};
  const double roll = double(s[3]), pitch = double(s[4]), yaw = double(s[5]);
  const double vel[3] = {double(s[6]), double(s[7]), double(s[8])};
  const double w[3] = {double(s[9]), double(s[10]), double(s[11])};
  // 1. position PID -> desired acceleration (world frame)
  const double pe[3] = {double(t[0]) - pos[0], double(t[1]) - pos[1], double(t[2]) - pos[2]};
  const double kidt = G.ki_xy * P.dt;
  integ[0] = clipn(integ[0] + kidt * pe[0], -G.xy_int_max, G.xy_int_max);
  integ[1] = clipn(integ[1] + kidt * pe[1], -G.xy_int_max, G.xy_int_max);
  double ax, ay, az;
  if (WORLD) {
    ax = G.kp_xy * pe[0] + G.kd_xy * (double(t[3]) - vel[0]) + integ[0];
    ay = G.kp_xy * pe[1] + G.kd_xy * (double(t[4]) - vel[1]) + integ[1];
    az = G.kp_z * pe[2] + G.kd_z * (double(t[5]) - vel[2]);
  } else {
    ax = G.kp_xy * pe[0] - G.kd_xy * vel[0] + integ[0];
    ay = G.kp_xy * pe[1] - G.kd_xy * vel[1] + integ[1];
    az = G.kp_z * pe[2] - G.kd_z * vel[2];
  }
  integ[2] = clipn(integ[2] + G.ki_z * P.dt * pe[2], -G.z_int_max, G.z_int_max);
  az += integ[2];
  if (WORLD) {
    ax += double(t[6]); ay += double(t[7]); az += double(t[8]);
  }
  ax = clipn(ax, -G.axy_max, G.axy_max);
  ay = clipn(ay, -G.axy_max, G.axy_max);
  az = clipn(az, G.az_min, G.az_max);
  // 2. acceleration -> thrust + desired attitude
  double sr, cr, sp, cp, sy, cy;
  q_sincos(roll, &sr, &cr);
  q_sincos(pitch, &sp, &cp);
  q_sincos(yaw, &sy, &cy);
  const double crcp = cr * cp;
  const double tilt = 0.5 > crcp ? 0.5 : crcp;  // max(cos_r * cos_p, 0.5)
  const double thrust = clipn(G.mass * (P.g + az) / tilt, 0.0, P.max_thrust);
  const double mt_motor = thrust / 4.0 * 2.0 * P.arm * G.torque_motor_frac;
  const double max_tau = G.torque_abs_max < mt_motor ? G.torque_abs_max : mt_motor;  // min(., torque_abs_max)
  double ax_b, ay_b;
  if (WORLD) {  // R(roll, pitch, yaw)^T (ax, ay, az), euler_to_rot_matrix's Z-Y-X entries
    ax_b = (cy * cp) * ax + (sy * cp) * ay + (-sp) * az;
    ay_b = (cy * sp * sr - sy * cr) * ax + (sy * sp * sr + cy * cr) * ay + (cp * sr) * az;
  } else {
    ax_b = cy * ax + sy * ay;
    ay_b = -sy * ax + cy * ay;
  }
  const double des_pitch = clipn(q_atan2(ax_b, P.g + az), -G.tilt_max, G.tilt_max);
  const double des_roll = clipn(q_atan2(-ay_b, P.g + az), -G.tilt_max, G.tilt_max);
  // 3. attitude P -> desired rates, rate PI -> torques
  const double ka = G.kp_att / G.kd_att, ky = G.kp_yaw / G.kd_yaw;
  double des[3], des_yaw;
  des[0] = ka * (des_roll - roll);
  des[1] = ka * (des_pitch - pitch);
  if (WORLD) {
    const double tvx = double(t[3]), tvy = double(t[4]);
    const double vn = q_sqrt(tvx * tvx + tvy * tvy);
    des_yaw = vn > 1e-6 ? q_atan2(tvy, tvx) : yaw;
    // angle_diff: (target - source + pi) % (2 pi) - pi with Python's sign-of-the-divisor remainder
    double m = fmod(des_yaw - yaw + PI, 2.0 * PI);
    if (m < 0.0) m += 2.0 * PI;
    des[2] = ky * (m - PI);
  } else {
    des_yaw = 0.0;
    des[2] = ky * (0.0 - yaw);
  }
  const double kd[3] = {G.kd_att, G.kd_att, G.kd_yaw};
  const double kidr = G.ki_rate_torque * P.dt;
  double tau[3];
#pragma unroll
  for (int j = 0; j < 3; j++) {
    const double re = des[j] - w[j];
    const double tau_p = P.inertia[j] * kd[j] * re;
    integ[3 + j] = clipn(integ[3 + j] + kidr * re, -G.rate_int_max, G.rate_int_max);
    tau[j] = tau_p + integ[3 + j];
  }
  const double lim_z = max_tau * G.yaw_torque_scale;
  tau[0] = clipn(tau[0], -max_tau, max_tau);
  tau[1] = clipn(tau[1], -max_tau, max_tau);
  tau[2] = clipn(tau[2], -lim_z, lim_z);
  // 4. normalize, cast, clip
  const float a[4] = {float(2.0 * thrust / P.max_thrust - 1.0), float(tau[0] / P.max_torque),
                      float(tau[1] / P.max_torque), float(tau[2] / P.max_torque)};
#pragma unroll
  for (int j = 0; j < 4; j++) act[j] = clipn(a[j], -1.0f, 1.0f);
  if (diag) {
    diag[0] = des[0]; diag[1] = des[1]; diag[2] = des[2];
    diag[3] = des_roll; diag[4] = des_pitch; diag[5] = des_yaw;
  }
}

// Per-env episode metrics of auto_tune_pid.py:66-124, accumulated step by step (QuadPidMetrics).
struct PidAcc {
  double total_reward = 0.0;
  double pe_sum = 0.0, pe_sq = 0.0, pe_max = 0.0;
  double yr_abs_sum = 0.0, yr_sum = 0.0, yr_sq = 0.0, yr_abs_max = 0.0, yr_delta = 0.0;
  int32_t sign_changes = 0;
  float prev_yr = 0.f;
  int32_t steps = 0;
};
// np.sign
QD_HD int sign_of(float x) { return x > 0.f ? 1 : (x < 0.f ? -1 : 0); }
// after a step: pos = info["state"][:3], tgt = the target the law read before the step
QD_HD void pid_acc_step(PidAcc& m, const float s12[12], const float tgt[3], float reward) {
#pragma clang fp contract(off)
  // np.linalg.norm(drone_pos - tgt_pos): float32 difference; squares summed in order, float64
  const double d0 = double(sub32(s12[0], tgt[0])), d1 = double(sub32(s12[1], tgt[1])), d2 = double(sub32(s12[2], tgt[2]));
  const double pe = sqrt((d0 * d0 + d1 * d1) + d2 * d2);
  m.total_reward += double(reward);
  m.pe_sum += pe;
  m.pe_sq += pe * pe;
  m.pe_max = pe > m.pe_max ? pe : m.pe_max;
  const float yr = s12[11];
  const double y = double(yr), ya = fabs(y);
  m.yr_abs_sum += ya;
  m.yr_sum += y;
  m.yr_sq += y * y;
  m.yr_abs_max = ya > m.yr_abs_max ? ya : m.yr_abs_max;
  if (m.steps > 0) {
    m.sign_changes += sign_of(yr) != sign_of(m.prev_yr) ? 1 : 0;
    m.yr_delta += fabs(y - double(m.prev_yr));
  }
  m.prev_yr = yr;
  m.steps += 1;
}

// env i's QuadPidMetrics entries, once, at the end of a fused run (the controller and the policy episode kernels)
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
// the metric status of a waypoint tracker's status: lap -> QUAD_PID_LAP, terminated / truncated -> their codes
__device__ __forceinline__ int32_t metric_status_of(int32_t tracker_status) {
  return tracker_status == 1 ? QUAD_PID_LAP
                             : (tracker_status == 2 ? QUAD_PID_TERMINATED
                                                    : (tracker_status == 3 ? QUAD_PID_TRUNCATED : QUAD_PID_RUNNING));
}

}  // namespace quadenv
