// quad_ctrl.h -- the reference's SE(3), sliding-mode and LQR control laws as __host__ __device__
// functions, beside the cascaded PID of quad_pid.h.
//
// One call of the reference class's compute():
//   QUAD_CTRL_SE3  se3_geometric_controller.py:247-426   SE3GeometricController
//   QUAD_CTRL_SMC  smc_controller_world_frame.py:146-322 (its class is also named CascadedPIDController)
//   QUAD_CTRL_LQR  lqr_controller_world_frame.py:139-289 (likewise)
// in float64 on the float32 state and target words, cast to float32 and clipped to [-1, 1] at the end.
// The operation order is the reference's, with np.clip / Python's max / min NaN behaviour (clipn and the
// selects). The reference computes every intermediate as a rounded Python / NumPy float64, so the laws
// are built with floating-point contraction off: no a*b+c is fused, on the host or on the device.
// Quirks are restated, not repaired: SE(3)'s np.linalg.qr sign flip, its unused yaw gains;
// SMC's xy integral that is updated and never read; LQR's ay reading xy_integral[0].
//
// cs[8]: xy integral 2, z integral, rate-torque integral 3 (quad_pid.h's order), v_yaw, des_wz_prev.
// Rows 6-7 belong to SMC alone; the other laws neither read nor write them.
// diag (nullptr to skip) [7]: des_rate 3, des_att 3, |e_R| (SE(3); 0 for the others).
#pragma once

#include "quad_pid.h"

namespace quadenv {

constexpr int CTRL_NSTATE = QUAD_CTRL_NSTATE;
constexpr int CTRL_NDIAG = QUAD_CTRL_NDIAG;

inline void ctrl_default_params_fill(QuadCtrlParams* p) {
  pid_default_gains_fill(&p->base);
  // control.lqr(A, B, I3, I1), A = [[0,1,0],[0,0,0],[1,0,0]], B = [0,1,0]^T
  // (lqr_controller_world_frame.py:129): K = [1 + sqrt 2, 1 + sqrt 2, 1] in closed form
  p->lqr_k[0] = 1.0 + sqrt(2.0); p->lqr_k[1] = 1.0 + sqrt(2.0); p->lqr_k[2] = 1.0;
  // smc_controller_world_frame.py:124-130
  p->yaw_stw_k1 = 1.2; p->yaw_stw_k2 = 2.0; p->yaw_stw_boundary = 0.05;
  p->yaw_deadband = 1.0 * (3.14159265358979323846 / 180.0);  // np.deg2rad(1.0)
  p->yaw_v_int_max = 2.0; p->yaw_rate_max = 3.0; p->yaw_rate_lpf_alpha = 0.2;
  p->se3_reorthonormalize = 1.0;
}

struct CtrlIn {
  double pos[3], roll, pitch, yaw, vel[3], w[3], tp[3], tv[3], ta[3];
};
QD_HD CtrlIn ctrl_in(const float s[12], const float t[9]) {
  CtrlIn i;
#pragma unroll
  for (int j = 0; j < 3; j++) {
    i.pos[j] = double(s[j]); i.vel[j] = double(s[6 + j]); i.w[j] = double(s[9 + j]);
    i.tp[j] = double(t[j]); i.tv[j] = double(t[3 + j]); i.ta[j] = double(t[6 + j]);
  }
  i.roll = double(s[3]); i.pitch = double(s[4]); i.yaw = double(s[5]);
  return i;
}

// angle_diff: (target - source + pi) % (2 pi) - pi with Python's sign-of-the-divisor remainder
QD_HD double ctrl_angle_diff(double target, double source) {
#pragma clang fp contract(off)
  const double PI = 3.14159265358979323846;
  double m = fmod(target - source + PI, 2.0 * PI);
  if (m < 0.0) m += 2.0 * PI;
  return m - PI;
}
// the trajectory tangent's heading, or the current yaw below 1e-6 of target speed
QD_HD double ctrl_des_yaw(const CtrlIn& I) {
#pragma clang fp contract(off)
  const double vn = sqrt(I.tv[0] * I.tv[0] + I.tv[1] * I.tv[1]);
  return vn > 1e-6 ? atan2(I.tv[1], I.tv[0]) : I.yaw;
}

// np.clip = minimum(maximum(x, lo), hi) with bounds that may be NaN (the torque limit follows the thrust): NaN
// if any of the three is, where clipn keeps a finite x
QD_HD double clip_nanb(double x, double lo, double hi) {
  const double a = (x >= lo || x != x) ? x : lo;
  return (a <= hi || a != a) ? a : hi;
}

// rate PI -> torque clip -> normalize, cast, clip: the tail all three laws share
// (kd: the P gain per axis; thrust: the clipped total thrust)
QD_HD void ctrl_rate_tail(const QuadPidGains& G, const PidPlant& P, const CtrlIn& I, const double des[3],
                          const double kd[3], double thrust, double cs[CTRL_NSTATE], float act[4]) {
#pragma clang fp contract(off)
  const double mt_motor = thrust / 4.0 * 2.0 * P.arm * G.torque_motor_frac;
  const double max_tau = G.torque_abs_max < mt_motor ? G.torque_abs_max : mt_motor;  // min(., torque_abs_max)
  const double kidr = G.ki_rate_torque * P.dt;
  double tau[3];
#pragma unroll
  for (int j = 0; j < 3; j++) {
    const double re = des[j] - I.w[j];
    const double tau_p = P.inertia[j] * kd[j] * re;
    cs[3 + j] = clipn(cs[3 + j] + kidr * re, -G.rate_int_max, G.rate_int_max);
    tau[j] = tau_p + cs[3 + j];
  }
  const double lim_z = max_tau * G.yaw_torque_scale;
  tau[0] = clip_nanb(tau[0], -max_tau, max_tau);
  tau[1] = clip_nanb(tau[1], -max_tau, max_tau);
  tau[2] = clip_nanb(tau[2], -lim_z, lim_z);
  const float a[4] = {float(2.0 * thrust / P.max_thrust - 1.0), float(tau[0] / P.max_torque),
                      float(tau[1] / P.max_torque), float(tau[2] / P.max_torque)};
#pragma unroll
  for (int j = 0; j < 4; j++) act[j] = clipn(a[j], -1.0f, 1.0f);
}

// acceleration (clipped, world frame) -> thrust, desired roll / pitch, their rate commands: the
// middle of the world-frame cascade (smc :236-262, lqr :215-241)
QD_HD void ctrl_accel_to_att(const QuadPidGains& G, const PidPlant& P, const CtrlIn& I, double ax, double ay, double az,
                             double* thrust, double des[3], double datt[3]) {
#pragma clang fp contract(off)
  double sr, cr, sp, cp, sy, cy;
  q_sincos(I.roll, &sr, &cr);
  q_sincos(I.pitch, &sp, &cp);
  q_sincos(I.yaw, &sy, &cy);
  const double crcp = cr * cp;
  const double tilt = 0.5 > crcp ? 0.5 : crcp;  // max(cos_r * cos_p, 0.5)
  *thrust = clipn(G.mass * (P.g + az) / tilt, 0.0, P.max_thrust);
  // R(roll, pitch, yaw)^T (ax, ay, az)
  const double ax_b = (cy * cp) * ax + (sy * cp) * ay + (-sp) * az;
  const double ay_b = (cy * sp * sr - sy * cr) * ax + (sy * sp * sr + cy * cr) * ay + (cp * sr) * az;
  datt[1] = clipn(atan2(ax_b, P.g + az), -G.tilt_max, G.tilt_max);   // des_pitch
  datt[0] = clipn(atan2(-ay_b, P.g + az), -G.tilt_max, G.tilt_max);  // des_roll
  const double ka = G.kp_att / G.kd_att;
  des[0] = ka * (datt[0] - I.roll);
  des[1] = ka * (datt[1] - I.pitch);
}

// np.linalg.qr's Q of the 3x3 matrix with columns x, y, z, as LAPACK computes it (dgeqr2 + dorg2r):
// two Householder reflectors with dlarfg's beta = -sign(alpha) norm, so the column signs are NumPy's;
// the third reflector of a square matrix is the identity (tau = 0). Q depends on the reflectors alone,
// which x and y fix (z enters R only). q: row-major Q.
QD_HD double ctrl_lapy2(double x, double y) {
#pragma clang fp contract(off)
  const double xa = fabs(x), ya = fabs(y);
  const double w = xa > ya ? xa : ya, z = xa > ya ? ya : xa;
  if (z == 0.0) return w;
  const double r = z / w;
  return w * sqrt(1.0 + r * r);
}
QD_HD void ctrl_qr_q(const double x[3], const double y[3], double q[9]) {
#pragma clang fp contract(off)
  // reflector 1 on column x
  double tau1 = 0.0, v12 = x[1], v13 = x[2];
  const double n1 = sqrt(x[1] * x[1] + x[2] * x[2]);
  if (!(n1 == 0.0)) {
    const double beta = -copysign(ctrl_lapy2(x[0], n1), x[0]);
    tau1 = (beta - x[0]) / beta;
    const double s = 1.0 / (x[0] - beta);
    v12 = x[1] * s; v13 = x[2] * s;
  }
  // H1 applied to column y, rows 2-3 (row 1 goes to R and is not needed)
  double a22 = y[1], a32 = y[2];
  if (!(tau1 == 0.0)) {
    const double w = y[0] + y[1] * v12 + y[2] * v13;
    const double t = -tau1 * w;
    a22 = a22 + v12 * t;
    a32 = a32 + v13 * t;
  }
  // reflector 2 on (a22, a32)
  double tau2 = 0.0, v23 = a32;
  const double n2 = fabs(a32);
  if (!(n2 == 0.0)) {
    const double beta = -copysign(ctrl_lapy2(a22, n2), a22);
    tau2 = (beta - a22) / beta;
    v23 = a32 * (1.0 / (a22 - beta));
  }
  // dorg2r, i = 3: column 3 = e3. i = 2: H2 on rows 2-3 of column 3, then column 2
  double q13 = 0.0, q23 = 0.0, q33 = 1.0;
  if (!(tau2 == 0.0)) {
    const double w = q23 + q33 * v23;
    const double t = -tau2 * w;
    q23 = q23 + t;
    q33 = q33 + v23 * t;
  }
  double q12 = 0.0, q22 = 1.0 - tau2, q32 = -tau2 * v23;
  // i = 1: H1 on columns 2-3, then column 1
  if (!(tau1 == 0.0)) {
    const double w2 = q12 + q22 * v12 + q32 * v13;
    const double t2 = -tau1 * w2;
    q12 = q12 + t2; q22 = q22 + v12 * t2; q32 = q32 + v13 * t2;
    const double w3 = q13 + q23 * v12 + q33 * v13;
    const double t3 = -tau1 * w3;
    q13 = q13 + t3; q23 = q23 + v12 * t3; q33 = q33 + v13 * t3;
  }
  q[0] = 1.0 - tau1; q[3] = -tau1 * v12; q[6] = -tau1 * v13;
  q[1] = q12; q[4] = q22; q[7] = q32;
  q[2] = q13; q[5] = q23; q[8] = q33;
}

// ---- QUAD_CTRL_SE3
QD_HD void se3_law(const QuadCtrlParams& C, const PidPlant& P, const float s[12], const float t[9],
                   double cs[CTRL_NSTATE], float act[4], double* diag) {
#pragma clang fp contract(off)
  const QuadPidGains& G = C.base;
  const CtrlIn I = ctrl_in(s, t);
  double sr, cr, sp, cp, sy, cy;
  q_sincos(I.roll, &sr, &cr);
  q_sincos(I.pitch, &sp, &cp);
  q_sincos(I.yaw, &sy, &cy);
  // R_current, euler_to_rot_matrix's Z-Y-X entries
  const double a00 = cy * cp, a01 = cy * sp * sr - sy * cr, a02 = cy * sp * cr + sy * sr;
  const double a10 = sy * cp, a11 = sy * sp * sr + cy * cr, a12 = sy * sp * cr - cy * sr;
  const double a20 = -sp, a21 = cp * sr, a22 = cp * cr;
  // 1. position control (world frame)
  const double pe[3] = {I.tp[0] - I.pos[0], I.tp[1] - I.pos[1], I.tp[2] - I.pos[2]};
  const double ve[3] = {I.tv[0] - I.vel[0], I.tv[1] - I.vel[1], I.tv[2] - I.vel[2]};
  const double kidt = G.ki_xy * P.dt;
  cs[0] = clipn(cs[0] + kidt * pe[0], -G.xy_int_max, G.xy_int_max);
  cs[1] = clipn(cs[1] + kidt * pe[1], -G.xy_int_max, G.xy_int_max);
  double ax = G.kp_xy * pe[0] + G.kd_xy * ve[0] + cs[0];
  double ay = G.kp_xy * pe[1] + G.kd_xy * ve[1] + cs[1];
  cs[2] = clipn(cs[2] + G.ki_z * P.dt * pe[2], -G.z_int_max, G.z_int_max);
  double az = G.kp_z * pe[2] + G.kd_z * ve[2] + cs[2];
  ax += I.ta[0]; ay += I.ta[1]; az += I.ta[2];
  ax = clipn(ax, -G.axy_max, G.axy_max);
  ay = clipn(ay, -G.axy_max, G.axy_max);
  az = clipn(az, G.az_min, G.az_max);
  // 2. desired rotation from the thrust vector and the yaw
  const double f0 = G.mass * (ax + 0.0), f1 = G.mass * (ay + 0.0), f2 = G.mass * (az + P.g);
  const double mag = clipn(sqrt(f0 * f0 + f1 * f1 + f2 * f2), 0.1, P.max_thrust);
  const double zd_den = mag + 1e-10;
  const double zd[3] = {f0 / zd_den, f1 / zd_den, f2 / zd_den};
  const double des_yaw = ctrl_des_yaw(I);
  const double cdy = cos(des_yaw), sdy = sin(des_yaw);
  // y_d = z_d x (cos, sin, 0); np.cross: each component is one product minus another
  double yd[3] = {zd[1] * 0.0 - zd[2] * sdy, zd[2] * cdy - zd[0] * 0.0, zd[0] * sdy - zd[1] * cdy};
  const double yn = sqrt(yd[0] * yd[0] + yd[1] * yd[1] + yd[2] * yd[2]);
  if (yn < 1e-3) {
    yd[0] = 0.0; yd[1] = 0.0; yd[2] = 1.0;
  } else {
    yd[0] /= yn; yd[1] /= yn; yd[2] /= yn;
  }
  double xd[3] = {yd[1] * zd[2] - yd[2] * zd[1], yd[2] * zd[0] - yd[0] * zd[2], yd[0] * zd[1] - yd[1] * zd[0]};
  const double xn = sqrt(xd[0] * xd[0] + xd[1] * xd[1] + xd[2] * xd[2]);
  if (xn < 1e-3) {
    xd[0] = 1.0; xd[1] = 0.0; xd[2] = 0.0;
  } else {
    xd[0] /= xn; xd[1] /= xn; xd[2] /= xn;
  }
  // R_desired = [x_d y_d z_d], then np.linalg.qr and the det < 0 branch (:369-371); scalars d_rc
  double d00 = xd[0], d01 = yd[0], d02 = zd[0], d10 = xd[1], d11 = yd[1], d12 = zd[1], d20 = xd[2], d21 = yd[2],
         d22 = zd[2];
  if (C.se3_reorthonormalize != 0.0) {
    double q[9];
    ctrl_qr_q(xd, yd, q);
    d00 = q[0]; d01 = q[1]; d02 = q[2]; d10 = q[3]; d11 = q[4]; d12 = q[5]; d20 = q[6]; d21 = q[7]; d22 = q[8];
    const double det = d00 * (d11 * d22 - d12 * d21) - d01 * (d10 * d22 - d12 * d20) + d02 * (d10 * d21 - d11 * d20);
    if (det < 0.0) {  // Householder Q of a 3x3 has det +1: never taken
      d00 = -d00; d01 = -d01; d02 = -d02; d10 = -d10; d11 = -d11; d12 = -d12; d20 = -d20; d21 = -d21; d22 = -d22;
    }
  }
  // 3. attitude_error_so3: R_e = R_d^T R_a; e_R = -1/2 vee(R_e - R_e^T)
  const double e21 = d02 * a01 + d12 * a11 + d22 * a21, e12 = d01 * a02 + d11 * a12 + d21 * a22;
  const double e02 = d00 * a02 + d10 * a12 + d20 * a22, e20 = d02 * a00 + d12 * a10 + d22 * a20;
  const double e10 = d01 * a00 + d11 * a10 + d21 * a20, e01 = d00 * a01 + d10 * a11 + d20 * a21;
  const double eR[3] = {-0.5 * (e21 - e12), -0.5 * (e02 - e20), -0.5 * (e10 - e01)};
  const double ka = G.kp_att / G.kd_att;
  const double des[3] = {ka * eR[0], ka * eR[1], ka * eR[2]};  // all three axes; kp_yaw / kd_yaw unused
  // 4. rate control, 5. normalize
  const double kd[3] = {G.kd_att, G.kd_att, G.kd_att};
  ctrl_rate_tail(G, P, I, des, kd, mag, cs, act);
  if (diag) {
    diag[0] = des[0]; diag[1] = des[1]; diag[2] = des[2];
    // rot_matrix_to_euler(R_desired)
    const double dp = asin(-d20);
    if (fabs(cos(dp)) > 1e-6) {
      diag[3] = atan2(d21, d22);
      diag[5] = atan2(d10, d00);
    } else {  // gimbal lock
      diag[3] = 0.0;
      diag[5] = atan2(-d01, d11);
    }
    diag[4] = dp;
    diag[6] = sqrt(eR[0] * eR[0] + eR[1] * eR[1] + eR[2] * eR[2]);
  }
}

// ---- QUAD_CTRL_SMC
QD_HD void smc_law(const QuadCtrlParams& C, const PidPlant& P, const float s[12], const float t[9],
                   double cs[CTRL_NSTATE], float act[4], double* diag) {
#pragma clang fp contract(off)
  const double PI = 3.14159265358979323846;
  const QuadPidGains& G = C.base;
  const CtrlIn I = ctrl_in(s, t);
  const double pe[3] = {I.tp[0] - I.pos[0], I.tp[1] - I.pos[1], I.tp[2] - I.pos[2]};
  const double kidt = G.ki_xy * P.dt;
  cs[0] = clipn(cs[0] + kidt * pe[0], -G.xy_int_max, G.xy_int_max);  // updated, never read (:195-198)
  cs[1] = clipn(cs[1] + kidt * pe[1], -G.xy_int_max, G.xy_int_max);
  // sliding surfaces s = e + 1 * edot, smoothed sign 2/pi atan(s * 1)
  const double sx = pe[0] + 1.0 * (I.tv[0] - I.vel[0]);
  const double sy = pe[1] + 1.0 * (I.tv[1] - I.vel[1]);
  const double sz = pe[2] + 1.0 * (I.tv[2] - I.vel[2]);
  double ax = G.axy_max * (2.0 / PI * atan(sx * 1.0));
  double ay = G.axy_max * (2.0 / PI * atan(sy * 1.0));
  double az = G.az_max * (2.0 / PI * atan(sz * 1.0));
  cs[2] = clipn(cs[2] + G.ki_z * P.dt * pe[2], -G.z_int_max, G.z_int_max);
  az += cs[2];
  ax += I.ta[0]; ay += I.ta[1]; az += I.ta[2];
  ax = clipn(ax, -G.axy_max, G.axy_max);
  ay = clipn(ay, -G.axy_max, G.axy_max);
  az = clipn(az, G.az_min, G.az_max);
  double thrust, des[3], datt[3];
  ctrl_accel_to_att(G, P, I, ax, ay, az, &thrust, des, datt);
  // super-twisting yaw loop (:264-286)
  datt[2] = ctrl_des_yaw(I);
  const double yaw_err = ctrl_angle_diff(datt[2], I.yaw);
  const double eff = fabs(yaw_err) < C.yaw_deadband ? 0.0 : yaw_err;
  const double sgn = 2.0 / PI * atan(eff / C.yaw_stw_boundary);
  const double v_dot = C.yaw_stw_k2 * sgn;
  cs[6] = clipn(cs[6] + v_dot * P.dt, -C.yaw_v_int_max, C.yaw_v_int_max);
  const double raw = C.yaw_stw_k1 * sqrt(fabs(eff)) * sgn + cs[6];
  const double wz = (1.0 - C.yaw_rate_lpf_alpha) * cs[7] + C.yaw_rate_lpf_alpha * raw;
  des[2] = clipn(wz, -C.yaw_rate_max, C.yaw_rate_max);
  cs[7] = des[2];
  const double kd[3] = {G.kd_att, G.kd_att, G.kd_yaw};
  ctrl_rate_tail(G, P, I, des, kd, thrust, cs, act);
  if (diag) {
    diag[0] = des[0]; diag[1] = des[1]; diag[2] = des[2];
    diag[3] = datt[0]; diag[4] = datt[1]; diag[5] = datt[2];
    diag[6] = 0.0;
  }
}

// ---- QUAD_CTRL_LQR
QD_HD void lqr_law(const QuadCtrlParams& C, const PidPlant& P, const float s[12], const float t[9],
                   double cs[CTRL_NSTATE], float act[4], double* diag) {
#pragma clang fp contract(off)
  const QuadPidGains& G = C.base;
  const CtrlIn I = ctrl_in(s, t);
  const double pe[3] = {I.tp[0] - I.pos[0], I.tp[1] - I.pos[1], I.tp[2] - I.pos[2]};
  const double kidt = G.ki_xy * P.dt;
  cs[0] = clipn(cs[0] + kidt * pe[0], -G.xy_int_max, G.xy_int_max);
  cs[1] = clipn(cs[1] + kidt * pe[1], -G.xy_int_max, G.xy_int_max);
  const double k0 = C.lqr_k[0], k1 = C.lqr_k[1], k2 = C.lqr_k[2];
  double ax = k0 * pe[0] + k1 * (I.tv[0] - I.vel[0]) + cs[0] * k2;
  double ay = k0 * pe[1] + k1 * (I.tv[1] - I.vel[1]) + cs[0] * k2;  // xy_integral[0], as :195 has it
  double az = k0 * pe[2] + k1 * (I.tv[2] - I.vel[2]);
  cs[2] = clipn(cs[2] + G.ki_z * P.dt * pe[2], -G.z_int_max, G.z_int_max);
  az += cs[2] * k2;
  ax += I.ta[0]; ay += I.ta[1]; az += I.ta[2];
  ax = clipn(ax, -G.axy_max, G.axy_max);
  ay = clipn(ay, -G.axy_max, G.axy_max);
  az = clipn(az, G.az_min, G.az_max);
  double thrust, des[3], datt[3];
  ctrl_accel_to_att(G, P, I, ax, ay, az, &thrust, des, datt);
  datt[2] = ctrl_des_yaw(I);
  des[2] = (G.kp_yaw / G.kd_yaw) * ctrl_angle_diff(datt[2], I.yaw);
  const double kd[3] = {G.kd_att, G.kd_att, G.kd_yaw};
  ctrl_rate_tail(G, P, I, des, kd, thrust, cs, act);
  if (diag) {
    diag[0] = des[0]; diag[1] = des[1]; diag[2] = des[2];
    diag[3] = datt[0]; diag[4] = datt[1]; diag[5] = datt[2];
    diag[6] = 0.0;
  }
}

// One law by its QUAD_CTRL_* id; the two PID ids call pid_law, so the family is a superset of quad_pid.h.
template <int LAW>
QD_HD void ctrl_law(const QuadCtrlParams& C, const PidPlant& P, const float s[12], const float t[9],
                    double cs[CTRL_NSTATE], float act[4], double* diag) {
  if constexpr (LAW == QUAD_CTRL_SE3) {
    se3_law(C, P, s, t, cs, act, diag);
  } else if constexpr (LAW == QUAD_CTRL_SMC) {
    smc_law(C, P, s, t, cs, act, diag);
  } else if constexpr (LAW == QUAD_CTRL_LQR) {
    lqr_law(C, P, s, t, cs, act, diag);
  } else {
    static_assert(LAW == QUAD_CTRL_PID_YAW || LAW == QUAD_CTRL_PID_WORLD, "unknown law");
    pid_law<LAW == QUAD_CTRL_PID_WORLD ? QUAD_PID_WORLD_FRAME : QUAD_PID_YAW_FRAME>(C.base, P, s, t, cs, act, diag);
    if (diag) diag[6] = 0.0;
  }
}

}  // namespace quadenv
