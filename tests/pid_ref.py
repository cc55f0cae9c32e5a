"""Float64 numpy restatement of the reference's two cascaded PID laws (TEST INFRASTRUCTURE ONLY).

``PidRef.compute`` is one call of ``CascadedPIDController.compute``:
  mode 0 (yaw frame)   pid_controller.py:99-191
  mode 1 (world frame) pid_controller_world_frame.py:179-283
in float64 on float32 inputs, with the float32 cast and the [-1, 1] clip at the end. Written
independently of csrc/quad_pid.h (plain numpy, the reference's operation order); both are held to
the same bars against tests/golden/golden_pid.npz.
"""
import json
import os

import numpy as np

YAW_FRAME, WORLD_FRAME = 0, 1
GAINS_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pid_gains.json")

# utils/drone_config.py
PLANT = dict(mass=0.2227, g=9.81, dt=0.01, max_total_thrust=52.0, max_torque=0.5, arm_length=0.039799,
             inertia=(4.16e-4, 4.23e-4, 5.37e-4))

# the 21 numbers the constructor reads, in QuadPidGains order: (json section, json key)
FIELDS = (("position_xy", "kp"), ("position_xy", "kd"), ("position_xy", "ki"),
          ("position_z", "kp"), ("position_z", "kd"), ("position_z", "ki"),
          ("attitude", "kp"), ("attitude", "kd"), ("yaw", "kp"), ("yaw", "kd"),
          ("rate", "ki_torque"), ("rate", "integral_max"),
          ("limits", "axy_max"), ("limits", "az_min"), ("limits", "az_max"), ("limits", "tilt_max"),
          ("limits", "z_integral_max"), ("limits", "xy_integral_max"), ("limits", "torque_motor_fraction"),
          ("limits", "torque_abs_max"), ("limits", "yaw_torque_scale"))


def load_gains(path=GAINS_JSON):
    return json.load(open(path))


def gains_vector(g) -> np.ndarray:
    return np.array([float(g[s][k]) for s, k in FIELDS], np.float64)


class PidRef:
    """integ = [xy_x, xy_y, z, rate_x, rate_y, rate_z] (the device law's integrator order)."""

    def __init__(self, gains=None, mode=YAW_FRAME, plant=None):
        self.g = gains if gains is not None else load_gains()
        self.mode = mode
        self.p = dict(PLANT, **(plant or {}))
        self.integ = np.zeros(6, np.float64)

    def reset(self):
        self.integ[:] = 0.0

    def compute(self, state, target9):
        g, p = self.g, self.p
        s = np.asarray(state, np.float32).astype(np.float64)
        t = np.asarray(target9, np.float32).astype(np.float64)
        if t.size == 3:
            t = np.concatenate([t, np.zeros(6)])
        pos, (roll, pitch, yaw), vel, (wx, wy, wz) = s[0:3], s[3:6], s[6:9], s[9:12]
        tp, tv, ta = t[0:3], t[3:6], t[6:9]
        xy, z, lim = g["position_xy"], g["position_z"], g["limits"]
        dt, G = p["dt"], p["g"]
        world = self.mode == WORLD_FRAME
        pe = tp - pos
        self.integ[0:2] = np.clip(self.integ[0:2] + xy["ki"] * dt * pe[:2], -lim["xy_integral_max"],
                                  lim["xy_integral_max"])
        if world:
            ax = xy["kp"] * pe[0] + xy["kd"] * (tv[0] - vel[0]) + self.integ[0]
            ay = xy["kp"] * pe[1] + xy["kd"] * (tv[1] - vel[1]) + self.integ[1]
            az = z["kp"] * pe[2] + z["kd"] * (tv[2] - vel[2])
        else:
            ax = xy["kp"] * pe[0] - xy["kd"] * vel[0] + self.integ[0]
            ay = xy["kp"] * pe[1] - xy["kd"] * vel[1] + self.integ[1]
            az = z["kp"] * pe[2] - z["kd"] * vel[2]
        self.integ[2] = np.clip(self.integ[2] + z["ki"] * dt * pe[2], -lim["z_integral_max"], lim["z_integral_max"])
        az += self.integ[2]
        if world:
            ax += ta[0]; ay += ta[1]; az += ta[2]
        ax = np.clip(ax, -lim["axy_max"], lim["axy_max"])
        ay = np.clip(ay, -lim["axy_max"], lim["axy_max"])
        az = np.clip(az, lim["az_min"], lim["az_max"])
        tilt = max(np.cos(roll) * np.cos(pitch), 0.5)
        thrust = np.clip(p["mass"] * (G + az) / tilt, 0.0, p["max_total_thrust"])
        max_tau = min(thrust / 4.0 * 2.0 * p["arm_length"] * lim["torque_motor_fraction"], lim["torque_abs_max"])
        cy, sy = np.cos(yaw), np.sin(yaw)
        if world:
            cr, sr, cp, sp = np.cos(roll), np.sin(roll), np.cos(pitch), np.sin(pitch)
            R = np.array([[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr],
                          [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
                          [-sp, cp * sr, cp * cr]], np.float64)
            ax_b, ay_b, _ = R.T @ np.array([ax, ay, az])
        else:
            ax_b = cy * ax + sy * ay
            ay_b = -sy * ax + cy * ay
        des_pitch = np.clip(np.arctan2(ax_b, G + az), -lim["tilt_max"], lim["tilt_max"])
        des_roll = np.clip(np.arctan2(-ay_b, G + az), -lim["tilt_max"], lim["tilt_max"])
        ka = g["attitude"]["kp"] / g["attitude"]["kd"]
        ky = g["yaw"]["kp"] / g["yaw"]["kd"]
        des_wx = ka * (des_roll - roll)
        des_wy = ka * (des_pitch - pitch)
        if world:
            des_yaw = np.arctan2(tv[1], tv[0]) if np.linalg.norm(tv[:2]) > 1e-6 else yaw
            des_wz = ky * ((des_yaw - yaw + np.pi) % (2.0 * np.pi) - np.pi)
        else:
            des_yaw = 0.0
            des_wz = ky * (0.0 - yaw)
        rate_err = np.array([des_wx - wx, des_wy - wy, des_wz - wz])
        kd = np.array([g["attitude"]["kd"], g["attitude"]["kd"], g["yaw"]["kd"]])
        tau_p = np.array(p["inertia"]) * kd * rate_err
        self.integ[3:6] = np.clip(self.integ[3:6] + g["rate"]["ki_torque"] * dt * rate_err,
                                  -g["rate"]["integral_max"], g["rate"]["integral_max"])
        tau = tau_p + self.integ[3:6]
        tau[0] = np.clip(tau[0], -max_tau, max_tau)
        tau[1] = np.clip(tau[1], -max_tau, max_tau)
        tau[2] = np.clip(tau[2], -max_tau * lim["yaw_torque_scale"], max_tau * lim["yaw_torque_scale"])
        action = np.array([2.0 * thrust / p["max_total_thrust"] - 1.0, tau[0] / p["max_torque"],
                           tau[1] / p["max_torque"], tau[2] / p["max_torque"]], np.float32)
        diag = np.array([des_wx, des_wy, des_wz, des_roll, des_pitch, des_yaw], np.float64)
        return np.clip(action, -1.0, 1.0), diag
