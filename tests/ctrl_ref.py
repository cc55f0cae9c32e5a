"""Float64 numpy restatement of the reference's SE(3), sliding-mode and LQR laws (TEST INFRASTRUCTURE ONLY).

``CtrlRef.compute`` is one call of the reference class's ``compute``:
  "se3"  se3_geometric_controller.py:247-426
  "smc"  smc_controller_world_frame.py:146-322
  "lqr"  lqr_controller_world_frame.py:139-289
in float64 on float32 inputs, with the float32 cast and the [-1, 1] clip at the end. Written independently
of csrc/quad_ctrl.h (plain numpy, the reference's operation order); both are held to the same bars
against tests/golden/golden_ctrl.npz. ``householder_q`` is np.linalg.qr's Q of a 3x3 matrix written out
(LAPACK's dgeqr2 + dorg2r); it does not call np.linalg.qr.

state = [xy_x, xy_y, z, rate_x, rate_y, rate_z, v_yaw, des_wz_prev] (the device block's row order).

After a call ``margin_branch`` is the distance of that call from the nearest discontinuity of the law (the
sign of x_d[0] under np.linalg.qr, the two 1e-3 norm fallbacks, the 1e-6 target-speed switch, the yaw wrap,
the SMC deadband) and ``margin_all`` also counts the clip edges of the integrators, v_yaw and des_wz. The
fixture generator keeps its call samples 1e-3 away from all of them and marks where an episode comes
within 1e-4 of a discontinuity.
"""
import numpy as np

from pid_ref import PLANT, load_gains

SMC_DEFAULTS = dict(yaw_stw_k1=1.2, yaw_stw_k2=2.0, yaw_stw_boundary=0.05, yaw_deadband=float(np.deg2rad(1.0)),
                    yaw_v_int_max=2.0, yaw_rate_max=3.0, yaw_rate_lpf_alpha=0.2)
LQR_K = (1.0 + np.sqrt(2.0), 1.0 + np.sqrt(2.0), 1.0)


def _lapy2(x, y):
    """dlapy2: sqrt(x^2 + y^2) as w sqrt(1 + (z / w)^2)."""
    xa, ya = abs(x), abs(y)
    w, z = (xa, ya) if xa > ya else (ya, xa)
    if z == 0.0:
        return w
    return w * np.sqrt(1.0 + (z / w) ** 2)


def _larfg(alpha, x):
    """dlarfg: (tau, v_tail) of the reflector that maps (alpha, x) to (beta, 0), beta = -sign(alpha) norm."""
    xnorm = np.sqrt(np.sum(x * x)) if len(x) > 1 else abs(x[0])
    if xnorm == 0.0:
        return 0.0, x.copy()
    beta = -np.copysign(_lapy2(alpha, xnorm), alpha)
    return (beta - alpha) / beta, x * (1.0 / (alpha - beta))


def householder_q(A) -> np.ndarray:
    """Q of np.linalg.qr(A) for a 3x3 A, column signs included."""
    A = np.array(A, np.float64)
    tau1, v1 = _larfg(A[0, 0], A[1:, 0])
    v1 = np.concatenate([[1.0], v1])
    if tau1 != 0.0:
        A[:, 1:] = A[:, 1:] + np.outer(v1, -tau1 * (A[:, 1:].T @ v1))
    tau2, v2 = _larfg(A[1, 1], A[2:, 1])
    v2 = np.concatenate([[1.0], v2])
    Q = np.eye(3)
    # dorg2r: apply H2 then H1 to the identity's trailing columns
    if tau2 != 0.0:
        Q[1:, 2:] = Q[1:, 2:] + np.outer(v2, -tau2 * (Q[1:, 2:].T @ v2))
    Q[1:, 1] = -tau2 * v2
    Q[1, 1] = 1.0 - tau2
    if tau1 != 0.0:
        Q[:, 1:] = Q[:, 1:] + np.outer(v1, -tau1 * (Q[:, 1:].T @ v1))
    Q[:, 0] = -tau1 * v1
    Q[0, 0] = 1.0 - tau1
    return Q


def _rot(roll, pitch, yaw):
    cr, sr, cp, sp, cy, sy = np.cos(roll), np.sin(roll), np.cos(pitch), np.sin(pitch), np.cos(yaw), np.sin(yaw)
    return np.array([[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr],
                     [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
                     [-sp, cp * sr, cp * cr]], np.float64)


def _norm(v):
    return np.sqrt(np.sum(np.asarray(v) ** 2))


class CtrlRef:
    def __init__(self, law, gains=None, plant=None, lqr_k=LQR_K, smc=None, se3_reorthonormalize=True):
        assert law in ("se3", "smc", "lqr")
        self.law = law
        self.g = gains if gains is not None else load_gains()
        self.p = dict(PLANT, **(plant or {}))
        self.K = tuple(float(k) for k in lqr_k)
        self.smc = dict(SMC_DEFAULTS, **(smc or {}))
        self.reortho = bool(se3_reorthonormalize)
        self.state = np.zeros(8, np.float64)

    def reset(self):
        self.state[:] = 0.0

    def compute(self, state, target9):
        with np.errstate(all="ignore"):
            return self._compute(state, target9)

    def _edge(self, pre, lim):
        """a value about to be clipped to [-lim, lim]"""
        self._clip_m.append(abs(abs(pre) - lim))

    def _compute(self, state, target9):
        g, p, st = self.g, self.p, self.state
        self._clip_m, br = [], []
        s = np.asarray(state, np.float32).astype(np.float64)
        t = np.asarray(target9, np.float32).astype(np.float64)
        if t.size == 3:
            t = np.concatenate([t, np.zeros(6)])
        pos, (roll, pitch, yaw), vel, w = s[0:3], s[3:6], s[6:9], s[9:12]
        tp, tv, ta = t[0:3], t[3:6], t[6:9]
        xy, z, lim = g["position_xy"], g["position_z"], g["limits"]
        dt, G = p["dt"], p["g"]
        ka = g["attitude"]["kp"] / g["attitude"]["kd"]
        pe = tp - pos
        ve = tv - vel
        for v in st[0:2] + xy["ki"] * dt * pe[:2]:
            self._edge(v, lim["xy_integral_max"])
        self._edge(st[2] + z["ki"] * dt * pe[2], lim["z_integral_max"])
        st[0:2] = np.clip(st[0:2] + xy["ki"] * dt * pe[:2], -lim["xy_integral_max"], lim["xy_integral_max"])
        if self.law == "se3":
            ax = xy["kp"] * pe[0] + xy["kd"] * ve[0] + st[0]
            ay = xy["kp"] * pe[1] + xy["kd"] * ve[1] + st[1]
            st[2] = np.clip(st[2] + z["ki"] * dt * pe[2], -lim["z_integral_max"], lim["z_integral_max"])
            az = z["kp"] * pe[2] + z["kd"] * ve[2] + st[2]
        elif self.law == "smc":
            ax = lim["axy_max"] * (2 / np.pi * np.arctan(pe[0] + 1 * ve[0]))
            ay = lim["axy_max"] * (2 / np.pi * np.arctan(pe[1] + 1 * ve[1]))
            az = lim["az_max"] * (2 / np.pi * np.arctan(pe[2] + 1 * ve[2]))
            st[2] = np.clip(st[2] + z["ki"] * dt * pe[2], -lim["z_integral_max"], lim["z_integral_max"])
            az += st[2]
        else:
            K = self.K
            ax = K[0] * pe[0] + K[1] * ve[0] + st[0] * K[2]
            ay = K[0] * pe[1] + K[1] * ve[1] + st[0] * K[2]
            az = K[0] * pe[2] + K[1] * ve[2]
            st[2] = np.clip(st[2] + z["ki"] * dt * pe[2], -lim["z_integral_max"], lim["z_integral_max"])
            az += st[2] * K[2]
        ax += ta[0]; ay += ta[1]; az += ta[2]
        ax = np.clip(ax, -lim["axy_max"], lim["axy_max"])
        ay = np.clip(ay, -lim["axy_max"], lim["axy_max"])
        az = np.clip(az, lim["az_min"], lim["az_max"])
        des_yaw = np.arctan2(tv[1], tv[0]) if _norm(tv[:2]) > 1e-6 else yaw
        if _norm(tv[:2]) != 0.0:  # an exactly zero target velocity (hover) never crosses the switch
            br.append(abs(_norm(tv[:2]) - 1e-6))
        R = _rot(roll, pitch, yaw)
        err_norm = 0.0
        if self.law == "se3":
            f = p["mass"] * (np.array([ax, ay, az]) + np.array([0.0, 0.0, G]))
            thrust = np.clip(_norm(f), 0.1, p["max_total_thrust"])
            zd = f / (thrust + 1e-10)
            xw = np.array([np.cos(des_yaw), np.sin(des_yaw), 0.0])
            yd = np.cross(zd, xw)
            yn = _norm(yd)
            br.append(abs(yn - 1e-3))
            yd = np.array([0.0, 0.0, 1.0]) if yn < 1e-3 else yd / yn
            xd = np.cross(yd, zd)
            xn = _norm(xd)
            br.append(abs(xn - 1e-3))
            xd = np.array([1.0, 0.0, 0.0]) if xn < 1e-3 else xd / xn
            self.xd0 = float(xd[0])
            Rd = np.column_stack([xd, yd, zd])
            if self.reortho:
                br.append(abs(xd[0]))
                Rd = householder_q(Rd)
                if np.linalg.det(Rd) < 0:
                    Rd = -Rd
            Re = Rd.T @ R
            E = Re - Re.T
            eR = -0.5 * np.array([E[2, 1], E[0, 2], E[1, 0]])
            des = ka * eR
            kd = np.array([g["attitude"]["kd"]] * 3)
            dpitch = np.arcsin(-Rd[2, 0])
            if np.abs(np.cos(dpitch)) > 1e-6:
                datt = np.array([np.arctan2(Rd[2, 1], Rd[2, 2]), dpitch, np.arctan2(Rd[1, 0], Rd[0, 0])])
            else:
                datt = np.array([0.0, dpitch, np.arctan2(-Rd[0, 1], Rd[1, 1])])
            err_norm = _norm(eR)
        else:
            tilt = max(np.cos(roll) * np.cos(pitch), 0.5)
            thrust = np.clip(p["mass"] * (G + az) / tilt, 0.0, p["max_total_thrust"])
            ax_b, ay_b, _ = R.T @ np.array([ax, ay, az])
            des_pitch = np.clip(np.arctan2(ax_b, G + az), -lim["tilt_max"], lim["tilt_max"])
            des_roll = np.clip(np.arctan2(-ay_b, G + az), -lim["tilt_max"], lim["tilt_max"])
            yaw_err = (des_yaw - yaw + np.pi) % (2.0 * np.pi) - np.pi
            br.append(abs(abs(yaw_err) - np.pi))
            if self.law == "smc":
                c = self.smc
                eff = 0.0 if np.abs(yaw_err) < c["yaw_deadband"] else yaw_err
                br.append(abs(abs(yaw_err) - c["yaw_deadband"]))
                sgn = 2.0 / np.pi * np.arctan(eff / c["yaw_stw_boundary"])
                self._edge(st[6] + c["yaw_stw_k2"] * sgn * dt, c["yaw_v_int_max"])
                st[6] = np.clip(st[6] + c["yaw_stw_k2"] * sgn * dt, -c["yaw_v_int_max"], c["yaw_v_int_max"])
                raw = c["yaw_stw_k1"] * np.sqrt(np.abs(eff)) * sgn + st[6]
                des_wz = (1.0 - c["yaw_rate_lpf_alpha"]) * st[7] + c["yaw_rate_lpf_alpha"] * raw
                self._edge(des_wz, c["yaw_rate_max"])
                des_wz = np.clip(des_wz, -c["yaw_rate_max"], c["yaw_rate_max"])
                st[7] = des_wz
            else:
                des_wz = (g["yaw"]["kp"] / g["yaw"]["kd"]) * yaw_err
            des = np.array([ka * (des_roll - roll), ka * (des_pitch - pitch), des_wz])
            kd = np.array([g["attitude"]["kd"], g["attitude"]["kd"], g["yaw"]["kd"]])
            datt = np.array([des_roll, des_pitch, des_yaw])
        max_tau = min(thrust / 4.0 * 2.0 * p["arm_length"] * lim["torque_motor_fraction"], lim["torque_abs_max"])
        rate_err = des - w
        tau_p = np.array(p["inertia"]) * kd * rate_err
        for v in st[3:6] + g["rate"]["ki_torque"] * dt * rate_err:
            self._edge(v, g["rate"]["integral_max"])
        self.margin_branch = min(br) if br else np.inf
        self.margin_all = min(br + self._clip_m)
        st[3:6] = np.clip(st[3:6] + g["rate"]["ki_torque"] * dt * rate_err, -g["rate"]["integral_max"],
                          g["rate"]["integral_max"])
        tau = tau_p + st[3:6]
        tau[0] = np.clip(tau[0], -max_tau, max_tau)
        tau[1] = np.clip(tau[1], -max_tau, max_tau)
        tau[2] = np.clip(tau[2], -max_tau * lim["yaw_torque_scale"], max_tau * lim["yaw_torque_scale"])
        action = np.array([2.0 * thrust / p["max_total_thrust"] - 1.0, tau[0] / p["max_torque"],
                           tau[1] / p["max_torque"], tau[2] / p["max_torque"]], np.float32)
        diag = np.concatenate([des, datt, [err_norm]]).astype(np.float64)
        return np.clip(action, -1.0, 1.0), diag


def from_params(law, cp) -> CtrlRef:
    """CtrlRef for a controllers.CtrlParams."""
    return CtrlRef(law, cp.to_dict(), plant={"mass": cp.mass}, lqr_k=(cp.lqr_k0, cp.lqr_k1, cp.lqr_k2),
                   smc={k: getattr(cp, k) for k in SMC_DEFAULTS}, se3_reorthonormalize=cp.se3_reorthonormalize != 0.0)
