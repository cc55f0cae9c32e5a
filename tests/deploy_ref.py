"""Numpy restatement of the reference's deployed observation path (TEST INFRASTRUCTURE ONLY).

``VelEstRef.update`` is one ``VelocityEstimator.update`` (state_estimator.py:27-57) in float64;
``build_obs`` is one ``build_observation`` (observation_builder.py:32-58): a float32 vector, the env's
normalisation in float32, then a clip to [-1, 1]. Written independently of csrc/quad_deploy.h (plain numpy,
the reference's operation order); both are held to the same bars against tests/golden/golden_deploy.npz.
"""
import numpy as np

# envs/hover_env.py:33-36, the bounds the builder copies
OBS_LOW = np.array([-4, -4, -2, -np.pi, -np.pi, -np.pi, -10, -10, -10, -6 * np.pi, -6 * np.pi, -6 * np.pi], np.float32)
OBS_HIGH = -OBS_LOW


class VelEstRef:
    """state = (prev_pos 3, prev_time, velocity 3, has_prev), the product's block layout."""

    def __init__(self, alpha=0.8, max_dt=0.1):
        self.alpha, self.max_dt = float(alpha), float(max_dt)
        self.prev_pos = np.zeros(3)
        self.prev_time = 0.0
        self.vel = np.zeros(3)
        self.has_prev = False
        self.branches = {"first": 0, "bad_dt": 0, "filter": 0}

    def update(self, pos, t):
        pos = np.asarray(pos, np.float64)
        t = float(t)
        with np.errstate(all="ignore"):
            if not self.has_prev:
                self.branches["first"] += 1
                self.vel = np.zeros(3)
            else:
                dt = t - self.prev_time
                if dt <= 0 or dt > self.max_dt:
                    self.branches["bad_dt"] += 1
                    self.vel = np.zeros(3)
                else:
                    self.branches["filter"] += 1
                    raw = (pos - self.prev_pos) / dt
                    self.vel = self.alpha * self.vel + (1.0 - self.alpha) * raw
        self.prev_pos, self.prev_time, self.has_prev = pos.copy(), t, True
        return self.vel.copy()

    def state(self):
        return np.concatenate([self.prev_pos, [self.prev_time], self.vel, [1.0 if self.has_prev else 0.0]])


def build_obs(drone_pos, target_pos, attitude, linear_vel, angular_vel, low=OBS_LOW, high=OBS_HIGH):
    """Inputs of any float type; the position difference is formed in float32 (the product's sub32)."""
    x = np.zeros(12, np.float32)
    with np.errstate(all="ignore"):
        x[0:3] = np.asarray(target_pos, np.float32) - np.asarray(drone_pos, np.float32)
        x[3:6] = np.asarray(attitude, np.float64)
        x[6:9] = np.asarray(linear_vel, np.float64)
        x[9:12] = np.asarray(angular_vel, np.float64)
        y = np.float32(2.0) * (x - low) / (high - low) - np.float32(1.0)
        return np.clip(y, np.float32(-1.0), np.float32(1.0)).astype(np.float32)


def vel_err_sq(state12_trace, pos0, alpha, dt, max_dt=0.1, step0=0):
    """sum over the steps of |v_est - v_true|^2 for one env: state12_trace [T,12] (after each step), pos0 the
    position the estimator saw before the first action at step count step0. Returns (sum, velocities [T,3])."""
    est = VelEstRef(alpha, max_dt)
    est.update(np.asarray(pos0, np.float32).astype(np.float64), step0 * dt)
    total, vs = 0.0, []
    for k, s in enumerate(np.asarray(state12_trace, np.float32)):
        v = est.update(s[0:3].astype(np.float64), (step0 + k + 1) * dt)
        d = v - s[6:9].astype(np.float64)
        total += (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        vs.append(v)
    return total, np.array(vs).reshape(-1, 3)
