"""Batched cascaded-PID baseline (the reference's pid_controller.py / pid_controller_world_frame.py).

  * ``PIDGains``      one gain set: the 21 numbers ``CascadedPIDController.__init__`` reads from
                      ``pid_gains.json`` (+ MASS), with ``from_json`` / ``to_json`` in that file's layout,
                      so tuned gains drop into the reference.
  * ``gain_table``    gain sets stacked into the device table the kernels index per env.
  * ``pid_act``       the law alone (``quad_pid_act``): the building block of host loops.
  * ``pid_episode``   the fused closed loop (``quad_pid_episode``): every env runs law -> env step until
                      it terminates, truncates or ``max_steps`` pass; per-env metrics as tensors.
  * ``pid_score``     ``compute_performance_score`` (auto_tune_pid.py:127-157), vectorised.

  * ``CtrlParams``    one parameter set of the controller family (the reference's SE(3), sliding-mode and
                      LQR controllers beside the PID): ``PIDGains`` plus the LQR gain row, the seven
                      super-twisting constants and ``se3_reorthonormalize``.
  * ``ctrl_act`` / ``ctrl_episode``  ``pid_act`` / ``pid_episode`` for any law of ``LAWS``
                      (``quad_ctrl_act`` / ``quad_ctrl_episode``).

  * ``ctrl_waypoints``  waypoint laps for any law in one launch (``quad_ctrl_waypoints``): the course of
                      ``waypoints.WaypointCourse`` after its ``begin``.

``QuadVecEnv.pid_act`` / ``pid_episode`` / ``ctrl_act`` / ``ctrl_episode`` are these functions bound as methods.
"""
from __future__ import annotations

import ctypes as C
import json
from dataclasses import dataclass, fields
from typing import Optional, Sequence, Union

import numpy as np
import torch

from . import _native as N

MODES = {"yaw_frame": N.PID_YAW_FRAME, "pid_controller": N.PID_YAW_FRAME, N.PID_YAW_FRAME: N.PID_YAW_FRAME,
         "world_frame": N.PID_WORLD_FRAME, "pid_controller_world_frame": N.PID_WORLD_FRAME,
         N.PID_WORLD_FRAME: N.PID_WORLD_FRAME}
STATUS = {N.PID_RUNNING: "running", N.PID_TERMINATED: "terminated", N.PID_TRUNCATED: "truncated",
          N.PID_INVALID: "invalid", N.PID_LAP: "lap"}

# field -> (pid_gains.json section, key), in QuadPidGains order
_JSON = (("kp_xy", "position_xy", "kp"), ("kd_xy", "position_xy", "kd"), ("ki_xy", "position_xy", "ki"),
         ("kp_z", "position_z", "kp"), ("kd_z", "position_z", "kd"), ("ki_z", "position_z", "ki"),
         ("kp_att", "attitude", "kp"), ("kd_att", "attitude", "kd"), ("kp_yaw", "yaw", "kp"), ("kd_yaw", "yaw", "kd"),
         ("ki_rate_torque", "rate", "ki_torque"), ("rate_int_max", "rate", "integral_max"),
         ("axy_max", "limits", "axy_max"), ("az_min", "limits", "az_min"), ("az_max", "limits", "az_max"),
         ("tilt_max", "limits", "tilt_max"), ("z_int_max", "limits", "z_integral_max"),
         ("xy_int_max", "limits", "xy_integral_max"), ("torque_motor_frac", "limits", "torque_motor_fraction"),
         ("torque_abs_max", "limits", "torque_abs_max"), ("yaw_torque_scale", "limits", "yaw_torque_scale"),
         ("mass", "drone_params", "mass_kg"))


@dataclass
class PIDGains:
    """Defaults: the reference's committed pid_gains.json and drone_config.py MASS."""
    kp_xy: float = 4.0
    kd_xy: float = 3.5
    ki_xy: float = 0.25
    kp_z: float = 6.0
    kd_z: float = 6.5
    ki_z: float = 0.8
    kp_att: float = 180.0
    kd_att: float = 26.0
    kp_yaw: float = 80.0
    kd_yaw: float = 30.0
    ki_rate_torque: float = 0.025
    rate_int_max: float = 0.01
    axy_max: float = 4.5
    az_min: float = -5.0
    az_max: float = 12.0
    tilt_max: float = 0.25
    z_int_max: float = 2.0
    xy_int_max: float = 0.4
    torque_motor_frac: float = 0.7
    torque_abs_max: float = 0.05
    yaw_torque_scale: float = 0.6
    mass: float = 0.2227

    @classmethod
    def from_dict(cls, d: dict) -> "PIDGains":
        g = cls()
        for f, sec, key in _JSON:
            if sec in d and key in d[sec]:
                setattr(g, f, float(d[sec][key]))
        return g

    @classmethod
    def from_json(cls, path: str) -> "PIDGains":
        with open(path) as fh:
            return cls.from_dict(json.load(fh))

    def to_dict(self, notes: Optional[dict] = None) -> dict:
        d: dict = {}
        for f, sec, key in _JSON:
            d.setdefault(sec, {})[key] = float(getattr(self, f))
        if notes:
            d["tuning_notes"] = notes
        return d

    def to_json(self, path: str, notes: Optional[dict] = None) -> None:
        """pid_gains.json's layout: CascadedPIDController(json.load(open(path))) accepts it."""
        with open(path, "w") as fh:
            json.dump(self.to_dict(notes), fh, indent=2)

    def vector(self) -> np.ndarray:
        return np.array([getattr(self, f) for f in N.PID_GAIN_FIELDS], np.float64)


assert tuple(f.name for f in fields(PIDGains)) == N.PID_GAIN_FIELDS

GainsLike = Union[None, PIDGains, Sequence[PIDGains], np.ndarray, torch.Tensor]


def gain_table(gains: GainsLike, device) -> torch.Tensor:
    """[n_sets, 22] float64 on `device`: rows are QuadPidGains structs. Accepts one PIDGains, a sequence
    of them, or an array / tensor already in that layout (the tuner builds its population that way)."""
    if gains is None:
        gains = PIDGains()
    if isinstance(gains, PIDGains):
        gains = [gains]
    if isinstance(gains, torch.Tensor):
        t = gains.to(device=device, dtype=torch.float64)
    elif isinstance(gains, np.ndarray):
        t = torch.from_numpy(np.asarray(gains, np.float64)).to(device)
    else:
        t = torch.from_numpy(np.stack([PIDGains.vector(g) for g in gains])).to(device)  # a CtrlParams' PID part
    t = t.reshape(-1, len(N.PID_GAIN_FIELDS)).contiguous()
    if t.shape[0] < 1:
        raise ValueError("at least one gain set is required")
    return t


def _set_of(set_of, n: int, device) -> Optional[torch.Tensor]:
    if set_of is None:
        return None
    t = torch.as_tensor(set_of).to(device=device, dtype=torch.int32).contiguous()
    if tuple(t.shape) != (n,):
        raise ValueError(f"set_of must have shape ({n},)")
    return t


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _act(env, entry: str, table_of, rows, set_of, law_id: int, state12, target9, state, n_state: int, out, diag,
         n_diag: int) -> torch.Tensor:
    """pid_act / ctrl_act: the shape checks, the action rows, the table (table_of(rows, device)) and the call."""
    n = int(state12.shape[0])
    env._check(state12, (n, 12), torch.float32)
    env._check(target9, (n, 9), torch.float32)
    env._check(state, (n_state, n), torch.float64)
    out = torch.empty(n, 4, dtype=torch.float32, device=env.device) if out is None else out
    env._check(out, (n, 4), torch.float32)
    if diag is not None:
        env._check(diag, (n, n_diag), torch.float64)
    tab = table_of(rows, env.device)
    so = _set_of(set_of, n, env.device)
    N.check(getattr(N.lib(), entry)(env._h, _ptr(tab), tab.shape[0], _ptr(so), law_id, _ptr(state12), _ptr(target9),
                                    n, _ptr(state), _ptr(out), _ptr(diag), env._stream()), entry)
    return out


def _episode(env, entry: str, run_type, tab: torch.Tensor, set_of, law_id: int, max_steps: int, trace_envs: int,
             state, n_state: int, course=None) -> dict:
    """pid_episode / ctrl_episode / ctrl_waypoints after the table: the metric tensors, the trace tensors of the
    first trace_envs envs (a lap's own when `course` is given), the run struct (run_type: N.QuadPidRun or
    N.QuadCtrlRun, one layout) and the call."""
    n, dev = env.num_envs, env.device
    T, M = int(max_steps), int(trace_envs)
    so = _set_of(set_of, n, dev)
    res = {k: torch.zeros(n, dtype=getattr(torch, dt), device=dev) for k, dt in N.PID_METRIC_FIELDS}
    if M > 0 and T > 0:
        res["actions"] = torch.zeros(T, M, 4, dtype=torch.float32, device=dev)
        res["state12"] = torch.zeros(T, M, 12, dtype=torch.float32, device=dev)
        if course is not None:
            res["rewards"] = torch.zeros(T, M, dtype=torch.float32, device=dev)
            res["flown_wp"] = torch.zeros(T, M, dtype=torch.int32, device=dev)
    if state is not None:
        env._check(state, (n_state, n), torch.float64)

    def ptr(t):
        return None if t is None else t.data_ptr()
    run = run_type(ptr(tab), ptr(so), tab.shape[0], law_id, T, M, ptr(state), ptr(res.get("actions")),
                   ptr(res.get("state12")), N.QuadPidMetrics(**{k: res[k].data_ptr() for k, _ in N.PID_METRIC_FIELDS}))
    args = (C.byref(run),)
    if course is not None:
        wr = course.run(res.get("rewards"), res.get("flown_wp"))
        args += (C.byref(wr),)
    N.check(getattr(N.lib(), entry)(env._h, *args, env._stream()), entry)
    return res


def pid_act(env, state12: torch.Tensor, target9: torch.Tensor, integ: torch.Tensor, gains: GainsLike = None,
            set_of=None, mode="yaw_frame", out: Optional[torch.Tensor] = None, diag: Optional[torch.Tensor] = None):
    """One CascadedPIDController.compute per row. state12 [n,12], target9 [n,9] float32; integ float64
    [6,n] (field-major; read and updated in place; zero it at an episode start); gains: see gain_table;
    set_of [n] int32 or None (set 0). Returns the actions [n,4] (and fills diag [n,6] float64 when given)."""
    return _act(env, "quad_pid_act", gain_table, gains, set_of, MODES[mode], state12, target9, integ, 6, out, diag, 6)


def target_info(env, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """info["target"], ["target_vel"], ["target_acc"] ([N,9]) for the envs' current step count."""
    out = torch.empty(env.num_envs, 9, dtype=torch.float32, device=env.device) if out is None else out
    env._check(out, (env.num_envs, 9), torch.float32)
    N.check(N.lib().quad_target_info(env._h, _ptr(out), env._stream()), "quad_target_info")
    return out


def pid_episode(env, gains: GainsLike = None, set_of=None, mode="yaw_frame", max_steps: Optional[int] = None,
                trace_envs: int = 0, integ: Optional[torch.Tensor] = None) -> dict:
    """The fused closed loop from the envs' current state (call env.reset() first). Every env runs until
    its first terminated / truncated step or `max_steps` (default: the env's max_episode_steps) and is
    then frozen, not reset. Returns the QuadPidMetrics arrays as tensors ([N]; status codes in STATUS);
    with trace_envs = M > 0 also "actions" [max_steps, M, 4] and "state12" [max_steps, M, 12] of the
    first M envs (rows past an env's last step stay zero)."""
    T = env.max_episode_steps if max_steps is None else max_steps
    return _episode(env, "quad_pid_episode", N.QuadPidRun, gain_table(gains, env.device), set_of, MODES[mode], T,
                    trace_envs, integ, 6)


def pid_score(metrics: dict) -> dict:
    """compute_performance_score (auto_tune_pid.py:127-157) for every episode of `metrics` (the tensors
    pid_episode returns): the analyses it reads -- oscillation energy, max |yaw rate|, sign-change
    frequency (analyze_yaw_oscillation), mean position error (analyze_position_tracking) -- from the
    per-episode sums. Episodes with no step (status invalid) score 0."""
    steps = metrics["steps"].to(torch.float64)
    ok = steps > 0
    n = torch.where(ok, steps, torch.ones_like(steps))
    dt = 0.01  # drone_config.DT: the reference's oscillation_freq uses it whatever the env's timestep
    osc_energy = metrics["yaw_rate_delta_sum"].to(torch.float64)
    rate_max = metrics["yaw_rate_abs_max"].to(torch.float64)
    osc_freq = metrics["yaw_rate_sign_changes"].to(torch.float64) / (n * dt)
    pos_err_mean = metrics["pos_err_sum"].to(torch.float64) / n
    yaw_score = 0.5 * (1.0 - torch.clamp(osc_energy / 1.0, max=1.0)) \
        + 0.3 * (1.0 - torch.clamp(rate_max / 3.0, max=1.0)) \
        + 0.2 * torch.clamp(1.0 - osc_freq / 5.0, min=0.0)
    pos_score = 1.0 / (1.0 + pos_err_mean)
    total = 0.6 * yaw_score + 0.4 * pos_score
    zero = torch.zeros_like(total)
    return {"yaw_score": torch.where(ok, yaw_score, zero), "pos_score": torch.where(ok, pos_score, zero),
            "total_score": torch.where(ok, total, zero), "oscillation_energy": osc_energy,
            "pos_error_mean": pos_err_mean, "rate_max": rate_max}


def gains_from_vector(v) -> PIDGains:
    v = np.asarray(v, np.float64).reshape(-1)
    return PIDGains(**{f: float(x) for f, x in zip(N.PID_GAIN_FIELDS, v)})


# ---------------------------------------------------------------------------------------------------
# the controller family
LAWS = {"pid": N.CTRL_PID_YAW, "pid_yaw": N.CTRL_PID_YAW, "yaw_frame": N.CTRL_PID_YAW,
        "pid_world": N.CTRL_PID_WORLD, "world_frame": N.CTRL_PID_WORLD,
        "se3": N.CTRL_SE3, "smc": N.CTRL_SMC, "lqr": N.CTRL_LQR}
LAWS.update({v: v for v in list(LAWS.values())})

# extra field -> (json section, key); every one optional in a file
_JSON_EXTRA = (("lqr_k0", "lqr", "k0"), ("lqr_k1", "lqr", "k1"), ("lqr_k2", "lqr", "k2"),
               ("yaw_stw_k1", "smc_yaw", "stw_k1"), ("yaw_stw_k2", "smc_yaw", "stw_k2"),
               ("yaw_stw_boundary", "smc_yaw", "stw_boundary"), ("yaw_deadband", "smc_yaw", "deadband"),
               ("yaw_v_int_max", "smc_yaw", "v_int_max"), ("yaw_rate_max", "smc_yaw", "rate_max"),
               ("yaw_rate_lpf_alpha", "smc_yaw", "rate_lpf_alpha"),
               ("se3_reorthonormalize", "se3", "reorthonormalize"))


@dataclass
class CtrlParams(PIDGains):
    """QuadCtrlParams. Defaults: PIDGains', control.lqr's gain row of lqr_controller_world_frame.py:129 in
    closed form, smc_controller_world_frame.py:124-130, and the reference's QR step switched on."""
    lqr_k0: float = 1.0 + 2.0 ** 0.5
    lqr_k1: float = 1.0 + 2.0 ** 0.5
    lqr_k2: float = 1.0
    yaw_stw_k1: float = 1.2
    yaw_stw_k2: float = 2.0
    yaw_stw_boundary: float = 0.05
    yaw_deadband: float = float(np.deg2rad(1.0))
    yaw_v_int_max: float = 2.0
    yaw_rate_max: float = 3.0
    yaw_rate_lpf_alpha: float = 0.2
    se3_reorthonormalize: float = 1.0

    @classmethod
    def from_dict(cls, d: dict) -> "CtrlParams":
        """A pid_gains.json-shaped dict; the sections "lqr", "smc_yaw" and "se3" are optional."""
        g = cls()
        for f, sec, key in _JSON + _JSON_EXTRA:
            if sec in d and key in d[sec]:
                setattr(g, f, float(d[sec][key]))
        return g

    def to_dict(self, notes: Optional[dict] = None) -> dict:
        d = super().to_dict(notes)
        for f, sec, key in _JSON_EXTRA:
            d.setdefault(sec, {})[key] = float(getattr(self, f))
        return d

    def vector(self) -> np.ndarray:
        return np.array([getattr(self, f) for f in N.CTRL_PARAM_FIELDS], np.float64)


assert tuple(f.name for f in fields(CtrlParams)) == N.CTRL_PARAM_FIELDS
assert C.sizeof(N.QuadCtrlParams) == 8 * len(N.CTRL_PARAM_FIELDS)

ParamsLike = Union[None, PIDGains, Sequence[PIDGains], np.ndarray, torch.Tensor]


def params_from_vector(v) -> CtrlParams:
    v = np.asarray(v, np.float64).reshape(-1)
    return CtrlParams(**{f: float(x) for f, x in zip(N.CTRL_PARAM_FIELDS, v)})


def _as_ctrl(g: PIDGains) -> CtrlParams:
    """A plain PIDGains takes the default extras."""
    return g if isinstance(g, CtrlParams) else CtrlParams(**{f: getattr(g, f) for f in N.PID_GAIN_FIELDS})


def param_table(params: ParamsLike, device) -> torch.Tensor:
    """[n_sets, 33] float64 on `device`: rows are QuadCtrlParams structs. Accepts one CtrlParams (or PIDGains),
    a sequence of them, or an array / tensor already in that layout."""
    if params is None:
        params = CtrlParams()
    if isinstance(params, PIDGains):
        params = [params]
    if isinstance(params, torch.Tensor):
        t = params.to(device=device, dtype=torch.float64)
    elif isinstance(params, np.ndarray):
        t = torch.from_numpy(np.asarray(params, np.float64)).to(device)
    else:
        t = torch.from_numpy(np.stack([_as_ctrl(g).vector() for g in params])).to(device)
    t = t.reshape(-1, len(N.CTRL_PARAM_FIELDS)).contiguous()
    if t.shape[0] < 1:
        raise ValueError("at least one parameter set is required")
    return t


def ctrl_act(env, state12: torch.Tensor, target9: torch.Tensor, state: torch.Tensor, params: ParamsLike = None,
             set_of=None, law="se3", out: Optional[torch.Tensor] = None, diag: Optional[torch.Tensor] = None):
    """One compute() of the law's reference class per row. As pid_act, with `state` float64 [8,n] (the six
    integrators, v_yaw, des_wz_prev; zero it at an episode start) and diag [n,7] (des_rate 3, des_att 3, |e_R|)."""
    return _act(env, "quad_ctrl_act", param_table, params, set_of, LAWS[law], state12, target9, state, N.CTRL_NSTATE,
                out, diag, N.CTRL_NDIAG)


def ctrl_episode(env, params: ParamsLike = None, set_of=None, law="se3", max_steps: Optional[int] = None,
                 trace_envs: int = 0, state: Optional[torch.Tensor] = None) -> dict:
    """pid_episode for any law of LAWS: the same metrics, traces and freezing rules, one launch."""
    T = env.max_episode_steps if max_steps is None else max_steps
    return _episode(env, "quad_ctrl_episode", N.QuadCtrlRun, param_table(params, env.device), set_of, LAWS[law], T,
                    trace_envs, state, N.CTRL_NSTATE)


def ctrl_waypoints(env, course, params: ParamsLike = None, set_of=None, law="pid_world", max_steps: int = 5000,
                   trace_envs: int = 0, state: Optional[torch.Tensor] = None) -> dict:
    """quad_ctrl_waypoints: every env of a hover `env` whose tracker status is 0 flies (law -> env step ->
    tracker) until it completes its lap, terminates, truncates or `max_steps` pass, in one launch. `course`: a
    WaypointCourse after course.begin(env) (or an earlier run: the tracker carries on). Returns ctrl_episode's
    metric tensors (status PID_LAP where the lap was completed); with trace_envs = M > 0 also "actions",
    "state12", "rewards" [T, M] and "flown_wp" [T, M] (the waypoint each step flew toward). The tracker arrays
    are course.tracker."""
    return _episode(env, "quad_ctrl_waypoints", N.QuadCtrlRun, param_table(params, env.device), set_of, LAWS[law],
                    max_steps, trace_envs, state, N.CTRL_NSTATE, course)


__all__ = ["PIDGains", "gain_table", "pid_act", "pid_episode", "pid_score", "target_info", "gains_from_vector",
           "MODES", "STATUS", "CtrlParams", "LAWS", "param_table", "params_from_vector", "ctrl_act", "ctrl_episode",
           "ctrl_waypoints"]
