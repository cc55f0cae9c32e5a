"""Batched GPU evaluation of a deterministic policy.

The reference evaluates one env at a time in Python loops (evaluate.py): ``evaluate`` runs
``num_episodes`` episodes from random resets (:296-437) and ``evaluate_trajectory`` follows a
waypoint lap (:440-612). Here N evaluations run at once on the GPU:

  * ``evaluate_episodes``  -- N episodes in parallel (HoverEnv resets, no auto-reset), each to
    termination or truncation; per-episode return and length (the reference's summary).
  * ``evaluate_waypoints`` -- N waypoint laps in parallel (one waypoint set per env, e.g. the
    eight / circle / square generators at several spacings); the bookkeeping -- reward sum, step
    count, waypoint switching within ``reach_radius``, lap completion, target update -- runs inside
    the fused ``quad_policy_waypoints`` launch (12-D observations, hover env), else it is the
    ``quad_waypoints_update`` kernel after each step of the loop. ``evaluate_ctrl_waypoints`` flies the
    same courses with a classical law (``quad_ctrl_waypoints``), ``compare_pair(..., trajectories=...)``
    any two fliers on identical courses (``--trajectory ... --controller lqr``, ``--trajectory ...
    --compare pid model``, ``--trajectory ... --deployed``).

  * ``evaluate_pid_episodes`` -- the same N episodes flown by the cascaded PID baseline
    (``controllers.py``; one fused launch), and ``compare_controllers`` -- a policy and the PID on the
    same Philox episodes, side by side (the reference's controller comparison, batched).
  * ``evaluate_ctrl_episodes`` / ``compare_pair`` -- the same for the SE(3), sliding-mode and LQR
    controllers: any two of pid / se3 / smc / lqr / model on the same episodes (``--compare A B``).

Actions are ``model.predict(obs, deterministic=True)``: the Gaussian mean clipped to the action
box (SB3 clips Box actions in predict), computed by the MFMA policy kernels for 12-D obs (the 12-128-128
ReLU net on its own kernels, any other 12-H1-H2-4 ReLU / tanh net of the reference's family on the general
actor, ppo.fused.fused_actor_for) and by the torch policy otherwise (RelPosActWrapper's 7-D obs, three hidden
layers, other widths). The model is an SB3 archive (the reference's
``hover_policy_final.zip`` or one written by ``export.save_sb3_zip``), a ``policy.pt`` state dict or
an ``ActorCritic``; with an archive the wrapper is read from the sibling ``config.json`` like
evaluate.py:314-321.

    python -m uav_reinforcement_learning_control_amd.evaluate --model models_trained/<run>/hover_policy_final.zip \\
        --trajectory eight circle square --spacing 0.25 0.5 --max-steps 5000
"""
from __future__ import annotations

import argparse
import copy
import ctypes as C
import json
import os
from typing import Optional, Sequence, Union

import numpy as np
import torch

from . import _native as N
from .envs import QuadVecEnv
from .ppo.policy import ActorCritic
from .utils.trajectories import make_trajectory


def load_policy(model: Union[str, ActorCritic], device) -> tuple:
    """(ActorCritic on device, wrapper name or None from config.json)."""
    wrapper = None
    if isinstance(model, ActorCritic):  # a copy: the caller's module stays where it is
        return copy.deepcopy(model).to(device), wrapper
    path = str(model)
    cfg_path = os.path.join(os.path.dirname(os.path.abspath(path)), "config.json")
    if os.path.exists(cfg_path):
        w = json.load(open(cfg_path)).get("wrapper", "none")
        wrapper = None if w in (None, "none") else w
    if path.endswith(".zip"):
        from .export import load_sb3_policy
        return load_sb3_policy(path, device, activations=("relu", "tanh")), wrapper
    sd = torch.load(path, map_location="cpu", weights_only=True)
    obs_dim = sd["mlp_extractor.policy_net.0.weight"].shape[1]
    hidden = (sd["mlp_extractor.policy_net.0.weight"].shape[0], sd["mlp_extractor.policy_net.2.weight"].shape[0])
    pol = ActorCritic(obs_dim, sd["action_net.weight"].shape[0], hidden)  # a state dict names no activation: ReLU
    pol.load_state_dict(sd)
    return pol.to(device), wrapper


class _Actor:
    """Deterministic actions into a fixed [N,4] buffer."""

    def __init__(self, policy: ActorCritic, n: int, device):
        self.policy = policy
        self.out = torch.zeros(n, 4, device=device)
        self.fp = None
        from .ppo.fused import _net_supported, fused_actor_for
        if _net_supported(policy):  # the 128-128 ReLU net's own kernel, the general actor for the rest of the family
            self.fp = fused_actor_for(policy)
            self.fp.pack()

    @torch.no_grad()
    def __call__(self, obs: torch.Tensor) -> torch.Tensor:
        if self.fp is not None:
            self.fp.act(obs, self.out, deterministic=True)
        else:
            mean, _ = self.policy.forward_heads(obs)
            torch.clamp(mean, -1.0, 1.0, out=self.out)
        return self.out


def _waypoint_sets(trajectories, spacings) -> list:
    sets = []
    for t in trajectories:
        if isinstance(t, str):
            for sp in spacings:
                sets.append((f"{t}@{sp}", make_trajectory(t, spacing=sp)))
        else:
            sets.append((f"custom{len(sets)}", np.asarray(t, np.float64)))
    return sets


def _lap_extras(out: dict, sets, n: int, m: Optional[dict]) -> dict:
    out["name"] = np.array([sets[i % len(sets)][0] for i in range(n)])
    out["n_waypoints"] = np.array([len(sets[i % len(sets)][1]) for i in range(n)])
    if m is not None:
        out["metrics"] = m
        out["pos_errors"] = m["pos_err_sum"] / np.maximum(m["steps"], 1)
    return out


def _lap_record(out: dict, m: dict) -> None:
    """record=True from the fused traces: rows up to the longest flight; rows past an env's last step are zero."""
    T = max(int(out["steps"].max()), 1)
    out["positions"] = m.pop("state12")[:T, :, :3].copy()
    out["actions"] = m.pop("actions")[:T]
    out["rewards"] = m.pop("rewards")[:T]
    out["flown_wp"] = m.pop("flown_wp")[:T]


@torch.no_grad()
def evaluate_waypoints(model, trajectories: Sequence = ("eight",), spacings: Sequence[float] = (0.5,),
                       reach_radius: float = 0.25, max_steps: int = 5000, replicas: int = 1,
                       wrapper: Optional[str] = "auto", env: str = "hover", device="cuda",
                       seed: int = 0, record: bool = False, fused: Optional[bool] = None, obs_mode: str = "env",
                       velocity_alpha: Optional[float] = None) -> dict:
    """One lap per (waypoint set x replica) env, all at once. Returns per-env numpy arrays
    (name, steps, reached, laps, status, total_reward; with record=True also positions /
    actions / rewards [T, N, ...]) -- status 1 = lap completed, 2 = terminated, 3 = max steps.
    `fused`: None flies the laps in one quad_policy_waypoints / quad_actor_waypoints launch where that is supported
    (a 12-H1-H2-4 policy of ppo.fused.FusedActor's family on a hover env with 12-D observations), else in the per-step loop; both give the same bits for
    every env up to its last step (the loop goes on stepping a finished env, the launch freezes it and leaves
    its later record rows zero). The launch adds "metrics" (the QuadPidMetrics arrays and vel_err_sq) and
    "pos_errors"; obs_mode="deployed" (fused only) feeds the policy the ROS2 node's observation, velocity
    estimated with `velocity_alpha` (default 0.8)."""
    from .ppo.fused import fused_actor_for, waypoints_supported
    from .waypoints import WaypointCourse
    device = torch.device(device)
    policy, cfg_wrapper = load_policy(model, device)
    wrapper = cfg_wrapper if wrapper == "auto" else wrapper
    sets = _waypoint_sets(trajectories, spacings)
    n = len(sets) * replicas
    course = WaypointCourse([p for _, p in sets], n, reach_radius, device)
    e = QuadVecEnv(n, env=env, wrapper=wrapper, device=device, seed=seed,
                   max_episode_steps=max_steps, auto_reset=False)
    e.reset()
    obs = course.begin(e)
    if obs_mode not in ("env", "deployed"):
        raise ValueError(f"obs_mode must be \"env\" or \"deployed\", got {obs_mode!r}")
    ok = waypoints_supported(policy, e)
    use = ok if fused is None else bool(fused)
    if use and not ok:
        raise ValueError("fused=True: the one-launch laps fly 12-H1-H2-4 policies (ppo.fused.FusedActor's family) on "
                         "hover envs with 12-D observations")
    if obs_mode == "deployed" and not use:
        raise ValueError("obs_mode=\"deployed\" runs in the fused launch only")
    if use:
        fp = fused_actor_for(policy)
        fp.pack()
        m = fp.waypoints(e, course, max_steps=max_steps, obs_mode=obs_mode, trace_envs=n if record else 0,
                         alpha_all=0.8 if velocity_alpha is None else float(velocity_alpha))
        torch.cuda.synchronize(device)
        m = {k: v.cpu().numpy() for k, v in m.items()}
        out = course.result()
        if record:
            _lap_record(out, m)
            m.pop("obs"), m.pop("vel_est")
        e.close()
        return _lap_extras(out, sets, n, m)
    act = _Actor(policy, n, device)
    rec = {"positions": [], "actions": [], "rewards": []} if record else None
    for t in range(max_steps):
        a = act(obs)
        _, rew, te, tr, info = e.step(a, obs=obs, info="full")
        if rec is not None:
            rec["positions"].append(info["state"][:, :3].clone())
            rec["actions"].append(a.clone())
            rec["rewards"].append(rew.clone())
        course.update(e, info["state"], rew, te, tr)
        if (t + 1) % 128 == 0 and bool((course.tracker["status"] != 0).all()):
            break
    torch.cuda.synchronize(device)
    out = _lap_extras(course.result(), sets, n, None)
    if rec is not None:
        out["positions"] = torch.stack(rec["positions"]).cpu().numpy()
        out["actions"] = torch.stack(rec["actions"]).cpu().numpy()
        out["rewards"] = torch.stack(rec["rewards"]).cpu().numpy()
    e.close()
    return out


def _lap_law(law: str) -> str:
    """A lap is trajectory following: "pid" is the world-frame PID, the reference's trajectory follower."""
    return "pid_world" if law == "pid" else law


@torch.no_grad()
def evaluate_ctrl_waypoints(law: str, params=None, trajectories: Sequence = ("eight",),
                            spacings: Sequence[float] = (0.5,), reach_radius: float = 0.25, max_steps: int = 5000,
                            replicas: int = 1, device="cuda", seed: int = 0, record: bool = False) -> dict:
    """evaluate_waypoints flown by a law of the controller family ("pid": the world-frame PID; "pid_yaw",
    "se3", "smc", "lqr") in one quad_ctrl_waypoints launch, on the same courses (same sets, same env order).
    `params`: a CtrlParams / PIDGains, a pid_gains.json-shaped path, or None. Returns evaluate_waypoints'
    keys (name, n_waypoints, wp_idx, reached, laps, steps, status, total_reward), "metrics" (the
    QuadPidMetrics arrays) and "pos_errors" (per-env mean position error against the target each step was
    flown with); with record=True also positions / actions / rewards / flown_wp [T, N, ...]."""
    from .controllers import CtrlParams, ctrl_waypoints
    from .waypoints import WaypointCourse
    device = torch.device(device)
    if isinstance(params, str):
        params = CtrlParams.from_json(params)
    sets = _waypoint_sets(trajectories, spacings)
    n = len(sets) * replicas
    course = WaypointCourse([p for _, p in sets], n, reach_radius, device)
    e = QuadVecEnv(n, env="hover", wrapper=None, device=device, seed=seed, max_episode_steps=max_steps,
                   auto_reset=False)
    e.reset()
    course.begin(e)
    m = ctrl_waypoints(e, course, params, law=_lap_law(law), max_steps=max_steps, trace_envs=n if record else 0)
    torch.cuda.synchronize(device)
    m = {k: v.cpu().numpy() for k, v in m.items()}
    out = course.result()
    if record:
        _lap_record(out, m)
    e.close()
    return _lap_extras(out, sets, n, m)


def lap_table(rows_in) -> str:
    """One line per flier: status counts, mean steps, waypoints reached and mean position error."""
    rows = [f"{'controller':>14} {'laps':>6} {'term.':>6} {'max steps':>9} {'running':>8} {'steps':>9} "
            f"{'reached':>8} {'pos error':>10}"]
    for name, r in rows_in:
        st = np.asarray(r["status"])
        pe = f"{float(np.mean(r['pos_errors'])):9.3f}m" if "pos_errors" in r else f"{'-':>10}"
        rows.append(f"{name:>14} {int((st == 1).sum()):6d} {int((st == 2).sum()):6d} {int((st == 3).sum()):9d} "
                    f"{int((st == 0).sum()):8d} {float(np.mean(r['steps'])):9.1f} {float(np.mean(r['reached'])):8.2f} "
                    f"{pe}")
    return "\n".join(rows)


def _use_fused(fused: Optional[bool], policy, e, obs_mode: str) -> bool:
    """None: the fused launch where quad_policy_episode flies this policy on this env, else the per-step loop."""
    from .ppo.fused import episode_supported
    if obs_mode not in ("env", "deployed"):
        raise ValueError(f"obs_mode must be \"env\" or \"deployed\", got {obs_mode!r}")
    ok = episode_supported(policy, e)
    use = ok if fused is None else bool(fused)
    if use and not ok:
        raise ValueError("fused=True: the one-launch episodes fly 12-H1-H2-4 policies (ppo.fused.FusedActor's family) "
                         "on hover / trajectory envs with 12-D observations")
    if obs_mode == "deployed" and not use:
        raise ValueError("obs_mode=\"deployed\" runs in the fused launch only")
    return use


def _first_obs(e, obs: torch.Tensor) -> torch.Tensor:
    """The per-step loop's first observation: quad_observe's, which is what the one-launch episodes start from
    (their contract, include/quadenv.h). quad_reset's returned observation is built from the drawn Euler angles,
    quad_observe's from the stored quaternion: the attitude features differ by up to 2 ulp in about a third of
    the envs, enough to move a return by one ulp of a step's reward now and then, so a loop started from
    reset()'s row is not bit-identical to the launch."""
    e.observe(out=obs)
    return obs


def _fused_episodes(policy, e, obs_mode: str, velocity_alpha: Optional[float]) -> dict:
    """One quad_policy_episode / quad_actor_episode launch over e's envs; the metric arrays on the host."""
    from .ppo.fused import fused_actor_for
    fp = fused_actor_for(policy)
    fp.pack()
    m = fp.episode(e, obs_mode=obs_mode, alpha_all=0.8 if velocity_alpha is None else float(velocity_alpha))
    torch.cuda.synchronize(e.device)
    return {k: v.cpu().numpy() for k, v in m.items()}


def vel_rmse(vel_err_sq, steps) -> float:
    """evaluate.py:751-760's RMSE of the velocity estimate: sqrt(sum of |v_est - v_true|^2 / samples)."""
    return float(np.sqrt(np.sum(np.asarray(vel_err_sq, np.float64)) / max(int(np.sum(steps)), 1)))


@torch.no_grad()
def evaluate_episodes(model, num_episodes: int = 1024, wrapper: Optional[str] = "auto", env: str = "hover",
                      max_episode_steps: Optional[int] = None, device="cuda", seed: int = 0,
                      fused: Optional[bool] = None, obs_mode: str = "env",
                      velocity_alpha: Optional[float] = None) -> dict:
    """``num_episodes`` episodes at once from HoverEnv resets, deterministic policy, each run to
    termination or truncation (evaluate.py:296-437 without the viewer). Returns per-episode
    rewards / lengths / terminated flags and their mean / std. `fused`: None flies them in one
    quad_policy_episode / quad_actor_episode launch where that is supported, else in the per-step loop (the same
    bits: the loop starts from quad_observe's observation, as the launch does, see _first_obs);
    obs_mode="deployed" feeds the policy the ROS2 node's observation (velocity estimated with
    `velocity_alpha`, default 0.8; clipped) and adds vel_rmse and pos_errors."""
    device = torch.device(device)
    policy, cfg_wrapper = load_policy(model, device)
    wrapper = cfg_wrapper if wrapper == "auto" else wrapper
    e = QuadVecEnv(num_episodes, env=env, wrapper=wrapper, device=device, seed=seed,
                   max_episode_steps=max_episode_steps, auto_reset=False)
    obs = e.reset().clone()
    if _use_fused(fused, policy, e, obs_mode):
        m = _fused_episodes(policy, e, obs_mode, velocity_alpha)
        e.close()
        r, l = m["total_reward"], m["steps"]
        out = {"rewards": r, "lengths": l, "terminated": m["status"] == N.PID_TERMINATED,
               "mean_reward": float(r.mean()), "std_reward": float(r.std()),
               "mean_length": float(l.mean()), "std_length": float(l.std())}
        if obs_mode == "deployed":
            out["vel_rmse"] = vel_rmse(m["vel_err_sq"], l)
            out["pos_errors"] = m["pos_err_sum"] / np.maximum(l, 1)
        return out
    act = _Actor(policy, num_episodes, device)
    obs = _first_obs(e, obs)
    ret = torch.zeros(num_episodes, dtype=torch.float64, device=device)
    length = torch.zeros(num_episodes, dtype=torch.int32, device=device)
    running = torch.ones(num_episodes, dtype=torch.bool, device=device)
    terminated = torch.zeros(num_episodes, dtype=torch.bool, device=device)
    for t in range(e.max_episode_steps):
        a = act(obs)
        _, rew, te, tr, _ = e.step(a, obs=obs, info="raw")
        ret += torch.where(running, rew.double(), 0.0)
        length += running.int()
        terminated |= running & te
        running &= ~(te | tr)
        if (t + 1) % 64 == 0 and not bool(running.any()):
            break
    r, l = ret.cpu().numpy(), length.cpu().numpy()
    e.close()
    return {"rewards": r, "lengths": l, "terminated": terminated.cpu().numpy(),
            "mean_reward": float(r.mean()), "std_reward": float(r.std()),
            "mean_length": float(l.mean()), "std_length": float(l.std())}


def _summary(rewards, lengths, terminated, **extra) -> dict:
    r, l = np.asarray(rewards, np.float64), np.asarray(lengths)
    return {"rewards": r, "lengths": l, "terminated": np.asarray(terminated, bool),
            "mean_reward": float(r.mean()), "std_reward": float(r.std()),
            "mean_length": float(l.mean()), "std_length": float(l.std()), **extra}


def _pid_mode(env: str, mode: Optional[str]) -> str:
    """The reference flies HoverEnv with pid_controller.py and TrajectoryFollowEnv with the world-frame law."""
    return mode or ("world_frame" if env in ("trajectory", "TrajectoryFollowEnv") else "yaw_frame")


@torch.no_grad()
def evaluate_pid_episodes(gains=None, num_episodes: int = 1024, env: str = "hover", mode: Optional[str] = None,
                          max_episode_steps: Optional[int] = None, device="cuda", seed: int = 0,
                          env_id_base: int = 0) -> dict:
    """``evaluate_episodes`` with the cascaded PID baseline as the controller: the same resets (same seed
    and env ids), each episode to termination or truncation, in one fused launch. `gains`: a PIDGains, a
    pid_gains.json path, or None (the reference's committed gains). Returns evaluate_episodes' keys plus
    pos_errors (per-episode mean position error), mean_pos_error, survival (fraction that reached the
    time limit), reset_obs and the raw metrics."""
    from .controllers import PIDGains, pid_episode
    device = torch.device(device)
    if isinstance(gains, str):
        gains = PIDGains.from_json(gains)
    e = QuadVecEnv(num_episodes, env=env, wrapper=None, device=device, seed=seed, env_id_base=env_id_base,
                   max_episode_steps=max_episode_steps, auto_reset=False)
    reset_obs = e.reset().clone()
    m = pid_episode(e, gains, mode=_pid_mode(env, mode))
    torch.cuda.synchronize(device)
    m = {k: v.cpu().numpy() for k, v in m.items()}
    e.close()
    pe = m["pos_err_sum"] / np.maximum(m["steps"], 1)
    return _summary(m["total_reward"], m["steps"], m["status"] == N.PID_TERMINATED, pos_errors=pe,
                    mean_pos_error=float(pe.mean()), survival=float((m["status"] == N.PID_TRUNCATED).mean()),
                    reset_obs=reset_obs.cpu().numpy(), metrics=m)


@torch.no_grad()
def compare_controllers(model, gains=None, num_episodes: int = 256, wrapper: Optional[str] = "auto",
                        env: str = "hover", mode: Optional[str] = None, max_episode_steps: Optional[int] = None,
                        device="cuda", seed: int = 0) -> dict:
    """A policy and the PID baseline on the same Philox episodes (same seed and env ids, so identical
    start states and targets): {"policy": ..., "pid": ...}, each with evaluate_episodes' keys plus
    pos_errors / mean_pos_error, survival and reset_obs; "table" is the side-by-side text."""
    device = torch.device(device)
    pol, max_steps = _policy_episodes(model, num_episodes, wrapper, env, max_episode_steps, device, seed)
    pid = evaluate_pid_episodes(gains, num_episodes, env=env, mode=mode, max_episode_steps=max_steps,
                                device=device, seed=seed)
    return {"policy": pol, "pid": pid, "table": _table((("policy", pol), ("pid", pid)))}


def _table(rows_in) -> str:
    rows = [f"{'controller':>10} {'reward':>18} {'length':>16} {'survival':>9} {'pos error':>10}"]
    for name, r in rows_in:
        rows.append(f"{name:>10} {r['mean_reward']:9.2f} +/- {r['std_reward']:5.2f} {r['mean_length']:8.1f} +/- "
                    f"{r['std_length']:5.1f} {100 * r['survival']:8.1f}% {r['mean_pos_error']:9.3f}m")
    return "\n".join(rows)


def _policy_episodes(model, num_episodes, wrapper, env, max_episode_steps, device, seed,
                     fused: Optional[bool] = None, obs_mode: str = "env",
                     velocity_alpha: Optional[float] = None) -> tuple:
    """The policy's episodes with the PID metric's position error: (summary, the env's time limit). `fused`,
    `obs_mode` and `velocity_alpha` as in evaluate_episodes."""
    policy, cfg_wrapper = load_policy(model, device)
    wrapper = cfg_wrapper if wrapper == "auto" else wrapper
    e = QuadVecEnv(num_episodes, env=env, wrapper=wrapper, device=device, seed=seed,
                   max_episode_steps=max_episode_steps, auto_reset=False)
    obs = e.reset().clone()
    reset_obs = obs.clone()
    digests = episode_digests(e)
    if _use_fused(fused, policy, e, obs_mode):
        m = _fused_episodes(policy, e, obs_mode, velocity_alpha)
        l, te_np = m["steps"], m["status"] == N.PID_TERMINATED
        pe = m["pos_err_sum"] / np.maximum(l, 1)
        extra = {"vel_rmse": vel_rmse(m["vel_err_sq"], l)} if obs_mode == "deployed" else {}
        pol = _summary(m["total_reward"], l, te_np, pos_errors=pe, mean_pos_error=float(pe.mean()),
                       survival=float((~te_np).mean()), reset_obs=reset_obs.cpu().numpy(), digests=digests, **extra)
        max_steps = e.max_episode_steps
        e.close()
        return pol, max_steps
    act = _Actor(policy, num_episodes, device)
    obs = _first_obs(e, obs)
    n = num_episodes
    ret = torch.zeros(n, dtype=torch.float64, device=device)
    perr = torch.zeros(n, dtype=torch.float64, device=device)
    length = torch.zeros(n, dtype=torch.int32, device=device)
    running = torch.ones(n, dtype=torch.bool, device=device)
    terminated = torch.zeros(n, dtype=torch.bool, device=device)
    target = e.current_target_info()[:, 0:3].clone()  # the target in hand before the step, as the PID metric reads it
    for t in range(e.max_episode_steps):
        a = act(obs)
        _, rew, te, tr, info = e.step(a, obs=obs, info="full")
        d = (info["state"][:, 0:3] - target).double().norm(dim=1)
        target.copy_(info["target"])
        ret += torch.where(running, rew.double(), 0.0)
        perr += torch.where(running, d, 0.0)
        length += running.int()
        terminated |= running & te
        running &= ~(te | tr)
        if (t + 1) % 64 == 0 and not bool(running.any()):
            break
    l = length.cpu().numpy()
    pe = perr.cpu().numpy() / np.maximum(l, 1)
    te_np = terminated.cpu().numpy()
    pol = _summary(ret.cpu().numpy(), l, te_np, pos_errors=pe, mean_pos_error=float(pe.mean()),
                   survival=float((~te_np).mean()), reset_obs=reset_obs.cpu().numpy(), digests=digests)
    max_steps = e.max_episode_steps
    e.close()
    return pol, max_steps


CONTROLLERS = ("pid", "se3", "smc", "lqr")


@torch.no_grad()
def evaluate_ctrl_episodes(law: str, params=None, num_episodes: int = 1024, env: str = "hover",
                           max_episode_steps: Optional[int] = None, device="cuda", seed: int = 0,
                           env_id_base: int = 0) -> dict:
    """evaluate_pid_episodes for any law of the controller family ("pid": the PID the reference flies on
    `env`; "se3", "smc", "lqr"), one fused launch. `params`: a CtrlParams / PIDGains, a pid_gains.json-shaped
    path, or None (the reference's values, SE(3)'s QR step included: see DESIGN 15 before flying it on hover)."""
    from .controllers import CtrlParams, ctrl_episode
    device = torch.device(device)
    if isinstance(params, str):
        params = CtrlParams.from_json(params)
    law = _pid_mode(env, None) if law == "pid" else law
    e = QuadVecEnv(num_episodes, env=env, wrapper=None, device=device, seed=seed, env_id_base=env_id_base,
                   max_episode_steps=max_episode_steps, auto_reset=False)
    reset_obs = e.reset().clone()
    digests = episode_digests(e)
    m = ctrl_episode(e, params, law=law)
    torch.cuda.synchronize(device)
    m = {k: v.cpu().numpy() for k, v in m.items()}
    e.close()
    pe = m["pos_err_sum"] / np.maximum(m["steps"], 1)
    return _summary(m["total_reward"], m["steps"], m["status"] == N.PID_TERMINATED, pos_errors=pe,
                    mean_pos_error=float(pe.mean()), survival=float((m["status"] == N.PID_TRUNCATED).mean()),
                    reset_obs=reset_obs.cpu().numpy(), metrics=m, digests=digests)


def episode_digests(e: QuadVecEnv) -> list:
    """One digest per env of its state right after reset() (qpos, qvel, target: whatever wrapper shapes the
    observation): two runs with equal digests flew the same resets."""
    import hashlib
    st = e.get_state()
    rows = np.concatenate([np.ascontiguousarray(st[k], np.float32).reshape(e.num_envs, -1)
                           for k in ("qpos", "qvel", "target")], axis=1)
    return [hashlib.sha256(row.tobytes()).hexdigest()[:16] for row in rows]


@torch.no_grad()
def compare_pair(a: str, b: str, model=None, params=None, num_episodes: int = 256, env: str = "hover",
                 wrapper: Optional[str] = "auto", max_episode_steps: Optional[int] = None, device="cuda",
                 seed: int = 0, survive_steps: int = 512, trajectories: Optional[Sequence] = None,
                 spacings: Sequence[float] = (0.5,), reach_radius: float = 0.25, max_steps: int = 5000,
                 replicas: int = 1, obs_mode: str = "env", velocity_alpha: Optional[float] = None) -> dict:
    """The reference's compare_controllers.py, batched: controllers `a` and `b` (any of CONTROLLERS, or
    "model" for the policy `model`) on the same Philox episodes. {a: ..., b: ..., "table"}; each entry has
    evaluate_pid_episodes' keys plus "digests" and "survival_rate" (episodes of at least `survive_steps`
    steps, compare_controllers.py's measure); the table prints its four metrics. With `trajectories` both
    sides fly waypoint laps on the same courses instead (evaluate_waypoints / evaluate_ctrl_waypoints with
    `spacings`, `reach_radius`, `max_steps`, `replicas`; hover env): each entry has their keys, the table is
    lap_table's."""
    device = torch.device(device)
    out = {}
    if trajectories is not None:
        for name in (a, b):
            if name == "model":
                if model is None:
                    raise ValueError("comparing against \"model\" needs a policy")
                out[name] = evaluate_waypoints(model, trajectories, spacings, reach_radius, max_steps, replicas,
                                               wrapper=wrapper, device=device, seed=seed, obs_mode=obs_mode,
                                               velocity_alpha=velocity_alpha)
            elif name in CONTROLLERS:
                out[name] = evaluate_ctrl_waypoints(name, params, trajectories, spacings, reach_radius, max_steps,
                                                    replicas, device=device, seed=seed)
            else:
                raise ValueError(f"unknown controller {name!r}: one of {CONTROLLERS + ('model',)}")
        out["table"] = lap_table([(name, out[name]) for name in dict.fromkeys((a, b))])
        return out
    for name in (a, b):
        if name == "model":
            if model is None:
                raise ValueError("comparing against \"model\" needs a policy")
            r, _ = _policy_episodes(model, num_episodes, wrapper, env, max_episode_steps, device, seed)
        elif name in CONTROLLERS:
            r = evaluate_ctrl_episodes(name, params, num_episodes, env, max_episode_steps, device, seed)
        else:
            raise ValueError(f"unknown controller {name!r}: one of {CONTROLLERS + ('model',)}")
        r["survival_rate"] = float((r["lengths"] >= survive_steps).mean())
        out[name] = r
    rows = [f"{'controller':>10} {'mean reward':>12} {'mean length':>12} {'pos error':>10} {'survival':>9}"]
    for name in dict.fromkeys((a, b)):
        r = out[name]
        rows.append(f"{name:>10} {r['mean_reward']:12.2f} {r['mean_length']:12.1f} {r['mean_pos_error']:9.3f}m "
                    f"{100 * r['survival_rate']:8.1f}%")
    out["table"] = "\n".join(rows)
    return out


@torch.no_grad()
def evaluate_velocity_estimator(model, alphas: Sequence[float] = (0.0, 0.1, 0.2), num_episodes: int = 256,
                                max_steps: int = 2000, closed_loop: bool = False, wrapper: Optional[str] = "auto",
                                env: str = "hover", device="cuda", seed: int = 0, trace_envs: int = 0) -> dict:
    """The reference's ``evaluate.py --test-velocity`` (:615-770), batched: every alpha of `alphas` flies the
    same `num_episodes` resets (alpha-major: env a * num_episodes + e starts from reset e, so a wave shares
    its alpha) for up to `max_steps` steps in one launch. closed_loop=False is the reference's test: the
    policy sees the env's observation and the estimators run beside it. closed_loop=True feeds the policy
    the deployed observation, which the reference never does. Returns {"alphas", "rmse" (per alpha:
    sqrt(sum vel_err_sq / sum steps)), "steps", "start" (the copied start states), "metrics", "table"}, with
    closed_loop=True also "mean_reward", "mean_length", "survival" and "mean_pos_error" per alpha."""
    from .ppo.fused import episode_supported, fused_actor_for
    device = torch.device(device)
    alphas = [float(a) for a in alphas]
    if not alphas or num_episodes < 1:
        raise ValueError("at least one alpha and one episode are required")
    policy, cfg_wrapper = load_policy(model, device)
    wrapper = cfg_wrapper if wrapper == "auto" else wrapper
    A, E = len(alphas), int(num_episodes)
    src = QuadVecEnv(E, env=env, wrapper=wrapper, device=device, seed=seed, max_episode_steps=max_steps,
                     auto_reset=False)
    src.reset()
    st = src.get_state()
    src.close()
    e = QuadVecEnv(A * E, env=env, wrapper=wrapper, device=device, seed=seed, max_episode_steps=max_steps,
                   auto_reset=False)
    if not episode_supported(policy, e):
        e.close()
        raise ValueError("evaluate_velocity_estimator needs a 12-H1-H2-4 policy (ppo.fused.FusedActor's family) on a "
                         "12-D observation env")
    start = {k: np.tile(v, (A,) + (1,) * (v.ndim - 1)) for k, v in st.items()}
    e.set_state(**start)
    fp = fused_actor_for(policy)
    fp.pack()
    alpha = torch.tensor(alphas, dtype=torch.float64, device=device).repeat_interleave(E)
    m = fp.episode(e, max_steps=max_steps, obs_mode="deployed" if closed_loop else "env", alpha=alpha,
                   trace_envs=trace_envs)
    torch.cuda.synchronize(device)
    m = {k: v.cpu().numpy() for k, v in m.items()}
    e.close()
    return velocity_summary(alphas, E, m, closed_loop, start)


def velocity_summary(alphas, episodes: int, m: dict, closed_loop: bool, start: Optional[dict] = None) -> dict:
    """evaluate_velocity_estimator's figures from the alpha-major metric arrays of one launch."""
    A, E = len(alphas), int(episodes)
    steps = np.asarray(m["steps"]).reshape(A, E)
    out = {"alphas": list(alphas), "steps": steps.sum(axis=1), "metrics": m, "start": start,
           "rmse": np.array([vel_rmse(np.asarray(m["vel_err_sq"]).reshape(A, E)[a], steps[a]) for a in range(A)])}
    rows = [f"{'alpha':>6} {'vel RMSE':>12} {'samples':>9}"]
    if closed_loop:
        st = np.asarray(m["status"]).reshape(A, E)
        out["mean_reward"] = np.asarray(m["total_reward"]).reshape(A, E).mean(axis=1)
        out["mean_length"] = steps.mean(axis=1)
        out["survival"] = (st != N.PID_TERMINATED).mean(axis=1)
        out["mean_pos_error"] = (np.asarray(m["pos_err_sum"]).reshape(A, E) / np.maximum(steps, 1)).mean(axis=1)
        rows[0] += f" {'reward':>10} {'length':>8} {'survival':>9} {'pos error':>10}"
    for a in range(A):
        row = f"{alphas[a]:6.2f} {out['rmse'][a]:8.4f} m/s {int(out['steps'][a]):9d}"
        if closed_loop:
            row += (f" {out['mean_reward'][a]:10.2f} {out['mean_length'][a]:8.1f} {100 * out['survival'][a]:8.1f}% "
                    f"{out['mean_pos_error'][a]:9.3f}m")
        rows.append(row)
    out["table"] = "\n".join(rows)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--model", default=None, help="policy archive / state dict (not needed with --controller pid)")
    ap.add_argument("--controller", choices=["policy", "pid", "both", "se3", "smc", "lqr"], default="policy",
                    help="pid: the cascaded PID baseline; both: policy and PID on the same episodes; "
                         "se3 / smc / lqr: the reference's other classical controllers")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"), default=None,
                    help="fly two controllers (pid, se3, smc, lqr or model) on the same episodes")
    ap.add_argument("--se3-reorthonormalize", type=int, choices=[0, 1], default=1,
                    help="0: skip the SE(3) controller's np.linalg.qr step (as written it does not hover)")
    ap.add_argument("--gains", default=None, help="pid_gains.json-shaped file (default: the reference's gains)")
    ap.add_argument("--env", default="hover", choices=["hover", "trajectory"])
    ap.add_argument("--mode", choices=["episodes", "trajectory"], default="trajectory")
    ap.add_argument("--trajectory", nargs="+", default=None, choices=["eight", "circle", "square"],
                    help="waypoint laps (default eight); given with --controller pid|se3|smc|lqr, --compare or "
                         "--deployed, those fly the laps instead of hover episodes")
    ap.add_argument("--spacing", nargs="+", type=float, default=[0.5])
    ap.add_argument("--reach-radius", type=float, default=0.25)
    ap.add_argument("--max-steps", type=int, default=5000)
    ap.add_argument("--replicas", type=int, default=1)
    ap.add_argument("--num-episodes", type=int, default=1024)
    ap.add_argument("--test-velocity", nargs="*", type=float, default=None, metavar="ALPHA",
                    help="the velocity estimator's RMSE per low-pass alpha (default 0.0 0.1 0.2)")
    ap.add_argument("--deployed", action="store_true",
                    help="feed the policy the ROS2 node's observation (estimated velocity, clipped); with "
                         "--test-velocity: close the loop through the estimator")
    ap.add_argument("--velocity-alpha", type=float, default=None,
                    help="the estimator's alpha for --deployed episodes (default 0.8)")
    a = ap.parse_args(argv)
    laps = a.trajectory is not None  # asked for by name: the classical laws, --compare and --deployed fly laps too
    a.trajectory = a.trajectory or ["eight"]
    if a.test_velocity is not None:
        if a.model is None:
            ap.error("--test-velocity needs --model")
        r = evaluate_velocity_estimator(a.model, a.test_velocity or [0.0, 0.1, 0.2], a.num_episodes,
                                        max_steps=min(a.max_steps, 2000), closed_loop=a.deployed, env=a.env)
        print(r["table"])
        return r
    if a.compare or a.controller in ("se3", "smc", "lqr"):
        from .controllers import CtrlParams
        params = CtrlParams.from_json(a.gains) if a.gains else CtrlParams()
        params.se3_reorthonormalize = float(a.se3_reorthonormalize)
        if a.compare:
            if "model" in a.compare and a.model is None:
                ap.error("--compare with model needs --model")
            if laps:
                r = compare_pair(a.compare[0], a.compare[1], a.model, params, trajectories=a.trajectory,
                                 spacings=a.spacing, reach_radius=a.reach_radius, max_steps=a.max_steps,
                                 replicas=a.replicas, obs_mode="deployed" if a.deployed else "env",
                                 velocity_alpha=a.velocity_alpha)
            else:
                r = compare_pair(a.compare[0], a.compare[1], a.model, params, a.num_episodes, env=a.env)
            print(r["table"])
            return r
        if laps:
            r = evaluate_ctrl_waypoints(a.controller, params, a.trajectory, a.spacing, a.reach_radius, a.max_steps,
                                        a.replicas)
            _print_laps(a.controller, r)
            return r
        r = evaluate_ctrl_episodes(a.controller, params, a.num_episodes, env=a.env)
        print(f"Episodes: {a.num_episodes}\nSurvival: {100 * r['survival']:.0f}%\n"
              f"Mean reward: {r['mean_reward']:.2f} +/- {r['std_reward']:.2f}\n"
              f"Mean length: {r['mean_length']:.1f} +/- {r['std_length']:.1f}\nMean error: {r['mean_pos_error']:.3f}m")
        return r
    if a.controller == "pid" and laps:
        r = evaluate_ctrl_waypoints("pid", a.gains, a.trajectory, a.spacing, a.reach_radius, a.max_steps, a.replicas)
        _print_laps("pid", r)
        return r
    if a.controller == "pid":
        r = evaluate_pid_episodes(a.gains, a.num_episodes, env=a.env)
        print(f"Episodes: {a.num_episodes}\nSurvival: {100 * r['survival']:.0f}%\n"
              f"Mean reward: {r['mean_reward']:.2f} +/- {r['std_reward']:.2f}\n"
              f"Mean length: {r['mean_length']:.1f} +/- {r['std_length']:.1f}\nMean error: {r['mean_pos_error']:.3f}m")
        return r
    if a.model is None:
        ap.error("--model is required unless --controller pid")
    if a.controller == "both":
        r = compare_controllers(a.model, a.gains, a.num_episodes, env=a.env)
        print(r["table"])
        return r
    if a.mode == "episodes" or (a.deployed and not laps):
        r = evaluate_episodes(a.model, a.num_episodes, obs_mode="deployed" if a.deployed else "env",
                              velocity_alpha=a.velocity_alpha)
        print(f"Episodes: {a.num_episodes}\nMean reward: {r['mean_reward']:.2f} +/- {r['std_reward']:.2f}\n"
              f"Mean length: {r['mean_length']:.1f} +/- {r['std_length']:.1f}")
        if a.deployed:
            print(f"Velocity RMSE: {r['vel_rmse']:.4f} m/s\nMean error: {r['pos_errors'].mean():.3f}m")
        return r
    r = evaluate_waypoints(a.model, a.trajectory, a.spacing, a.reach_radius, a.max_steps, a.replicas,
                           obs_mode="deployed" if a.deployed else "env", velocity_alpha=a.velocity_alpha)
    _print_laps("policy (deployed)" if a.deployed else "policy", r)
    return r


def _print_laps(name: str, r: dict) -> None:
    """evaluate.py's per-course line, with the mean position error where the fused launch measured it, and the
    summary line of lap_table."""
    from .waypoints import STATUS
    for i in range(len(r["name"])):
        pe = f"  pos error {r['pos_errors'][i]:.3f}m" if "pos_errors" in r else ""
        print(f"{r['name'][i]:>12}: steps {r['steps'][i]:5d}  waypoints {r['reached'][i]:3d}/"
              f"{r['n_waypoints'][i]:3d}  laps {r['laps'][i]}  reward {r['total_reward'][i]:9.2f}  "
              f"{STATUS[int(r['status'][i])]}{pe}")
    print(lap_table([(name, r)]))


if __name__ == "__main__":
    main()
