#!/usr/bin/env python3
"""Generate tests/golden/golden_pid.npz from the reference's two PID controllers, run unmodified.

Like gen_golden.py this runs only where the reference tree is present (REF below); only the
fixture it writes is committed. The controllers import with three workarounds: tools/refstubs ahead
of the reference on sys.path (gymnasium, mujoco), an empty stand-in registered as mujoco.viewer,
and os.makedirs neutralised during the import (pid_controller_world_frame.py:36-41 creates plot
directories beside itself).

Fixture contents
  (a) call sequences, both modes (prefix yaw_ / world_): state, target9, action, diag
      (des_rate 3, des_att 3), integ (xy 2, z, rate 3) after each call; integrators carried within
      runs of RUN calls. compute() is handed the float32 state / target values as float64 arrays:
      handed float32 arrays, NumPy 2 evaluates the position error, the integrator increments and
      cos / sin of the scalar angles in float32, which no float64 law reproduces to the fixture's
      1e-12 / 1e-9 bars. The float32-input actions are recorded too (action_f32in) and agree with
      the float64-input ones far inside one float32 rounding step.
  (b) closed-loop hover episodes of each controller on the reference HoverEnv (oracle physics),
      reset(seed=0..7): reset qpos / qvel / target, per-step reward and the info["state"] columns the
      comparisons and the score read (position, yaw rate), and the first KEEP actions.
  (c) the reference's analyze_yaw_oscillation / analyze_position_tracking /
      compute_performance_score outputs for those episodes.

Usage:  python tools/gen_golden_pid.py  [--out tests/golden]
"""
from __future__ import annotations

import argparse
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as GG  # noqa: E402  (the reference / stub / oracle setup)

RUN = 50       # calls per integrator run
N_RUNS = 24    # runs per mode: 1,200 rows per mode
KEEP = 200      # closed-loop steps whose actions are kept (the GPU comparison's horizon)
SEEDS = range(8)
ANALYSIS_KEYS = ("rate_mean", "rate_std", "rate_max", "zero_crossings", "oscillation_freq", "oscillation_energy",
                 "pos_error_mean", "pos_error_std", "pos_error_max", "total_reward", "episode_length",
                 "yaw_score", "pos_score", "total_score")


def _import_controllers():
    GG._setup()
    import mujoco
    viewer = types.ModuleType("mujoco.viewer")
    sys.modules["mujoco.viewer"] = viewer
    mujoco.viewer = viewer
    real = os.makedirs
    os.makedirs = lambda *a, **k: None
    try:
        import auto_tune_pid
        import pid_controller
        import pid_controller_world_frame
    finally:
        os.makedirs = real
    return pid_controller, pid_controller_world_frame, auto_tune_pid


def _integ(c):
    return np.concatenate([np.asarray(c.xy_integral, np.float64), [float(c.z_integral)],
                           np.asarray(c.rate_int_torque, np.float64)])


def call_sequences(mod, world: bool, seed: int) -> dict:
    rng = np.random.default_rng(seed)
    S, T, A, A32, D, I = [], [], [], [], [], []
    for run in range(N_RUNS):
        c, c32 = mod.CascadedPIDController(), mod.CascadedPIDController()
        wide = run % 4 == 3  # every fourth run: wide attitude and rates; the others near hover
        for _ in range(RUN):
            while True:
                s = np.zeros(12)
                s[0:3] = rng.uniform(-1.0, 1.0, 3) + (0, 0, 1.0)
                s[3:5] = rng.uniform(-1.2, 1.2, 2) if wide else rng.uniform(-0.1, 0.1, 2)
                s[5] = rng.uniform(-3.0, 3.0) if wide else rng.uniform(-0.1, 0.1)
                s[6:9] = rng.uniform(-2.0, 2.0, 3) if wide else rng.uniform(-0.2, 0.2, 3)
                s[9:12] = rng.uniform(-4.0, 4.0, 3) if wide else rng.uniform(-0.3, 0.3, 3)
                t = np.zeros(9)
                t[0:3] = s[0:3] + (rng.uniform(-1.5, 1.5, 3) if wide else rng.uniform(-0.15, 0.15, 3))
                if world:
                    t[3:6] = rng.uniform(-1.0, 1.0, 3)
                    t[6:9] = rng.uniform(-1.0, 1.0, 3)
                s32, t32 = s.astype(np.float32), t.astype(np.float32)
                if world:  # keep clear of the yaw-error wrap and of the velocity-norm switch
                    vn = float(np.hypot(float(t32[3]), float(t32[4])))
                    if 1e-7 < vn < 1e-5:
                        continue
                    e = np.arctan2(float(t32[4]), float(t32[3])) - float(s32[5])
                    if abs(abs((e + np.pi) % (2 * np.pi) - np.pi) - np.pi) < 1e-3:
                        continue
                break
            s64, t64 = s32.astype(np.float64), t32.astype(np.float64)
            tgt = (t64[0:3], t64[3:6], t64[6:9]) if world else t64[0:3]
            tgt32 = (t32[0:3], t32[3:6], t32[6:9]) if world else t32[0:3]
            a, d = c.compute(s64, tgt)
            a32, _ = c32.compute(s32, tgt32)
            S.append(s32); T.append(t32); A.append(a); A32.append(a32)
            D.append(np.concatenate([d["des_rate"], d["des_att"]]).astype(np.float64))
            I.append(_integ(c))
    out = dict(state=np.array(S, np.float32), target9=np.array(T, np.float32), action=np.array(A, np.float32),
               action_f32in=np.array(A32, np.float32), diag=np.array(D, np.float64), integ=np.array(I, np.float64))
    # strictly inside the torque clip: |tau| below max_tau (x yaw_torque_scale for yaw), max_tau
    # recomputed from the thrust the action carries, with a 1e-5 margin over its float32 rounding
    lim = mod.DEFAULT_GAINS["limits"]
    a64 = out["action"].astype(np.float64)
    thrust = (a64[:, 0] + 1.0) * 0.5 * mod.MAX_TOTAL_THRUST
    max_tau = np.minimum(thrust / 4.0 * 2.0 * mod.L * lim["torque_motor_fraction"], lim["torque_abs_max"])
    bound = max_tau[:, None] * np.array([1.0, 1.0, lim["yaw_torque_scale"]])
    free = np.abs(a64[:, 1:4]) * mod.MAX_TORQUE < bound * (1 - 1e-5)
    assert free.mean() >= 0.5, f"only {free.mean():.2f} of the torque components are inside their clip"
    print(f"  torque components strictly inside their clip: {free.mean():.3f}")
    print(f"  max |action(float64 in) - action(float32 in)| = {np.abs(out['action'] - out['action_f32in']).max():.3g}")
    return out


def episodes(mod, AT, world: bool) -> dict:
    from envs.hover_env import HoverEnv
    env = HoverEnv()
    L = env.max_episode_steps if hasattr(env, "max_episode_steps") else 512
    out = {k: [] for k in ("qpos0", "qvel0", "target", "length", "actions", "pos", "yaw_rate", "rewards")}
    ana = {k: [] for k in ANALYSIS_KEYS}
    for seed in SEEDS:
        obs, info = env.reset(seed=seed)
        c = mod.CascadedPIDController()
        c.reset()
        out["qpos0"].append(np.array(env.data.qpos, np.float64))
        out["qvel0"].append(np.array(env.data.qvel, np.float64))
        out["target"].append(np.array(info["target"], np.float32))
        acts = np.zeros((L, 4), np.float32); sts = np.zeros((L, 12), np.float32); rews = np.zeros(L, np.float64)
        m = {k: [] for k in ("times", "yaws", "yaw_rates", "positions", "pos_errors", "roll", "pitch", "rewards")}
        done, n = False, 0
        while not done:
            state = info["state"]
            tgt_pos = info.get("target", np.zeros(3))
            traj = (tgt_pos, info.get("target_vel", np.zeros(3)), info.get("target_acc", np.zeros(3)))
            action, _ = c.compute(state, traj if world else tgt_pos)
            obs, reward, terminated, truncated, info = env.step(action)
            done = terminated or truncated
            s = info["state"]
            acts[n] = action; sts[n] = s; rews[n] = reward
            n += 1
            # auto_tune_pid.py:66-80
            m["times"].append(n * 0.01); m["yaws"].append(s[5]); m["yaw_rates"].append(s[11])
            m["positions"].append(s[:3].copy())
            m["pos_errors"].append(float(np.linalg.norm(s[:3] - np.asarray(tgt_pos))))
            m["roll"].append(s[3]); m["pitch"].append(s[4]); m["rewards"].append(reward)
        out["length"].append(n); out["actions"].append(acts[:KEEP]); out["rewards"].append(rews)
        out["pos"].append(sts[:, 0:3]); out["yaw_rate"].append(sts[:, 11])
        ya, pa = AT.analyze_yaw_oscillation(m), AT.analyze_position_tracking(m)
        sc = AT.compute_performance_score(ya, pa)
        for k in ANALYSIS_KEYS:
            ana[k].append(float({**ya, **pa, **sc}[k]))
    res = {k: np.array(v) for k, v in out.items()}
    res["length"] = res["length"].astype(np.int32)
    res.update({"ana_" + k: np.array(v, np.float64) for k, v in ana.items()})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(GG.REPO, "tests", "golden"))
    a = ap.parse_args()
    yaw_mod, world_mod, AT = _import_controllers()
    fx = {}
    for name, mod, world in (("yaw", yaw_mod, False), ("world", world_mod, True)):
        for k, v in call_sequences(mod, world, 11 + int(world)).items():
            fx[f"{name}_{k}"] = v
        for k, v in episodes(mod, AT, world).items():
            fx[f"{name}_ep_{k}"] = v
    path = os.path.join(a.out, "golden_pid.npz")
    np.savez_compressed(path, **fx)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")
    for name in ("yaw", "world"):
        print(name, "lengths", fx[f"{name}_ep_length"], "returns", np.round(fx[f"{name}_ep_rewards"].sum(1), 1),
              "scores", np.round(fx[f"{name}_ep_ana_total_score"], 4))


if __name__ == "__main__":
    main()
