#!/usr/bin/env python3
"""Generate tests/golden/golden_ctrl.npz from the reference's SE(3), sliding-mode and LQR controllers,
run unmodified.

Like gen_golden_pid.py this runs only where the reference tree is present; only the fixture it writes is
committed. The controllers import with gen_golden_pid.py's workarounds (tools/refstubs ahead of the
reference, a stand-in mujoco.viewer, os.makedirs neutralised during the import), with tools/refstubs/control
for lqr_controller_world_frame.py's `import control`, and with print silenced while a controller is
constructed (the SE(3) and LQR constructors print).

Fixture contents
  (a) call sequences, prefixes se3h_ (SE(3), position-only target: zero target velocity, so the desired yaw
      is the current yaw), se3_ (SE(3), trajectory target), smc_, lqr_: state, target9, action, action_f32in,
      diag (des_rate 3, des_att 3, |e_R| or 0), cstate (xy 2, z, rate 3, v_yaw, des_wz_prev) after each
      call; controller state carried within runs of RUN calls; every fourth run wide. compute() is handed
      the float32 values as float64 arrays (see gen_golden_pid.py). A sample is redrawn until
      tests/ctrl_ref.py, run beside the reference from the reference's own state, reports it at least
      1e-3 away from every branch threshold and integrator clip edge (CtrlRef.margin_all).
  (b) closed-loop hover episodes on the reference HoverEnv (oracle physics), reset(seed=0..7), prefixes
      se3_hov_ (as written), se3nq_hov_ (np.linalg.qr skipped: the module's np.linalg.qr replaced by one
      that returns its argument, for those episodes only), smc_hov_, lqr_hov_: reset qpos / qvel / target,
      length, return, the first KEEP positions, and `cut`: the first step at which the run came within
      1e-4 of a discontinuity of its law (CtrlRef.margin_branch), or the recorded length.
  (c) closed-loop trajectory episodes on the reference TrajectoryFollowEnv, two seeds, the first KEEP steps:
      the state and target the law read, its action, length and return, and `cut` as in (b); prefixes
      se3_traj_, smc_traj_, lqr_traj_.
  (d) lqr_K: the gain row the LQR constructor computed.

Usage:  python tools/gen_golden_ctrl.py  [--out tests/golden]
"""
from __future__ import annotations

import argparse
import builtins
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as GG  # noqa: E402  (the reference / stub / oracle setup)

RUN = 50      # calls per run
N_RUNS = 8    # runs per sequence
KEEP = 300    # closed-loop steps kept
SEEDS = range(8)
TRAJ_SEEDS = (0, 1)
MARGIN = 1e-3
CUT = 1e-4


def _quiet(make):
    real = builtins.print
    builtins.print = lambda *a, **k: None
    try:
        return make()
    finally:
        builtins.print = real


def _import_controllers():
    GG._setup()
    sys.path.insert(0, os.path.join(GG.REPO, "tests"))
    import mujoco
    viewer = types.ModuleType("mujoco.viewer")
    sys.modules["mujoco.viewer"] = viewer
    mujoco.viewer = viewer
    real = os.makedirs
    os.makedirs = lambda *a, **k: None
    try:
        import lqr_controller_world_frame
        import se3_geometric_controller
        import smc_controller_world_frame
    finally:
        os.makedirs = real
    return {"se3": (se3_geometric_controller, "SE3GeometricController"),
            "smc": (smc_controller_world_frame, "CascadedPIDController"),
            "lqr": (lqr_controller_world_frame, "CascadedPIDController")}


def _make(mods, law):
    mod, cls = mods[law]
    return _quiet(getattr(mod, cls))


def _cstate(c):
    return np.concatenate([np.asarray(c.xy_integral, np.float64), [float(c.z_integral)],
                           np.asarray(c.rate_int_torque, np.float64),
                           [float(getattr(c, "v_yaw", 0.0)), float(getattr(c, "des_wz_prev", 0.0))]])


def _diag(law, d):
    extra = [float(d["attitude_error"])] if law == "se3" else [0.0]
    return np.concatenate([d["des_rate"], np.asarray(d["des_att"], np.float64), extra]).astype(np.float64)


def call_sequences(mods, law: str, traj: bool, seed: int) -> dict:
    import ctrl_ref
    rng = np.random.default_rng(seed)
    S, T, A, A32, D, C, X0 = [], [], [], [], [], [], []
    redraws = 0
    for run in range(N_RUNS):
        c, c32 = _make(mods, law), _make(mods, law)
        shadow = ctrl_ref.CtrlRef(law)
        wide = run % 4 == 3
        for _ in range(RUN):
            while True:
                s = np.zeros(12)
                s[0:3] = rng.uniform(-1.0, 1.0, 3) + (0, 0, 1.0)
                s[3:5] = rng.uniform(-1.2, 1.2, 2) if wide else rng.uniform(-0.1, 0.1, 2)
                s[5] = rng.uniform(-3.0, 3.0)  # every heading: both signs of x_d[0]
                s[6:9] = rng.uniform(-2.0, 2.0, 3) if wide else rng.uniform(-0.2, 0.2, 3)
                s[9:12] = rng.uniform(-4.0, 4.0, 3) if wide else rng.uniform(-0.3, 0.3, 3)
                t = np.zeros(9)
                t[0:3] = s[0:3] + (rng.uniform(-1.5, 1.5, 3) if wide else rng.uniform(-0.15, 0.15, 3))
                if traj:
                    t[3:6] = rng.uniform(-1.0, 1.0, 3)
                    t[6:9] = rng.uniform(-1.0, 1.0, 3)
                s32, t32 = s.astype(np.float32), t.astype(np.float32)
                shadow.state[:] = _cstate(c)
                shadow.compute(s32, t32)
                if shadow.margin_all >= MARGIN:
                    break
                redraws += 1
            s64, t64 = s32.astype(np.float64), t32.astype(np.float64)
            tgt = (t64[0:3], t64[3:6], t64[6:9]) if traj else t64[0:3]
            tgt32 = (t32[0:3], t32[3:6], t32[6:9]) if traj else t32[0:3]
            a, d = c.compute(s64, tgt)
            a32, _ = c32.compute(s32, tgt32)
            S.append(s32); T.append(t32); A.append(a); A32.append(a32); D.append(_diag(law, d)); C.append(_cstate(c))
            X0.append(getattr(shadow, "xd0", 0.0))
    out = dict(state=np.array(S, np.float32), target9=np.array(T, np.float32), action=np.array(A, np.float32),
               action_f32in=np.array(A32, np.float32), diag=np.array(D, np.float64), cstate=np.array(C, np.float64))
    mod = mods[law][0]
    lim = mod.DEFAULT_GAINS["limits"]
    a64 = out["action"].astype(np.float64)
    # strictly inside the torque clip (gen_golden_pid.py): SE(3)'s thrust is the clipped |thrust vector|, the
    # cascades' is the tilt-compensated one; the action carries either
    thrust = (a64[:, 0] + 1.0) * 0.5 * mod.MAX_TOTAL_THRUST
    max_tau = np.minimum(thrust / 4.0 * 2.0 * mod.L * lim["torque_motor_fraction"], lim["torque_abs_max"])
    bound = max_tau[:, None] * np.array([1.0, 1.0, lim["yaw_torque_scale"]])
    free = np.abs(a64[:, 1:4]) * mod.MAX_TORQUE < bound * (1 - 1e-5)
    assert free.mean() >= 0.5, f"only {free.mean():.2f} of the torque components are inside their clip"
    if law == "se3":
        pos = np.mean(np.array(X0) > 0)
        assert 0.25 <= pos <= 0.75, f"x_d[0] > 0 on {pos:.2f} of the rows"
        print(f"  x_d[0] > 0 on {pos:.3f} of the rows")
    print(f"  {law}{'' if traj else ' (position target)'}: {redraws} redraws; torque components inside their clip "
          f"{free.mean():.3f}; max |action(f64 in) - action(f32 in)| = "
          f"{np.abs(out['action'] - out['action_f32in']).max():.3g}")
    return out


def episodes(mods, law: str, kind: str, reortho: bool = True) -> dict:
    import ctrl_ref
    if kind == "hover":
        from envs.hover_env import HoverEnv as Env
        seeds = SEEDS
    else:
        from envs.trajectory_follow_env import TrajectoryFollowEnv as Env
        seeds = TRAJ_SEEDS
    env = Env()
    mod = mods[law][0]
    real_qr = np.linalg.qr
    keys = ("qpos0", "qvel0", "target", "length", "ret", "pos", "cut") + (("state", "target9", "actions") if kind != "hover" else ())
    out = {k: [] for k in keys}
    for seed in seeds:
        obs, info = env.reset(seed=seed)
        c = _make(mods, law)
        c.reset()
        shadow = ctrl_ref.CtrlRef(law, se3_reorthonormalize=reortho)
        out["qpos0"].append(np.array(env.data.qpos, np.float64))
        out["qvel0"].append(np.array(env.data.qvel, np.float64))
        out["target"].append(np.array(info["target"], np.float32))
        pos = np.zeros((KEEP, 3), np.float32)
        st = np.zeros((KEEP, 12), np.float32); t9 = np.zeros((KEEP, 9), np.float32); acts = np.zeros((KEEP, 4), np.float32)
        done, n, ret, cut = False, 0, 0.0, None
        while not done:
            state = info["state"]
            tgt_pos = info.get("target", np.zeros(3))
            traj = (tgt_pos, info.get("target_vel", np.zeros(3)), info.get("target_acc", np.zeros(3)))
            tgt = traj if kind != "hover" else tgt_pos
            t9n = np.concatenate([np.asarray(x, np.float64).reshape(3) for x in traj]) if kind != "hover" \
                else np.concatenate([np.asarray(tgt_pos, np.float64), np.zeros(6)])
            shadow.state[:] = _cstate(c)
            shadow.compute(state, t9n)
            if cut is None and shadow.margin_branch < CUT:
                cut = n
            if not reortho:
                mod.np.linalg.qr = lambda a: (a, None)
            try:
                action, _ = c.compute(state, tgt)
            finally:
                mod.np.linalg.qr = real_qr
            if n < KEEP:
                st[n], t9[n], acts[n] = state, t9n, action
            obs, reward, terminated, truncated, info = env.step(action)
            done = terminated or truncated
            if n < KEEP:
                pos[n] = info["state"][:3]
            ret += float(reward)
            n += 1
        out["length"].append(n); out["ret"].append(ret); out["pos"].append(pos)
        out["cut"].append(min(n, KEEP) if cut is None else min(cut, KEEP))
        if kind != "hover":
            out["state"].append(st); out["target9"].append(t9); out["actions"].append(acts)
    res = {k: np.array(v) for k, v in out.items()}
    res["length"] = res["length"].astype(np.int32)
    res["cut"] = res["cut"].astype(np.int32)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(GG.REPO, "tests", "golden"))
    a = ap.parse_args()
    mods = _import_controllers()
    fx = {"lqr_K": np.asarray(_make(mods, "lqr").K, np.float64).reshape(-1)}
    for prefix, law, traj, seed in (("se3h", "se3", False, 21), ("se3", "se3", True, 22), ("smc", "smc", True, 23),
                                    ("lqr", "lqr", True, 24)):
        for k, v in call_sequences(mods, law, traj, seed).items():
            fx[f"{prefix}_{k}"] = v
    for prefix, law, reortho in (("se3", "se3", True), ("se3nq", "se3", False), ("smc", "smc", True), ("lqr", "lqr", True)):
        for k, v in episodes(mods, law, "hover", reortho).items():
            fx[f"{prefix}_hov_{k}"] = v
        print(prefix, "hover lengths", fx[f"{prefix}_hov_length"], "returns", np.round(fx[f"{prefix}_hov_ret"], 1),
              "cut", fx[f"{prefix}_hov_cut"])
    for law in ("se3", "smc", "lqr"):
        for k, v in episodes(mods, law, "trajectory").items():
            if k not in ("qpos0", "qvel0", "target", "pos"):
                fx[f"{law}_traj_{k}"] = v
        print(law, "trajectory lengths", fx[f"{law}_traj_length"], "returns", np.round(fx[f"{law}_traj_ret"], 1),
              "cut", fx[f"{law}_traj_cut"])
    path = os.path.join(a.out, "golden_ctrl.npz")
    np.savez_compressed(path, **fx)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")
    assert os.path.getsize(path) <= 657290
    print("lqr_K", fx["lqr_K"])


if __name__ == "__main__":
    main()
