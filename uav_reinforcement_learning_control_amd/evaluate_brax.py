"""Brax-profile evaluation driver (the reference's evaluate_brax_ppo.py on the MI355X env).

    python -m uav_reinforcement_learning_control_amd.evaluate_brax --summary models_brax/<run>/training_summary.json

The arguments, their defaults and the ``--summary`` precedence are evaluate_brax_ppo.py's (:201-273): a summary
overrides --env, --traj-duration-seconds and --episode-length; it supplies --params, --policy-hidden-sizes and
--activation only where the command line left them out; what neither gives falls to "256,256,256" / "silu".

Accepted and ignored (JAX / MJX or value-net settings with nothing to configure here): --xml, --backend, --impl,
--action-min, --action-max, --value-hidden-sizes. No counterpart: --checkpoint-path (Orbax checkpoints are not
read; a summary's checkpoint_dir is ignored) -- giving it without --params is an error.

The reference flies its episodes one after another on one env; here the ``--episodes`` episodes are the N envs of one
handle, reset from ``--seed``, and fly together: in ONE launch (quad_brax_episode) when the policy has two hidden
layers of the MFMA family, in a torch forward + env step loop otherwise (the default three-layer net among them).
Outputs, as the reference writes them under <plots-dir>/brax_eval_<stamp>/: the per-episode lines and the final block
on stdout, trajectory_error_per_episode.csv, evaluation_summary.json, and the three plots if matplotlib imports.
"""
from __future__ import annotations

import argparse
import json
import os
from datetime import datetime

import numpy as np

CSV_HEADER = "episode,mean_traj_error,rmse_traj_error,return,length"
SUMMARY_KEYS = ("env", "params", "policy_hidden_sizes", "value_hidden_sizes", "activation", "episodes",
                "deterministic", "mean_return", "mean_length", "mean_traj_error", "mean_rmse_traj_error",
                "plot_paths", "csv_path")
PLOT_ENVS = 16  # episodes whose per-step traces are kept for the plots


def _sizes(v: str):
    items = [x.strip() for x in v.split(",") if x.strip()]
    if not items:
        raise ValueError("Hidden layer sizes cannot be empty.")
    out = tuple(int(x) for x in items)
    if any(x <= 0 for x in out):
        raise ValueError("All hidden layer sizes must be positive integers.")
    return out


def parse(argv=None):
    ap = argparse.ArgumentParser(description="Evaluate Brax PPO checkpoint")
    ap.add_argument("--summary", default=None, help="Path to training_summary.json")
    ap.add_argument("--params", default=None, help="Path to ppo_params.msgpack")
    ap.add_argument("--checkpoint-path", default=None, help="no counterpart: Orbax checkpoints are not read")
    ap.add_argument("--env", default="hover", choices=["hover", "jax_mjx_quad"])
    ap.add_argument("--xml", default=None, help="ignored")
    ap.add_argument("--backend", default="mjx", help="ignored")
    ap.add_argument("--impl", default="jax", help="ignored")
    ap.add_argument("--traj-duration-seconds", type=float, default=5.0)
    ap.add_argument("--episode-length", type=int, default=500)
    ap.add_argument("--action-min", type=float, default=0.0, help="ignored")
    ap.add_argument("--action-max", type=float, default=13.0, help="ignored")
    ap.add_argument("--policy-hidden-sizes", default=None)
    ap.add_argument("--value-hidden-sizes", default=None, help="ignored (reported in the summary)")
    ap.add_argument("--activation", default=None, choices=["silu", "relu", "tanh"])
    ap.add_argument("--episodes", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--deterministic", action="store_true")
    ap.add_argument("--max-steps", type=int, default=None)
    ap.add_argument("--plots-dir", default="plots")
    return ap.parse_args(argv)


def resolve(a, summary=None):
    """evaluate_brax_ppo.py:225-273 on the parsed arguments: the summary's precedence, then the defaults."""
    if a.summary and summary is None:
        with open(a.summary, "r", encoding="utf-8") as f:
            summary = json.load(f)
    if summary is not None:
        a.env = summary.get("env", a.env)
        a.traj_duration_seconds = summary.get("traj_duration_seconds", a.traj_duration_seconds)
        a.episode_length = int(summary.get("episode_length", a.episode_length))
        if a.params is None:
            a.params = summary.get("params_path", a.params)
        if a.policy_hidden_sizes is None and summary.get("policy_hidden_sizes") is not None:
            a.policy_hidden_sizes = ",".join(str(v) for v in summary["policy_hidden_sizes"])
        if a.value_hidden_sizes is None and summary.get("value_hidden_sizes") is not None:
            a.value_hidden_sizes = ",".join(str(v) for v in summary["value_hidden_sizes"])
        if a.activation is None and summary.get("activation") is not None:
            a.activation = summary["activation"]
    if a.params is None:
        if a.checkpoint_path is not None:
            raise ValueError("--checkpoint-path: Orbax checkpoints are not read here; give --params")
        raise ValueError("Provide --params (or --summary containing params_path)")
    if a.policy_hidden_sizes is None:
        a.policy_hidden_sizes = "256,256,256"
    if a.value_hidden_sizes is None:
        a.value_hidden_sizes = "256,256,256"
    if a.activation is None:
        a.activation = "silu"
    return a


def episode_errors(err_sum, err_sq_sum, err_count):
    """(mean, rmse) per episode from the sums; nan where no step's error was finite (evaluate_brax_ppo.py:354-359)."""
    s, q, c = (np.asarray(x, np.float64) for x in (err_sum, err_sq_sum, err_count))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(c > 0, s / c, np.nan), np.where(c > 0, np.sqrt(q / c), np.nan)


def write_outputs(plot_dir, a, params_source, returns, lengths, mean_err, rmse_err, plot_paths=None, out=print):
    """The reference's per-episode lines, CSV, summary JSON and final block (evaluate_brax_ppo.py:364-419)."""
    n = len(returns)
    for i in range(n):
        out(f"episode={i} return={returns[i]:.4f} length={int(lengths[i])} "
            f"mean_traj_error={mean_err[i]:.6f} rmse_traj_error={rmse_err[i]:.6f}")
    mean_return = float(sum(float(r) for r in returns) / n)
    mean_length = float(sum(int(l) for l in lengths) / n)
    fm, fr = [v for v in mean_err if np.isfinite(v)], [v for v in rmse_err if np.isfinite(v)]
    mean_traj_error = float(np.mean(fm)) if fm else float("nan")
    mean_rmse_error = float(np.mean(fr)) if fr else float("nan")
    os.makedirs(plot_dir, exist_ok=True)
    csv_path = os.path.join(plot_dir, "trajectory_error_per_episode.csv")
    with open(csv_path, "w", encoding="utf-8") as f:
        f.write(CSV_HEADER + "\n")
        for i in range(n):
            f.write(f"{i},{float(mean_err[i])},{float(rmse_err[i])},{float(returns[i])},{int(lengths[i])}\n")
    summary_path = os.path.join(plot_dir, "evaluation_summary.json")
    summary = {"env": a.env, "params": params_source, "policy_hidden_sizes": list(_sizes(a.policy_hidden_sizes)),
               "value_hidden_sizes": list(_sizes(a.value_hidden_sizes)), "activation": a.activation,
               "episodes": n, "deterministic": bool(a.deterministic), "mean_return": mean_return,
               "mean_length": mean_length, "mean_traj_error": mean_traj_error,
               "mean_rmse_traj_error": mean_rmse_error, "plot_paths": plot_paths, "csv_path": csv_path}
    with open(summary_path, "w", encoding="utf-8") as f:
        json.dump(summary, f, indent=2)
    out("---")
    out(f"env={a.env} params={params_source}")
    out(f"episodes={n} deterministic={bool(a.deterministic)}")
    out(f"mean_return={mean_return:.4f} mean_length={mean_length:.2f}")
    out(f"mean_traj_error={mean_traj_error:.6f} mean_rmse_traj_error={mean_rmse_error:.6f}")
    out(f"saved_eval_summary={summary_path}")
    if plot_paths is not None:
        out(f"saved_plot_curve={plot_paths['curve']}")
        out(f"saved_plot_hist={plot_paths['hist']}")
        out(f"saved_plot_traj3d={plot_paths['traj3d']}")
    out(f"saved_error_csv={csv_path}")
    return summary


def _save_plots(pos, tgt, lengths, plot_dir):
    """evaluate_brax_ppo.py:128-197 for the traced episodes: pos, tgt [T, M, 3], lengths [M]."""
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except Exception as exc:
        print(f"plot_warning=matplotlib_unavailable reason={exc}")
        return None
    os.makedirs(plot_dir, exist_ok=True)
    errs = []
    for i, L in enumerate(lengths):
        e = np.linalg.norm(pos[:L, i] - tgt[:L, i], axis=-1)
        errs.append(e[np.isfinite(e)])
    fig, ax = plt.subplots(figsize=(10, 5))
    for i, e in enumerate(errs):
        if len(e):
            ax.plot(np.arange(len(e)), e, label=f"ep{i}", alpha=0.85, marker="o", markersize=2)
    ax.set_title(f"Trajectory Following Error per Step (non-empty episodes={sum(len(e) > 0 for e in errs)})")
    ax.set_xlabel("Step")
    ax.set_ylabel("Position Error (L2)")
    if len(errs) <= 10:
        ax.legend()
    ax.grid(True, alpha=0.3)
    fig.tight_layout()
    paths = {"curve": os.path.join(plot_dir, "trajectory_error_curve.png")}
    fig.savefig(paths["curve"], dpi=160)
    plt.close(fig)
    fig, ax = plt.subplots(figsize=(8, 5))
    ax.hist(np.concatenate(errs) if errs else np.zeros(0), bins=40)
    ax.set_title("Trajectory Error Distribution")
    ax.set_xlabel("Position Error (L2)")
    ax.set_ylabel("Count")
    ax.grid(True, alpha=0.3)
    fig.tight_layout()
    paths["hist"] = os.path.join(plot_dir, "trajectory_error_hist.png")
    fig.savefig(paths["hist"], dpi=160)
    plt.close(fig)
    fig = plt.figure(figsize=(8, 6))
    ax = fig.add_subplot(111, projection="3d")
    for i, L in enumerate(lengths):
        if L:
            ax.plot(pos[:L, i, 0], pos[:L, i, 1], pos[:L, i, 2], label=f"actual_ep{i}")
            ax.plot(tgt[:L, i, 0], tgt[:L, i, 1], tgt[:L, i, 2], linestyle="--", label=f"target_ep{i}")
    ax.set_title("3D Trajectory: Actual vs Target")
    ax.set_xlabel("X")
    ax.set_ylabel("Y")
    ax.set_zlabel("Z")
    if len(lengths) <= 5:
        ax.legend(loc="best")
    fig.tight_layout()
    paths["traj3d"] = os.path.join(plot_dir, "trajectory_3d_actual_vs_target.png")
    fig.savefig(paths["traj3d"], dpi=160)
    plt.close(fig)
    return paths


def _loop_episodes(env, policy, norm, dist, T, deterministic, seed, trace_envs):
    """The per-step form: torch forward + env.step on an auto_reset = 0 handle, the launch's metrics and traces."""
    import torch
    n, dev = env.num_envs, env.device
    gen = torch.Generator(device=dev)
    gen.manual_seed(int(seed))
    mean, std = (torch.as_tensor(norm[k], dtype=torch.float32, device=dev) for k in ("mean", "std"))
    f64 = dict(dtype=torch.float64, device=dev)
    res = dict(ret=torch.zeros(n, **f64), steps=torch.zeros(n, dtype=torch.int32, device=dev),
               err_sum=torch.zeros(n, **f64), err_sq_sum=torch.zeros(n, **f64),
               err_count=torch.zeros(n, dtype=torch.int32, device=dev))
    M = int(trace_envs)
    if M:
        res["pos"] = torch.zeros(T, M, 3, device=dev)
        res["target"] = torch.zeros(T, M, 3, device=dev)
    active = torch.ones(n, dtype=torch.bool, device=dev)
    obs = env.observe().clone()
    zero = torch.zeros((), **f64)
    with torch.no_grad():
        for t in range(T):
            logits = policy((obs - mean) / std)
            raw = dist.split(logits)[0] if deterministic else dist.sample_raw(logits, gen)
            o, rw, te, tr, info = env.step(torch.tanh(raw).contiguous(), info="full")
            err = torch.linalg.vector_norm(o[:, :3] - info["target"], dim=-1)
            ok = active & torch.isfinite(err)
            res["ret"] += torch.where(active, rw.double(), zero)
            res["steps"] += active.int()
            res["err_sum"] += torch.where(ok, err.double(), zero)
            res["err_sq_sum"] += torch.where(ok, err.double() ** 2, zero)
            res["err_count"] += ok.int()
            if M:
                res["pos"][t] = torch.where(active[:M, None], o[:M, :3], res["pos"][t])
                res["target"][t] = torch.where(active[:M, None], info["target"][:M], res["target"][t])
            active &= ~(te | tr)
            obs = o.clone()
            if t % 16 == 15 and not bool(active.any()):
                break
    return res


def main(argv=None):
    import torch

    from .envs import QuadVecEnv
    from .export import load_brax_params
    from .ppo.brax_ppo import BraxMLP, NormalTanh
    from .ppo.fused import FusedBraxActor, brax_launch_chosen

    a = resolve(parse(argv))
    a.params = os.path.abspath(a.params)
    norm, pol, _ = load_brax_params(a.params)
    sizes = _sizes(a.policy_hidden_sizes)
    print(f"Eval actor hidden sizes: {sizes}")
    print(f"Eval critic hidden sizes: {_sizes(a.value_hidden_sizes)}")
    print(f"Eval activation: {a.activation}")
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
    kind = {"hover": "brax_hover", "jax_mjx_quad": "brax_jax_mjx"}[a.env]
    env = QuadVecEnv(a.episodes, env=kind, seed=a.seed, max_episode_steps=a.episode_length, auto_reset=False,
                     cfg_overrides={"traj_duration": a.traj_duration_seconds})
    env.reset()
    T = a.max_steps if a.max_steps is not None else a.episode_length
    want_plots = True
    try:
        import matplotlib  # noqa: F401
    except Exception:
        want_plots = False
    M = min(a.episodes, PLOT_ENVS) if want_plots else 0
    if brax_launch_chosen(sizes, a.activation, env):
        actor = FusedBraxActor(pol, norm, activation=a.activation, device=env.device)
        actor.pack()
        res = actor.episode(env, max_steps=T, deterministic=a.deterministic, seed=a.seed, trace_envs=M)
        form = "one launch (quad_brax_episode)"
    else:
        net = BraxMLP((env.obs_dim, *sizes, 8), a.activation).to(env.device)
        net.load_flax_params(pol)
        res = _loop_episodes(env, net, norm, NormalTanh(4), T, a.deterministic, a.seed, M)
        form = "torch forward + env step loop"
    print(f"Eval form: {form}")
    torch.cuda.synchronize()
    returns, lengths = res["ret"].cpu().numpy(), res["steps"].cpu().numpy()
    mean_err, rmse_err = episode_errors(res["err_sum"].cpu().numpy(), res["err_sq_sum"].cpu().numpy(),
                                        res["err_count"].cpu().numpy())
    plot_dir = os.path.join(os.path.abspath(a.plots_dir), "brax_eval_" + datetime.now().strftime("%Y%m%d_%H%M%S"))
    plot_paths = None
    if M:
        plot_paths = _save_plots(res["pos"].cpu().numpy(), res["target"].cpu().numpy(), lengths[:M], plot_dir)
    else:
        print("plot_warning=matplotlib_unavailable reason=import failed")
    summary = write_outputs(plot_dir, a, a.params, returns, lengths, mean_err, rmse_err, plot_paths)
    env.close()
    return summary


if __name__ == "__main__":
    main()
