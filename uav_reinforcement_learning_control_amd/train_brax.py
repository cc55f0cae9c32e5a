"""Brax-profile PPO training driver (the reference's train_brax_ppo.py:432-680 on the MI355X env).

    python -m uav_reinforcement_learning_control_amd.train_brax --env jax_mjx_quad --num-envs 65536

Same arguments and defaults as train_brax_ppo.py where they apply (the JAX/MJX-specific --xml,
--impl, --backend and Orbax checkpoints have no counterpart here). --num-evals K runs brax's in-training
evaluation (K evaluations evenly spaced over the run on a separate eval env, BraxPPO.evaluate: one launch per
evaluation); its default here is 0, so a run without the flag prints and writes what it always did. --fused-unroll
collects each training step's unrolls in one launch (ppo/fused.py FusedBraxActor.unroll), off by default;
--fused-update computes each minibatch gradient in fused launches (ppo/fused.py FusedBraxLearner), off by default;
--fused-arch-update does so for every two-hidden-layer net of the Brax actor's family (tanh, SiLU, wider, policy and
value of different sizes: ppo/fused.py fused_brax_learner_for), off by default. Outputs mirror the
reference's run directory: <output-dir>/<timestamp>/ppo_params.msgpack (brax model.save_params
format, ppo/brax_ppo.py + export.save_brax_params), checkpoints/params_step_<n>.msgpack every
--checkpoint-interval steps, and training_summary.json.
"""
from __future__ import annotations

import argparse
import json
import os
import time
from datetime import datetime

import torch
import torch.distributed as dist

from .envs import QuadVecEnv
from .export import load_brax_params, save_brax_params
from .ppo.brax_ppo import BraxPPO, BraxPPOConfig


def _sizes(v: str):
    out = tuple(int(x) for x in v.split(",") if x.strip())
    if not out or any(x <= 0 for x in out):
        raise ValueError("hidden sizes must be positive integers")
    return out


def eval_schedule(num_timesteps: int, steps_per_training_step: int, num_evals: int):
    """The training-step counts after which an evaluation runs (0: before training). brax ppo.train (restated from
    the published algorithm, parity unpinned) runs max(num_evals - 1, 1) epochs of equal length with an evaluation
    after each, and one before training when num_evals > 1, sizing the epochs so that they reach num_timesteps.
    The run here is the fixed number of training steps that reaches num_timesteps, so epoch j ends after
    round(j * training steps / epochs) of them: num_evals evaluations, evenly spaced, the last at the end (fewer
    when the run has fewer training steps than epochs). Empty for num_evals <= 0."""
    if num_evals <= 0:
        return []
    total = max(1, -(-int(num_timesteps) // int(steps_per_training_step)))
    epochs = max(num_evals - 1, 1)
    pts = sorted({max(1, (2 * j * total + epochs) // (2 * epochs)) for j in range(1, epochs + 1)})
    return ([0] if num_evals > 1 else []) + pts


def progress_line(step: int, train_reward, eval_reward, sps: float) -> str:
    """train_brax_ppo.py:563-573's progress line."""
    fin = lambda v: v is not None and v == v and abs(v) != float("inf")
    if fin(eval_reward) and fin(train_reward):
        return f"step={step:,} train_reward={train_reward:.4f} eval_reward={eval_reward:.4f} sps={sps:.1f}"
    if fin(eval_reward):
        return f"step={step:,} eval_reward={eval_reward:.4f} sps={sps:.1f}"
    if fin(train_reward):
        return f"step={step:,} train_reward={train_reward:.4f} sps={sps:.1f}"
    return f"step={step:,} train_reward=invalid eval_reward=invalid sps={sps:.1f}"


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--env", default="hover", choices=["hover", "jax_mjx_quad"])
    ap.add_argument("--num-timesteps", type=int, default=2_000_000)
    ap.add_argument("--episode-length", type=int, default=500)
    ap.add_argument("--num-envs", type=int, default=1024, help="envs per GPU")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--learning-rate", type=float, default=3e-4)
    ap.add_argument("--entropy-cost", type=float, default=1e-3)
    ap.add_argument("--discounting", type=float, default=0.99)
    ap.add_argument("--traj-duration-seconds", type=float, default=5.0)
    ap.add_argument("--unroll-length", type=int, default=10)
    ap.add_argument("--batch-size", type=int, default=1024)
    ap.add_argument("--num-minibatches", type=int, default=16)
    ap.add_argument("--num-updates-per-batch", type=int, default=4)
    ap.add_argument("--gae-lambda", type=float, default=0.95)
    ap.add_argument("--reward-scaling", type=float, default=1.0)
    ap.add_argument("--policy-hidden-sizes", default="128, 128")
    ap.add_argument("--value-hidden-sizes", default="128, 128")
    ap.add_argument("--activation", default="relu", choices=["silu", "relu", "tanh"])
    ap.add_argument("--checkpoint-interval", type=int, default=200_000)
    ap.add_argument("--restore-checkpoint-path", default=None, help="a params .msgpack to start from")
    ap.add_argument("--output-dir", default="models_brax")
    ap.add_argument("--num-evals", type=int, default=0,
                    help="in-training evaluations, evenly spaced (one before training when > 1); the reference's\n"
                         "default is 10, here 0: no evaluation, the output of a run without the flag is unchanged")
    ap.add_argument("--num-eval-envs", type=int, default=128, help="envs of the separate eval env (brax: 128)")
    ap.add_argument("--deterministic-eval", action="store_true", help="evaluate tanh(loc) instead of samples")
    ap.add_argument("--fused-unroll", action="store_true",
                    help="collect each training step's unrolls in one launch (Philox action noise) instead of the\n"
                         "torch per-step loop; needs a two-hidden-layer policy of the MFMA family. Off by default:\n"
                         "the output of a run without the flag is unchanged")
    ap.add_argument("--fused-update", action="store_true",
                    help="compute each minibatch gradient in four fused launches (quad_brax_ppo_grad, Philox entropy\n"
                         "noise) and step Adam with quad_clip_adam instead of torch autograd; needs (128, 128) ReLU\n"
                         "policy and value nets. Off by default: the output of a run without the flag is unchanged")
    ap.add_argument("--fused-arch-update", action="store_true",
                    help="the fused minibatch gradient for every two-hidden-layer policy and value net of the MFMA\n"
                         "family (h1 a multiple of 32 up to 512, h2 in 64 / 128 / 256, relu / tanh / silu, the two\n"
                         "nets' sizes independent): quad_brax_ppo_arch_grad, and quad_brax_ppo_grad for (128, 128)\n"
                         "ReLU. Off by default: the output of a run without the flag is unchanged")
    return ap.parse_args(argv)


def main(argv=None):
    a = parse(argv)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    if world > 1:
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    cfg = BraxPPOConfig(num_envs=a.num_envs, episode_length=a.episode_length, learning_rate=a.learning_rate,
                        entropy_cost=a.entropy_cost, discounting=a.discounting, unroll_length=a.unroll_length,
                        batch_size=a.batch_size, num_minibatches=a.num_minibatches,
                        num_updates_per_batch=a.num_updates_per_batch, gae_lambda=a.gae_lambda,
                        reward_scaling=a.reward_scaling, policy_hidden_sizes=_sizes(a.policy_hidden_sizes),
                        value_hidden_sizes=_sizes(a.value_hidden_sizes), activation=a.activation,
                        fused_unroll=a.fused_unroll, fused_update=a.fused_update,
                        fused_update_arch=a.fused_arch_update)
    kind = {"hover": "brax_hover", "jax_mjx_quad": "brax_jax_mjx"}[a.env]
    env = QuadVecEnv(a.num_envs, env=kind, device=f"cuda:{local}", seed=a.seed, env_id_base=rank * a.num_envs,
                     max_episode_steps=a.episode_length, cfg_overrides={"traj_duration": a.traj_duration_seconds})
    model = BraxPPO(env, cfg, seed=a.seed)
    if a.restore_checkpoint_path:
        norm, pol, val = load_brax_params(a.restore_checkpoint_path)
        model.net.policy.load_flax_params(pol)
        model.net.value.load_flax_params(val)
        for k in ("count", "mean", "summed_variance", "std"):
            getattr(model.norm, k).copy_(torch.as_tensor(norm[k]))
    if a.fused_unroll and rank == 0:
        print(f"unrolls: one launch per training step ({model.num_unrolls} x {cfg.unroll_length} steps, "
              f"quad_brax_unroll)", flush=True)
    if a.fused_update and rank == 0:
        print(f"update: fused minibatch gradient ({cfg.num_updates_per_batch} x {cfg.num_minibatches} steps of "
              f"quad_brax_ppo_grad + quad_clip_adam per training step)", flush=True)
    if a.fused_arch_update and not a.fused_update and rank == 0:
        print(f"update: fused minibatch gradient, general family (policy {tuple(cfg.policy_hidden_sizes)}, value "
              f"{tuple(cfg.value_hidden_sizes)}, {cfg.activation}: {cfg.num_updates_per_batch} x {cfg.num_minibatches} "
              f"steps of {type(model._learner).entry} + quad_clip_adam per training step)", flush=True)
    stamp = datetime.now().strftime("%Y%m%d_%H%M%S")
    run = os.path.abspath(os.path.join(a.output_dir, stamp))
    ckdir = os.path.join(run, "checkpoints")
    if rank == 0:
        os.makedirs(ckdir, exist_ok=True)
    # brax's eval_env: a second env of the same kind with its own key (here: the run's seed + 1, ids past the
    # training envs'), rank 0 only; each evaluation resets it, so each flies fresh episodes
    sched = eval_schedule(a.num_timesteps, cfg.unroll_length * model.num_unrolls * a.num_envs * world, a.num_evals)
    eval_env = None
    if sched and rank == 0:
        eval_env = QuadVecEnv(a.num_eval_envs, env=kind, device=f"cuda:{local}", seed=a.seed + 1,
                              env_id_base=world * a.num_envs, max_episode_steps=a.episode_length, auto_reset=False,
                              cfg_overrides={"traj_duration": a.traj_duration_seconds})
    eval_reward = None
    t0 = time.time()
    last_ck = 0
    stats = None
    done_steps = 0
    if 0 in sched and rank == 0:
        eval_reward, _ = model.evaluate(eval_env, deterministic=a.deterministic_eval)
        print(progress_line(0, None, eval_reward, 0.0), flush=True)
    while model.num_timesteps < a.num_timesteps:
        stats = model.training_step()
        done_steps += 1
        if rank == 0:
            sps = stats.env_steps * world / stats.seconds
            if done_steps in sched:
                eval_reward, _ = model.evaluate(eval_env, deterministic=a.deterministic_eval)
                print(progress_line(model.num_timesteps, stats.mean_episode_reward, eval_reward, sps), flush=True)
            else:
                print(f"step={model.num_timesteps:,} train_reward={stats.mean_episode_reward:.4f} sps={sps:.1f}",
                      flush=True)
            if a.checkpoint_interval > 0 and model.num_timesteps - last_ck >= a.checkpoint_interval:
                save_brax_params(os.path.join(ckdir, f"params_step_{model.num_timesteps}.msgpack"), model.params())
                last_ck = model.num_timesteps
    if rank == 0:
        params_path = save_brax_params(os.path.join(run, "ppo_params.msgpack"), model.params())
        summary = {"run_dir": run, "env": a.env, "num_timesteps": a.num_timesteps,
                   "episode_length": a.episode_length, "num_envs": a.num_envs * world, "seed": a.seed,
                   "learning_rate": a.learning_rate, "entropy_cost": a.entropy_cost,
                   "discounting": a.discounting, "unroll_length": a.unroll_length,
                   "batch_size": a.batch_size, "num_minibatches": a.num_minibatches,
                   "num_updates_per_batch": a.num_updates_per_batch, "gae_lambda": a.gae_lambda,
                   "reward_scaling": a.reward_scaling, "policy_hidden_sizes": list(cfg.policy_hidden_sizes),
                   "value_hidden_sizes": list(cfg.value_hidden_sizes), "activation": a.activation,
                   "traj_duration_seconds": a.traj_duration_seconds,
                   "checkpoint_interval": a.checkpoint_interval, "checkpoint_dir": ckdir,
                   "elapsed_sec": time.time() - t0,
                   "final_metrics": {"training/episode_reward": stats.mean_episode_reward if stats else None,
                                     **(stats.losses if stats else {})},
                   "params_path": params_path}
        if a.fused_unroll:
            summary["fused_unroll"] = True
        if a.fused_update:
            summary["fused_update"] = True
        if a.fused_arch_update:
            summary["fused_arch_update"] = True
        if a.num_evals > 0:
            summary["num_evals"] = a.num_evals
            summary["final_metrics"]["eval/episode_reward"] = eval_reward
        json.dump(summary, open(os.path.join(run, "training_summary.json"), "w"), indent=2)
        print(f"Saved parameters: {params_path}", flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
