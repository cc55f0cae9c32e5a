#!/usr/bin/env python3
"""Timing of the policy's whole-episode evaluation, hover + RateControlWrapper x 512 steps (HIP events, warmed
up, 5 alternating repetitions), at 1,024 and 65,536 envs:

  fused_env / fused_deployed   quad_policy_episode: one launch, either observation mode
  loop                         evaluate_episodes' per-step body: quad_policy_act + quad_step + the torch
                               bookkeeping per step, a host sync every 64 steps
  rollout                      quad_rollout with deterministic = 1 for the same envs and steps: the yardstick.
                               It does strictly more per step (both nets, buffer rows, reset draws)

and, at the smaller size, the fused launch in each block shape (QUADENV_EPISODE_BLOCK x QUADENV_ROLLOUT_NT),
which is what episode_block_shape's choice rests on. The policy must fly its episodes to the limit (a policy
that loses them ends the launch early and measures nothing): pass one with --model, or the tool trains the
HPO-pin configuration first (tests/hpo_repro.py's, 500k steps). Survival is reported.

Also recorded: ten 10-episode evaluations (the HPO-pin run's in-training load) through the loop and through the
fused launch, and a deployed-mode alpha sweep of the policy (return, survival, velocity RMSE).

    python tools/policy_episode_bench.py [--model policy.pt] [--out profiles/policy_episode/bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from uav_reinforcement_learning_control_amd import _native as N  # noqa: E402
from uav_reinforcement_learning_control_amd import evaluate as EV  # noqa: E402
from uav_reinforcement_learning_control_amd.envs import QuadVecEnv  # noqa: E402
from uav_reinforcement_learning_control_amd.ppo.fused import FusedPolicy  # noqa: E402

WRAP = "RateControlWrapper"
SHAPES = (("64", "1"), ("64", "2"), ("256", "2"))  # (QUADENV_EPISODE_BLOCK, QUADENV_ROLLOUT_NT)


def _timed(fn) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)  # ms


def train_policy(seed: int = 0, steps: int = 500_000):
    import hpo_repro
    from uav_reinforcement_learning_control_amd.ppo import PPO
    env = QuadVecEnv(8, env="hover", wrapper=WRAP, device="cuda:0", seed=seed)
    model = PPO(env, hpo_repro.ppo_config(), seed=seed)
    t0 = time.perf_counter()
    while model.num_timesteps < steps:
        model.collect_rollouts()
        model.train()
    torch.cuda.synchronize()
    env.close()
    return model.policy, time.perf_counter() - t0


def _pin(shape):
    for k in ("QUADENV_EPISODE_BLOCK", "QUADENV_ROLLOUT_NT"):
        os.environ.pop(k, None)
    if shape is not None:
        os.environ["QUADENV_EPISODE_BLOCK"], os.environ["QUADENV_ROLLOUT_NT"] = shape


def bench_size(policy, n: int, T: int, reps: int, shapes: bool) -> dict:
    dev = torch.device("cuda", 0)
    fp = FusedPolicy(policy)
    fp.pack()
    env = QuadVecEnv(n, wrapper=WRAP, device=dev, seed=1, max_episode_steps=T, auto_reset=False)
    env.reset()
    start = env.get_state()
    renv = QuadVecEnv(n, wrapper=WRAP, device=dev, seed=1, max_episode_steps=T, auto_reset=True)
    renv.reset()
    f = dict(dtype=torch.float32, device=dev)
    rb = dict(obs_copy=torch.zeros(1, n, 12, **f), actions=torch.zeros(1, n, 4, **f), log_prob=torch.zeros(1, n, **f),
              value=torch.zeros(1, n, **f), episode_starts=torch.zeros(1, n, **f), rewards=torch.zeros(1, n, **f),
              last_obs=torch.zeros(n, 12, **f), last_start=torch.ones(n, **f), ep_ret=torch.zeros(n, **f),
              ep_len=torch.zeros(n, **f), stats=torch.zeros(N.POLICY_STAT_SLOTS, 3, dtype=torch.float64, device=dev))
    obs0 = torch.zeros(n, 12, **f)
    done = {}

    def restore():
        env.set_state(**start)
        renv.set_state(**start)
        env.observe(out=obs0)
        rb["last_obs"].copy_(obs0)
        rb["last_start"].fill_(1.0); rb["ep_ret"].zero_(); rb["ep_len"].zero_()
        torch.cuda.synchronize()

    def fused(mode, shape=None):
        def run():
            _pin(shape)
            done[mode] = fp.episode(env, max_steps=T, obs_mode=mode)
            _pin(None)
        return run

    act = EV._Actor(policy, n, dev)
    obs = torch.zeros(n, 12, **f)

    def loop():  # evaluate_episodes' body
        obs.copy_(obs0)
        ret = torch.zeros(n, dtype=torch.float64, device=dev)
        length = torch.zeros(n, dtype=torch.int32, device=dev)
        running = torch.ones(n, dtype=torch.bool, device=dev)
        terminated = torch.zeros(n, dtype=torch.bool, device=dev)
        for t in range(T):
            a = act(obs)
            _, rew, te, tr, _ = env.step(a, obs=obs, info="raw")
            ret += torch.where(running, rew.double(), 0.0)
            length += running.int()
            terminated |= running & te
            running &= ~(te | tr)
            if (t + 1) % 64 == 0 and not bool(running.any()):
                break

    def rollout():
        fp.rollout(renv, t0=0, steps=T, seed=0, gamma=0.99, deterministic=True, **rb)

    forms = [("fused_env", fused("env")), ("fused_deployed", fused("deployed")), ("loop", loop), ("rollout", rollout)]
    if shapes:
        forms += [(f"fused_env_b{b}_nt{nt}", fused("env", (b, nt))) for b, nt in SHAPES]
        forms += [(f"fused_deployed_b{b}_nt{nt}", fused("deployed", (b, nt))) for b, nt in SHAPES]
    with torch.no_grad():
        for _, fn in forms:  # warm-up: code objects, allocator
            restore()
            fn()
            torch.cuda.synchronize()
        ms = {k: [] for k, _ in forms}
        for _ in range(reps):  # alternate the forms
            for k, fn in forms:
                restore()
                ms[k].append(_timed(fn))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    rec = {"envs": n, "steps": T, "reps": reps,
           "ms": {k: [round(x, 3) for x in v] for k, v in ms.items()},
           "ms_median": {k: round(v, 3) for k, v in med.items()},
           "ms_range": {k: [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()},
           "ratio_to_rollout": {k: round(v / med["rollout"], 3) for k, v in med.items()},
           "loop_over_fused_env": round(med["loop"] / med["fused_env"], 1),
           "env_steps": {k: int(v["steps"].sum().item()) for k, v in done.items()}, "env_steps_full": n * T,
           "survival": {k: float((v["status"] == N.PID_TRUNCATED).float().mean().item()) for k, v in done.items()}}
    env.close(); renv.close()
    return rec


def eval_load(policy, evals: int = 10, episodes: int = 10) -> dict:
    """The HPO-pin run's in-training evaluations: `evals` calls of evaluate_episodes at `episodes` episodes."""
    out = {}
    for name, fused in (("loop", False), ("fused", True)):
        EV.evaluate_episodes(policy, episodes, wrapper=WRAP, device="cuda:0", seed=1, fused=fused)  # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(evals):
            EV.evaluate_episodes(policy, episodes, wrapper=WRAP, device="cuda:0", seed=100 + k, fused=fused)
        out[name + "_seconds"] = round(time.perf_counter() - t0, 4)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--model", default=None, help="policy archive / state dict (default: train the HPO-pin configuration)")
    ap.add_argument("--envs", type=int, nargs="+", default=[1024, 65536])
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--alphas", type=float, nargs="+", default=[0.0, 0.5, 0.8, 0.95])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "policy_episode", "bench.json"))
    ap.add_argument("--save-policy", default=None, help="write the policy's state dict here (reuse it with --model)")
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "policy_episode_bench.py needs the GPU"
    rec = {"device": torch.cuda.get_device_name(0), "env": "hover + RateControlWrapper"}
    if a.model:
        policy, _ = EV.load_policy(a.model, torch.device("cuda", 0))
        rec["policy"] = os.path.basename(a.model)
    else:
        policy, secs = train_policy()
        rec["policy"] = "HPO-pin configuration, seed 0, 500k steps"
        rec["train_seconds"] = round(secs, 2)
    chk = EV._policy_episodes(policy, 1024, WRAP, "hover", a.steps, torch.device("cuda", 0), 1)[0]
    rec["survival_1024"] = chk["survival"]
    rec["mean_reward_1024"] = chk["mean_reward"]
    print(f"policy: {rec['policy']}; survival over 1,024 episodes {100 * chk['survival']:.1f}%", flush=True)
    rec["sizes"] = [bench_size(policy, n, a.steps, a.reps, shapes=(n <= 4096)) for n in a.envs]
    rec["eval_load_10x10"] = eval_load(policy)
    sw = EV.evaluate_velocity_estimator(policy, a.alphas, 1024, max_steps=a.steps, closed_loop=True, wrapper=WRAP)
    ol = EV.evaluate_velocity_estimator(policy, a.alphas, 1024, max_steps=a.steps, closed_loop=False, wrapper=WRAP)
    rec["alpha_sweep"] = {"alphas": a.alphas, "episodes": 1024, "steps": a.steps,
                          "closed_loop": {k: [float(x) for x in sw[k]] for k in
                                          ("rmse", "mean_reward", "mean_length", "survival", "mean_pos_error")},
                          "open_loop_rmse": [float(x) for x in ol["rmse"]]}
    print(sw["table"], flush=True)
    print(json.dumps(rec))
    if a.out:
        d = os.path.dirname(os.path.abspath(a.out))
        os.makedirs(d, exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(rec, indent=1) + "\n")
    if a.save_policy:
        torch.save(policy.state_dict(), a.save_policy)
    return rec


if __name__ == "__main__":
    main()
