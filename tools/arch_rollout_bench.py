"""Measure the SB3-profile rollout of nets other than 128-128 ReLU on the general family's rollout kernels
(PPOConfig.fused_rollout_arch: ppo.fused.FusedActorCritic, quad_actor_rollout / quad_actor_critic_act) against the
rollout those nets took before (the flag off: the captured torch PPO._rollout_step, the parent commit's path, the
yardstick); writes profiles/arch_rollout/bench.json and profiles/arch_rollout/README.md.

Rows: (64, 64) tanh, (256, 256) tanh and (512, 256) relu at (num_envs, n_steps) = (16, 1024) -- the reference's
train.py -- and (1024, 16). One process on one GPU, hover env with RateControlWrapper. The three forms are built with
the same seed, each on an env of its own:

  (a)  one launch     collect_rollouts with fused_rollout_arch and fused_rollout: quad_actor_critic_pack, one
                      quad_actor_rollout per chunk, the bootstrap value, GAE
  (a2) two launches   fused_rollout_arch without fused_rollout: quad_actor_critic_act + quad_step per step, replayed
                      from the captured graph, quad_actor_critic_post, the bootstrap value, GAE
  (b)  torch          the flag off: the captured torch per-step path, GAE

After one warm-up collect_rollouts of each (which captures the graphs), `--reps` runs of each form on a host clock
closed by a device synchronize; every run starts from the same restored env state, observation, carry tensors, noise
counters and parameters. train: PPO.train() of form (a)'s model with fused_update_arch, the median of three runs from
the same parameters and zeroed Adam state; the rollout's share of an iteration is rollout / (rollout + train).

Launches per step: the runtime's kernel-launch calls in torch's profiler trace of one eager collect_rollouts divided by
n_steps; null if the profiler is unavailable.

    python tools/arch_rollout_bench.py [--reps 5]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

ARCHS = (((64, 64), "tanh"), ((256, 256), "tanh"), ((512, 256), "relu"))
POINTS = ((16, 1024), (1024, 16))
FORMS = (("one_launch", True, True), ("two_launch", True, False), ("torch", False, False))
OUT_DIR = os.path.join(REPO, "profiles", "arch_rollout")
LAUNCH_CALLS = ("hipLaunchKernel", "hipExtModuleLaunchKernel", "hipModuleLaunchKernel", "hipExtLaunchKernel",
                "cudaLaunchKernel", "cuLaunchKernel")


def _model(hidden, act, n, T, arch, one):
    from uav_reinforcement_learning_control_amd.envs import QuadVecEnv
    from uav_reinforcement_learning_control_amd.ppo.ppo import PPO, PPOConfig
    env = QuadVecEnv(n, env="hover", wrapper="RateControlWrapper", device="cuda:0", seed=1)
    cfg = PPOConfig(n_steps=T, batch_size=n * T // 128, net_arch=hidden, activation=act, fused_update_arch=True,
                    fused_rollout_arch=arch, fused_rollout=one)
    return PPO(env, cfg, seed=1), env


def _restore(model, state, carry):
    """The env state, the observation, the carry tensors and both noise counters of the common start."""
    import torch
    torch.cuda.synchronize()
    model.env.set_state(**state)
    for k, v in carry.items():
        getattr(model, k).copy_(v)
    model._cursor.zero_()
    model._t_host = 0
    torch.manual_seed(7)


def _reset_params(model, params0):
    import torch
    with torch.no_grad():
        for p, q in zip(model.params, params0):
            p.copy_(q)
        for st in model.opt.state.values():
            for t in st.values():
                if torch.is_tensor(t):
                    t.zero_()


def _timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _launches(model, state, carry, steps):
    try:
        import torch
        from torch.profiler import ProfilerActivity, profile
        _restore(model, state, carry)
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            model.collect_rollouts(use_graph=False)
            torch.cuda.synchronize()
        n = sum(e.count for e in prof.key_averages() if e.key in LAUNCH_CALLS)
        return n / steps if n > 0 else None
    except Exception:  # the profiler's backend is optional
        return None


def measure(reps):
    import torch
    rows = []
    for hidden, act in ARCHS:
        for n, T in POINTS:
            forms = {name: _model(hidden, act, n, T, arch, one) for name, arch, one in FORMS}
            a = forms["one_launch"][0]
            assert a._one_launch and forms["two_launch"][0]._fp is not None and forms["torch"][0]._fp is None
            params0 = [p.detach().clone() for p in a.params]
            for m, _ in forms.values():
                assert all(torch.equal(p, q) for p, q in zip(params0, m.params))
                m.collect_rollouts()  # warm-up: the first reset, the graph captures
            torch.cuda.synchronize()
            state = a.env.get_state()
            carry = {k: getattr(a, k).clone() for k in ("last_obs", "last_start", "ep_ret", "ep_len")}
            times = {k: [] for k in forms}
            for rep in range(reps + 1):  # one more pass from the common start before the timed ones
                for name, (m, _) in forms.items():
                    _restore(m, state, carry)
                    t = _timed(m.collect_rollouts)
                    if rep > 0:
                        times[name].append(t)
            launches = {name: _launches(m, state, carry, T) for name, (m, _) in forms.items()}
            train = []
            for rep in range(4):
                _reset_params(a, params0)
                torch.manual_seed(7)
                t = _timed(a.train)
                if rep > 0:
                    train.append(t)
            for _, env in forms.values():
                env.close()
            row = {"net_arch": list(hidden), "activation": act, "num_envs": n, "n_steps": T, "reps": reps,
                   "train_ms": 1e3 * statistics.median(train), "train_ms_all": [1e3 * t for t in train]}
            for name, v in times.items():
                row[f"{name}_rollout_ms"] = 1e3 * statistics.median(v)
                row[f"{name}_rollout_ms_all"] = [1e3 * t for t in v]
                row[f"{name}_step_us"] = 1e6 * statistics.median(v) / T
                row[f"{name}_launches_per_step"] = launches[name]
                row[f"{name}_rollout_share"] = row[f"{name}_rollout_ms"] / (row[f"{name}_rollout_ms"] + row["train_ms"])
            row["torch_over_one_launch"] = row["torch_rollout_ms"] / row["one_launch_rollout_ms"]
            row["torch_over_two_launch"] = row["torch_rollout_ms"] / row["two_launch_rollout_ms"]
            rows.append(row)
            print(f"{hidden} {act} {n} x {T}: rollout (a) {row['one_launch_rollout_ms']:.2f} ms  (a2) "
                  f"{row['two_launch_rollout_ms']:.2f} ms  (b) {row['torch_rollout_ms']:.2f} ms  x"
                  f"{row['torch_over_one_launch']:.1f} | train {row['train_ms']:.0f} ms | share (b) "
                  f"{100 * row['torch_rollout_share']:.0f} % -> (a) {100 * row['one_launch_rollout_share']:.0f} %",
                  flush=True)
    return rows


def readme(doc) -> str:
    nc = lambda x: "not counted" if x is None else f"{x:.2f}"
    lines = ["# The SB3-profile rollout of tanh and wider nets: fused launches against the torch per-step path", "",
             "Written by `tools/arch_rollout_bench.py`; the numbers are `bench.json`'s.", "",
             f"Device: {doc['device']}; torch {doc['torch']}. {doc['workload']}.", "",
             "(a) one launch: `PPOConfig(fused_rollout_arch=True)`: `quad_actor_critic_pack`, one `quad_actor_rollout` "
             "per rollout, the bootstrap value and GAE. (a2) two launches: the same flag with `fused_rollout=False`: "
             "`quad_actor_critic_act` + `quad_step` per step, replayed from the captured graph. (b) torch: the flag "
             "off, the parent commit's captured `PPO._rollout_step`, in the same process. (b) is the yardstick.", "",
             "| net | envs x steps | rollout (a) ms | (a2) ms | (b) ms | (b) / (a) | us per step (a) | (a2) | (b) | "
             "launches per step (a, eager) | (a2) | (b) |",
             "|---|---|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|"]
    for g in doc["rows"]:
        lines.append(f"| {tuple(g['net_arch'])} {g['activation']} | {g['num_envs']:,} x {g['n_steps']:,} | "
                     f"{g['one_launch_rollout_ms']:.2f} | {g['two_launch_rollout_ms']:.2f} | {g['torch_rollout_ms']:.2f} | "
                     f"{g['torch_over_one_launch']:.1f} | {g['one_launch_step_us']:.1f} | {g['two_launch_step_us']:.1f} | "
                     f"{g['torch_step_us']:.1f} | {nc(g['one_launch_launches_per_step'])} | "
                     f"{nc(g['two_launch_launches_per_step'])} | {nc(g['torch_launches_per_step'])} |")
    lines += ["", "## The whole iteration (train() with fused_update_arch)", "",
              "| net | envs x steps | train ms | rollout's share (b) | (a2) | (a) | iteration (b) / (a) |",
              "|---|---|---:|---:|---:|---:|---:|"]
    for g in doc["rows"]:
        it = (g["torch_rollout_ms"] + g["train_ms"]) / (g["one_launch_rollout_ms"] + g["train_ms"])
        lines.append(f"| {tuple(g['net_arch'])} {g['activation']} | {g['num_envs']:,} x {g['n_steps']:,} | "
                     f"{g['train_ms']:.0f} | {100 * g['torch_rollout_share']:.0f} % | "
                     f"{100 * g['two_launch_rollout_share']:.0f} % | {100 * g['one_launch_rollout_share']:.1f} % | {it:.2f} |")
    losers = [g for g in doc["rows"] if g["torch_over_one_launch"] <= 1.0]
    lines.append("")
    if losers:
        lines.append("Rule (DESIGN 19 - 23): the fused rollout is taken where (a) < (b). It LOST at: " + "; ".join(
            f"{tuple(g['net_arch'])} {g['activation']} at {g['num_envs']} envs" for g in losers) +
            ". `ppo.fused.ARCH_ROLLOUT_KEEP_TORCH` must list those rows.")
    else:
        lines.append("Rule (DESIGN 19 - 23): the fused rollout is taken where (a) < (b). It won every row, so "
                     "`ppo.fused.ARCH_ROLLOUT_KEEP_TORCH` is empty.")
    return "\n".join(lines) + "\n"


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out-dir", default=OUT_DIR)
    a = ap.parse_args(argv)
    import torch
    rows = measure(a.reps)
    doc = {"workload": f"hover env with RateControlWrapper, medians of {a.reps} runs after a warm-up, every run from "
                       f"the same restored env state, carry tensors, noise counters and parameters; train: the median "
                       f"of three PPO.train() runs (20 epochs, 128 minibatches) with fused_update_arch",
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "rows": rows,
           "one_launch_faster_everywhere": all(g["torch_over_one_launch"] > 1.0 for g in rows)}
    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, "bench.json"), "w") as f:
        json.dump(doc, f, indent=1)
    with open(os.path.join(a.out_dir, "README.md"), "w") as f:
        f.write(readme(doc))
    print(f"wrote {a.out_dir}/bench.json and README.md")
    return 0


if __name__ == "__main__":
    sys.exit(main())
