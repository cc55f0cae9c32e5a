"""Measure the SB3-profile update of nets other than 128-128 ReLU on the general learner (PPOConfig.fused_update_arch:
ppo.learner.FusedArchLearner, quad_ppo_arch_grad + quad_clip_adam per minibatch step, the captured epoch) against the
update those nets took before (the flag off: torch autograd + torch Adam, the parent commit's path, the yardstick);
writes profiles/arch_update/bench.json and profiles/arch_update/README.md.

Rows: (64, 64) tanh, (256, 256) tanh and (512, 256) relu at (num_envs, n_steps, batch_size) = (16, 1024, 128) -- the
reference's train.py: 128 minibatches x 20 epochs = 2,560 minibatch steps per iteration -- and (1024, 16, 4096): 4 x 20 =
80 steps. One process on one GPU. Both forms are built with the same seed; the torch-path rollout of one fills the
buffers of both. After one warm-up train() of each, `--reps` runs of each form on a host clock closed by a device
synchronize; every run starts from the same parameters (the initial ones), zeroed Adam state (restored in place, so
the captured epoch's key holds) and the same buffers.

  train            PPO.train(): all epochs; per minibatch step: train / steps
  rollout          PPO.collect_rollouts(): the torch per-step path, the same for both forms
  iteration        rollout + train

Launches per minibatch step: the runtime's kernel-launch calls in torch's profiler trace of one eager epoch
(graph_update off for the count: a replayed graph is one call), divided by the epoch's steps; null if the profiler
is unavailable. One more row times FusedArchLearner.grads against FusedLearner.grads (quad_ppo_grad's specialised
kernels) on the 128-128 ReLU net, which ppo.learner.fused_learner_for keeps on the latter.

    python tools/arch_update_bench.py [--reps 5]
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
sys.path.insert(0, os.path.join(REPO, "tests"))

ARCHS = (((64, 64), "tanh"), ((256, 256), "tanh"), ((512, 256), "relu"))
POINTS = ((16, 1024, 128), (1024, 16, 4096))
OUT_DIR = os.path.join(REPO, "profiles", "arch_update")
LAUNCH_CALLS = ("hipLaunchKernel", "hipExtModuleLaunchKernel", "hipModuleLaunchKernel", "hipExtLaunchKernel",
                "cudaLaunchKernel", "cuLaunchKernel")
BUFS = ("buf_obs", "buf_act", "buf_logp", "buf_adv", "buf_ret")


def _model(hidden, act, n, T, B, fused):
    from uav_reinforcement_learning_control_amd.envs import QuadVecEnv
    from uav_reinforcement_learning_control_amd.ppo.ppo import PPO, PPOConfig
    env = QuadVecEnv(n, env="hover", wrapper="RateControlWrapper", device="cuda:0", seed=1)
    cfg = PPOConfig(n_steps=T, batch_size=B, net_arch=hidden, activation=act, fused_update_arch=fused)
    return PPO(env, cfg, seed=1), env


def _reset(model, params0):
    """The initial parameters and a zeroed Adam state, in place."""
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


def _launches(model, params0, steps_per_epoch):
    try:
        import torch
        from torch.profiler import ProfilerActivity, profile
        graph, model.cfg.graph_update = model.cfg.graph_update, False
        _reset(model, params0)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            model.train(n_epochs=1)
            torch.cuda.synchronize()
        model.cfg.graph_update = graph
        n = sum(e.count for e in prof.key_averages() if e.key in LAUNCH_CALLS)
        return n / steps_per_epoch if n >= steps_per_epoch else None
    except Exception:  # the profiler's backend is optional
        return None


def measure(reps):
    import torch
    rows = []
    for hidden, act in ARCHS:
        for n, T, B in POINTS:
            forms = {name: _model(hidden, act, n, T, B, fused) for name, fused in (("fused", True), ("torch", False))}
            src = forms["torch"][0]
            params0 = [p.detach().clone() for p in src.params]
            assert all(torch.equal(a, b) for a, b in zip(params0, forms["fused"][0].params))
            roll = [_timed(src.collect_rollouts) for _ in range(3)]
            for name in BUFS:
                getattr(forms["fused"][0], name).copy_(getattr(src, name))
            steps = src.cfg.n_epochs * (n * T // B)
            times = {k: [] for k in forms}
            for rep in range(reps + 1):  # the first pass warms up (and captures the epoch)
                for name, (model, _) in forms.items():
                    _reset(model, params0)
                    torch.manual_seed(7)
                    t = _timed(model.train)
                    if rep > 0:
                        times[name].append(t)
            launches = {name: _launches(m, params0, n * T // B) for name, (m, _) in forms.items()}
            for _, env in forms.values():
                env.close()
            row = {"net_arch": list(hidden), "activation": act, "num_envs": n, "n_steps": T, "batch_size": B,
                   "minibatch_steps": steps, "reps": reps, "rollout_ms": 1e3 * statistics.median(roll),
                   "rollout_ms_all": [1e3 * t for t in roll]}
            for name, v in times.items():
                row[f"{name}_train_ms"] = 1e3 * statistics.median(v)
                row[f"{name}_train_ms_all"] = [1e3 * t for t in v]
                row[f"{name}_minibatch_step_us"] = 1e6 * statistics.median(v) / steps
                row[f"{name}_iteration_ms"] = row[f"{name}_train_ms"] + row["rollout_ms"]
                row[f"{name}_rollout_share"] = row["rollout_ms"] / row[f"{name}_iteration_ms"]
                row[f"{name}_launches_per_minibatch_step"] = launches[name]
            row["torch_over_fused_train"] = row["torch_train_ms"] / row["fused_train_ms"]
            row["torch_over_fused_iteration"] = row["torch_iteration_ms"] / row["fused_iteration_ms"]
            rows.append(row)
            print(f"{hidden} {act} {n} x {T} / {B}: step fused {row['fused_minibatch_step_us']:.0f} us  torch "
                  f"{row['torch_minibatch_step_us']:.0f} us  x{row['torch_over_fused_train']:.1f} | train fused "
                  f"{row['fused_train_ms']:.0f} ms torch {row['torch_train_ms']:.0f} ms | rollout "
                  f"{row['rollout_ms']:.0f} ms", flush=True)
    return rows


def measure_128(reps):
    """FusedArchLearner.grads against FusedLearner.grads on the 128-128 ReLU net: medians of `reps` groups of 50 calls."""
    import torch
    import learner_arch_ref as R
    from uav_reinforcement_learning_control_amd.ppo.learner import FusedArchLearner, FusedLearner
    from uav_reinforcement_learning_control_amd.ppo.ppo import PPOConfig
    cfg = PPOConfig()
    pol = R.make_policy(0, (128, 128), "relu", "cuda")
    bufs = R.make_buffers(pol, 16384, 0, cfg.clip_range)
    out = []
    for B in (128, 4096):
        idx = torch.randperm(16384, device="cuda")[:B].contiguous()
        row = {"net_arch": [128, 128], "activation": "relu", "batch_size": B, "calls_per_group": 50, "reps": reps}
        for name, cls in (("general", FusedArchLearner), ("specialised", FusedLearner)):
            fl = cls(pol, cfg.clip_range, cfg.ent_coef, cfg.vf_coef, True)
            run = lambda: [fl.grads(*bufs, idx) for _ in range(50)]
            _timed(run)
            v = [_timed(run) / 50 for _ in range(reps)]
            row[f"{name}_grads_us"] = 1e6 * statistics.median(v)
            row[f"{name}_grads_us_all"] = [1e6 * t for t in v]
        row["general_over_specialised"] = row["general_grads_us"] / row["specialised_grads_us"]
        out.append(row)
        print(f"128-128 relu B {B}: general {row['general_grads_us']:.1f} us  specialised "
              f"{row['specialised_grads_us']:.1f} us (eager calls, host launch cost included)", flush=True)
    return out


def readme(doc) -> str:
    nc = lambda x: "not counted" if x is None else f"{x:.1f}"
    lines = ["# The SB3-profile update of tanh and wider nets: fused launches against torch autograd", "",
             "Written by `tools/arch_update_bench.py`; the numbers are `bench.json`'s.", "",
             f"Device: {doc['device']}; torch {doc['torch']}. {doc['workload']}.", "",
             "(a) fused: `PPOConfig(fused_update_arch=True)`: per minibatch step `quad_ppo_arch_grad` (three launches, "
             "the advantage sums once per epoch) and `quad_clip_adam` (two), the epoch replayed as one graph. (b) torch: "
             "the flag off, the parent commit's autograd update and torch Adam, in the same process.", "",
             "| net | envs x steps / batch | minibatch step (a) us | (b) us | (b) / (a) | launches per step (a, eager) | (b) |",
             "|---|---|---:|---:|---:|---:|---:|"]
    for g in doc["rows"]:
        lines.append(f"| {tuple(g['net_arch'])} {g['activation']} | {g['num_envs']:,} x {g['n_steps']:,} / "
                     f"{g['batch_size']:,} | {g['fused_minibatch_step_us']:.0f} | {g['torch_minibatch_step_us']:.0f} | "
                     f"{g['torch_over_fused_train']:.1f} | {nc(g['fused_launches_per_minibatch_step'])} | "
                     f"{nc(g['torch_launches_per_minibatch_step'])} |")
    lines += ["", "## The whole iteration", "",
              "| net | envs x steps / batch | rollout ms | train (b) ms | rollout's share (b) | train (a) ms | "
              "rollout's share (a) | iteration (b) / (a) |", "|---|---|---:|---:|---:|---:|---:|---:|"]
    for g in doc["rows"]:
        lines.append(f"| {tuple(g['net_arch'])} {g['activation']} | {g['num_envs']:,} x {g['n_steps']:,} / "
                     f"{g['batch_size']:,} | {g['rollout_ms']:.0f} | {g['torch_train_ms']:.0f} | "
                     f"{100 * g['torch_rollout_share']:.0f} % | {g['fused_train_ms']:.0f} | "
                     f"{100 * g['fused_rollout_share']:.0f} % | {g['torch_over_fused_iteration']:.2f} |")
    losers = [g for g in doc["rows"] if g["torch_over_fused_train"] <= 1.0]
    lines.append("")
    if losers:
        lines.append("Rule (DESIGN 19 - 22): the fused update is taken where (a) < (b). It LOST at: " + "; ".join(
            f"{tuple(g['net_arch'])} {g['activation']} batch {g['batch_size']}" for g in losers) +
            ". `ppo.learner.ARCH_UPDATE_KEEP_TORCH` must list those rows.")
    else:
        lines.append("Rule (DESIGN 19 - 22): the fused update is taken where (a) < (b). It won every row, so "
                     "`ppo.learner.ARCH_UPDATE_KEEP_TORCH` is empty.")
    lines += ["", "## The general kernels on the 128-128 ReLU net", "",
              "`FusedArchLearner.grads` against `FusedLearner.grads` (quad_ppo_grad's own kernels), eager calls, host "
              "launch cost included.", "", "| batch | general us | specialised us | general / specialised |",
              "|---:|---:|---:|---:|"]
    for g in doc["rows_128"]:
        lines.append(f"| {g['batch_size']:,} | {g['general_grads_us']:.1f} | {g['specialised_grads_us']:.1f} | "
                     f"{g['general_over_specialised']:.2f} |")
    return "\n".join(lines) + "\n"


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out-dir", default=OUT_DIR)
    a = ap.parse_args(argv)
    import torch
    rows = measure(a.reps)
    rows_128 = measure_128(a.reps)
    doc = {"workload": f"hover env with RateControlWrapper, 20 epochs per iteration, medians of {a.reps} runs after a "
                       f"warm-up, every run from the same parameters, Adam state and buffers",
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "rows": rows, "rows_128": rows_128,
           "fused_faster_everywhere": all(g["torch_over_fused_train"] > 1.0 for g in rows)}
    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, "bench.json"), "w") as f:
        json.dump(doc, f, indent=1)
    with open(os.path.join(a.out_dir, "README.md"), "w") as f:
        f.write(readme(doc))
    print(f"wrote {a.out_dir}/bench.json and README.md")
    return 0


if __name__ == "__main__":
    sys.exit(main())
