"""Measure the general fused Brax update (BraxPPOConfig.fused_update_arch: ppo.fused.FusedBraxArchLearner,
quad_brax_ppo_arch_grad + quad_clip_adam per minibatch step) against the torch autograd update it replaces (the flag
off: the parent commit's path, the yardstick); writes profiles/brax_arch_update/bench.json and README.md.

tools/brax_update_bench.py's method, over architectures: the brax trajectory kind, batch size 1,024, 16 minibatches, 4
updates per batch (64 minibatch steps per training step), at the recommended command's shape (2,048 envs x 8 unrolls x
10 steps) and at the reference defaults (1,024 x 16 x 10), with (64, 64) tanh, (256, 256) SiLU and (512, 256) tanh
policy and value nets. Both forms collect their unrolls in one launch. One process; after one warm-up pass, `--reps`
runs of each form on a host clock closed by a device synchronize; every run starts from the same restored env state,
parameters, optimizer state and running statistics. Launches per minibatch step come from torch's profiler; (a) is
seven by construction (k_brax_arch_value, k_brax_gae, k_brax_arch_fwd, k_brax_arch_wgrad, k_brax_arch_reduce,
k_grad_sumsq, k_adam) plus the torch kernels that slice the permutation and accumulate the logged losses.

    python tools/brax_arch_update_bench.py [--reps 5]
    python tools/brax_arch_update_bench.py --readme-only     # after the recommended command's logs were put in the folder
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
sys.path.insert(0, os.path.join(REPO, "tools"))

KIND = "brax_jax_mjx"
SHAPES = ((2048, 1000, 10.0), (1024, 500, 5.0))  # envs, episode length, trajectory seconds
ARCHS = (((64, 64), "tanh"), ((256, 256), "silu"), ((512, 256), "tanh"))  # policy = value sizes, activation
OUT_DIR = os.path.join(REPO, "profiles", "brax_arch_update")
FUSED_LAUNCHES = 7


def _model(n, limit, dur, sizes, act, fused):
    from uav_reinforcement_learning_control_amd.envs import QuadVecEnv
    from uav_reinforcement_learning_control_amd.ppo.brax_ppo import BraxPPO, BraxPPOConfig
    cfg = BraxPPOConfig(num_envs=n, episode_length=limit, fused_unroll=True, fused_update_arch=fused,
                        policy_hidden_sizes=sizes, value_hidden_sizes=sizes, activation=act)
    env = QuadVecEnv(n, env=KIND, device="cuda:0", seed=1, max_episode_steps=limit, cfg_overrides={"traj_duration": dur})
    return BraxPPO(env, cfg, seed=1), env


def measure(reps, out_dir):
    import torch
    from brax_unroll_bench import _Saved
    from brax_update_bench import _launches
    rows = []
    for sizes, act in ARCHS:
        for n, limit, dur in SHAPES:
            forms = {}
            for name, fused in (("fused", True), ("torch", False)):
                model, env = _model(n, limit, dur, sizes, act, fused)
                forms[name] = (model, env, _Saved(model, env))
            times = {f"{k}_{w}": [] for k in forms for w in ("unrolls", "step")}
            for rep in range(reps + 1):  # the first pass warms up
                for name, (model, env, saved) in forms.items():
                    for what, fn in (("unrolls", model._unrolls), ("step", model.training_step)):
                        saved.restore()
                        model._update_t = 0
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        fn()
                        torch.cuda.synchronize()
                        if rep > 0:
                            times[f"{name}_{what}"].append(time.perf_counter() - t0)
            model = forms["torch"][0]
            c = model.cfg
            mbs = c.num_updates_per_batch * c.num_minibatches
            launches = {name: _launches(m, sv) for name, (m, _, sv) in forms.items()}
            for _, env, _ in forms.values():
                env.close()
            row = {"kind": KIND, "policy_hidden_sizes": list(sizes), "value_hidden_sizes": list(sizes),
                   "activation": act, "envs": n, "num_minibatches": c.num_minibatches, "num_unrolls": model.num_unrolls,
                   "unroll_length": c.unroll_length, "episode_length": limit, "minibatch_steps": mbs,
                   "minibatch_trajectories": model.num_unrolls * n // c.num_minibatches, "reps": reps,
                   "env_steps": model.num_unrolls * c.unroll_length * n,
                   "fused_launches_by_construction": FUSED_LAUNCHES}
            for name, k in launches.items():
                row[f"{name}_launches_per_training_step"] = k
                row[f"{name}_launches_per_minibatch_step"] = None if k is None else k / mbs
            for k, v in times.items():
                row[f"{k}_ms"] = 1e3 * statistics.median(v)
                row[f"{k}_ms_all"] = [1e3 * t for t in v]
            for name in forms:
                row[f"{name}_update_ms"] = row[f"{name}_step_ms"] - row[f"{name}_unrolls_ms"]
                row[f"{name}_minibatch_step_ms"] = row[f"{name}_update_ms"] / mbs
                row[f"{name}_update_share"] = row[f"{name}_update_ms"] / row[f"{name}_step_ms"]
            row["torch_over_fused_update"] = row["torch_update_ms"] / row["fused_update_ms"]
            row["torch_over_fused_step"] = row["torch_step_ms"] / row["fused_step_ms"]
            row["keep_torch_key"] = [n, c.num_minibatches, c.unroll_length, [list(sizes), list(sizes), act]]
            rows.append(row)
            print(f"{sizes} {act} {n:5d} envs x {row['num_unrolls']} x {c.unroll_length}: minibatch step fused "
                  f"{row['fused_minibatch_step_ms']:.3f} ms  torch {row['torch_minibatch_step_ms']:.3f} ms  "
                  f"x{row['torch_over_fused_update']:.1f} | step fused {row['fused_step_ms']:.1f} ms  torch "
                  f"{row['torch_step_ms']:.1f} ms", flush=True)
            with open(os.path.join(out_dir, "bench_rows_partial.json"), "w") as f:
                json.dump(rows, f, indent=1)
    return rows


def readme(doc) -> str:
    arch = lambda g: f"({g['policy_hidden_sizes'][0]}, {g['policy_hidden_sizes'][1]}) {g['activation']}"
    lines = ["# The Brax learner's update for the whole net family: fused launches against torch autograd", "",
             "Written by `tools/brax_arch_update_bench.py`; the numbers are `bench.json`'s.", "",
             f"Device: {doc['device']}; torch {doc['torch']}. {doc['workload']}.", "",
             "(a) fused: `BraxPPO(fused_update_arch=True)`: per minibatch step `quad_brax_ppo_arch_grad` (five launches) "
             "and `quad_clip_adam` (two). (b) torch: the flag off, the parent commit's autograd update, in the same "
             "process. Both collect their unrolls in one launch.", "",
             "| nets | envs x U x L | minibatch step (a) ms | (b) ms | (b) / (a) | launches per minibatch step (a) | (b) |",
             "|---|---|---:|---:|---:|---:|---:|"]
    for g in doc["rows"]:
        tl, fl = g["torch_launches_per_minibatch_step"], g["fused_launches_per_minibatch_step"]
        lines.append(f"| {arch(g)} | {g['envs']:,} x {g['num_unrolls']} x {g['unroll_length']} | "
                     f"{g['fused_minibatch_step_ms']:.3f} | {g['torch_minibatch_step_ms']:.3f} | "
                     f"{g['torch_over_fused_update']:.1f} | {'not counted' if fl is None else f'{fl:.1f}'} | "
                     f"{'not counted' if tl is None else f'{tl:.0f}'} |")
    lines += ["", "## The phase split of `training_step`", "",
              "| nets | envs | unrolls ms | step (b) ms | update's share (b) | step (a) ms | update's share (a) | "
              "step (b) / (a) |", "|---|---:|---:|---:|---:|---:|---:|---:|"]
    for g in doc["rows"]:
        lines.append(f"| {arch(g)} | {g['envs']:,} | {g['fused_unrolls_ms']:.2f} | {g['torch_step_ms']:.1f} | "
                     f"{100 * g['torch_update_share']:.0f} % | {g['fused_step_ms']:.1f} | "
                     f"{100 * g['fused_update_share']:.0f} % | {g['torch_over_fused_step']:.2f} |")
    losers = [g for g in doc["rows"] if g["torch_over_fused_update"] <= 1.0]
    lines.append("")
    if losers:
        lines.append("Rule (DESIGN 19 - 22): the fused update is taken where (a) < (b). It LOST at: " + "; ".join(
            f"{arch(g)} at {g['envs']:,} envs" for g in losers) +
            ". `ppo.fused.BRAX_ARCH_UPDATE_KEEP_TORCH` must list those rows' `keep_torch_key`.")
    else:
        lines.append("Rule (DESIGN 19 - 22): the fused update is taken where (a) < (b). It won every row, so "
                     "`ppo.fused.BRAX_ARCH_UPDATE_KEEP_TORCH` is empty.")
    return "\n".join(lines + runs_section(doc.get("out_dir", OUT_DIR))) + "\n"


def runs_section(out_dir) -> list:
    """The recommended command's runs with (256, 256) SiLU nets, if their logs lie in out_dir as
    train_<torch|fused>_s<seed>.log (train_brax's stdout) beside train_<..>_summary.json: wall time, final and best
    train_reward per seed."""
    import glob
    import re
    logs = sorted(glob.glob(os.path.join(out_dir, "train_*_s*.log")))
    if not logs:
        return []
    lines = ["", "## The recommended command with (256, 256) SiLU nets, whole runs", "",
             "`train_brax --env jax_mjx_quad --num-timesteps 10000000 --episode-length 1000 --num-envs 2048 "
             "--traj-duration-seconds 10.0 --checkpoint-interval 0 --activation silu --policy-hidden-sizes 256,256 "
             "--value-hidden-sizes 256,256 --seed S --fused-unroll [--fused-arch-update]`, same box, one after the other "
             "(`torch`: --fused-unroll alone; `fused`: with --fused-arch-update; logs and summaries in this folder, paths "
             "in them relative to the runs' output directory).", "",
             "| form | seed | wall s | final train_reward | best train_reward |", "|---|---:|---:|---:|---:|"]
    finals = {}
    for path in logs:
        form, seed = re.match(r"train_(\w+)_s(\d+)\.log", os.path.basename(path)).groups()
        rew = [float(m.group(1)) for m in re.finditer(r"train_reward=([-0-9.eE+naif]+) sps=", open(path).read())]
        rew = [r for r in rew if r == r]
        summ = json.load(open(path[:-4] + "_summary.json"))
        finals.setdefault(form, []).append(rew[-1])
        lines.append(f"| {form} | {seed} | {summ['elapsed_sec']:.1f} | {rew[-1]:.1f} | {max(rew):.1f} |")
    if len(finals) == 2:
        (fa, a), (fb, b) = sorted(finals.items())
        overlap = max(min(a), min(b)) <= min(max(a), max(b))
        lines += ["", f"Final returns: {fa} {min(a):.1f} - {max(a):.1f}, {fb} {min(b):.1f} - {max(b):.1f}: the ranges "
                  + ("overlap." if overlap else "do NOT overlap.")]
    return lines


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out-dir", default=OUT_DIR)
    ap.add_argument("--readme-only", action="store_true",
                    help="rewrite README.md from the bench.json and the training logs already in --out-dir")
    a = ap.parse_args(argv)
    if a.readme_only:
        doc = json.load(open(os.path.join(a.out_dir, "bench.json")))
        with open(os.path.join(a.out_dir, "README.md"), "w") as f:
            f.write(readme(dict(doc, out_dir=a.out_dir)))
        return 0
    import torch
    os.makedirs(a.out_dir, exist_ok=True)
    rows = measure(a.reps, a.out_dir)  # bench_rows_partial.json holds the finished rows meanwhile
    os.remove(os.path.join(a.out_dir, "bench_rows_partial.json"))
    doc = {"workload": f"{KIND}, policy = value nets, 64 minibatch steps per training step, medians of {a.reps} runs "
                       f"after a warm-up, every run from the same restored state",
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "rows": rows,
           "fused_faster_everywhere": all(g["torch_over_fused_update"] > 1.0 for g in rows)}
    with open(os.path.join(a.out_dir, "bench.json"), "w") as f:
        json.dump(doc, f, indent=1)
    with open(os.path.join(a.out_dir, "README.md"), "w") as f:
        f.write(readme(dict(doc, out_dir=a.out_dir)))
    print(f"wrote {a.out_dir}/bench.json and README.md")
    return 0


if __name__ == "__main__":
    sys.exit(main())
