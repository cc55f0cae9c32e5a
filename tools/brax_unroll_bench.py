"""Measure the Brax learner's one-launch unrolls (ppo.fused.FusedBraxActor.unroll, csrc/brax_unroll.hip) against the
torch per-step loop they replace (BraxPPO._unrolls with fused_unroll=False), and the split of a training step between
the unrolls and the update; writes profiles/brax_unroll/bench.json and profiles/brax_unroll/README.md.

Workload: both brax env kinds at the reference defaults (1,024 envs, 16 unrolls of 10 steps, 500-step episodes) and at
the recommended command's shape (2,048 envs, 8 unrolls of 10 steps, 1,000-step episodes, 10 s trajectories), batch
size 1,024, 16 minibatches, 4 updates per batch, for the policies (128,128) relu (the training default), (256,256)
silu and (512,256) tanh with BraxPPO's own initialisation; the value net is the default (128,128). The hover kind is
measured as the learner sees it: its reset state sits on the floor, so its episodes end at once and every step of
every env takes the auto-reset branch. Per case, after one warm-up run, `--reps` runs of each form on a host clock
closed by a device synchronize; every run of every form starts from the same restored env state, parameters,
optimizer state and running statistics (restored before each run, not timed):

  (a) launch   BraxPPO(fused_unroll=True)._unrolls(): pack + one quad_brax_unroll launch
  (b) loop     BraxPPO(fused_unroll=False)._unrolls(): the torch per-step loop
  step (a), step (b)   training_step() of the two models: the unrolls, the statistics update, the minibatch updates

The update's share of a step is (step - unrolls) / step, per form. Each (kind, policy) is measured in a child process
of its own under a time limit; the first failure ends the run (nothing is retried).

    python tools/brax_unroll_bench.py [--reps 5] [--timeout 300]
    python tools/brax_unroll_bench.py --readme-only     # after the recommended command's logs were put in the folder
"""
from __future__ import annotations

import argparse
import copy
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

KINDS = ("brax_hover", "brax_jax_mjx")
POLICIES = ((128, 128, "relu"), (256, 256, "silu"), (512, 256, "tanh"))
SHAPES = ((1024, 500, 5.0), (2048, 1000, 10.0))  # envs, episode length, trajectory seconds
OUT_DIR = os.path.join(REPO, "profiles", "brax_unroll")


def _model(kind, n, limit, dur, h1, h2, activation, fused):
    from uav_reinforcement_learning_control_amd.envs import QuadVecEnv
    from uav_reinforcement_learning_control_amd.ppo.brax_ppo import BraxPPO, BraxPPOConfig
    cfg = BraxPPOConfig(num_envs=n, episode_length=limit, policy_hidden_sizes=(h1, h2), activation=activation,
                        fused_unroll=fused)
    env = QuadVecEnv(n, env=kind, device="cuda:0", seed=1, max_episode_steps=limit,
                     cfg_overrides={"traj_duration": dur})
    return BraxPPO(env, cfg, seed=1), env


class _Saved:
    """Everything a run changes, restored before the next one."""

    def __init__(self, model, env):
        self.model, self.env = model, env
        env.reset()
        self.state = env.get_state()
        self.net = copy.deepcopy(model.net.state_dict())
        self.opt = copy.deepcopy(model.opt.state_dict())
        self.norm = {k: getattr(model.norm, k).clone() for k in ("count", "mean", "summed_variance", "std")}

    def restore(self):
        m = self.model
        self.env.set_state(**self.state)
        m.net.load_state_dict(self.net)
        m.opt.load_state_dict(copy.deepcopy(self.opt))
        for k, v in self.norm.items():
            setattr(m.norm, k, v.clone())
        m._obs = self.env.observe().clone()
        m._ep_ret.zero_()
        m._noise_t = 0
        m.gen.manual_seed(1)


def measure(kind, h1, h2, activation, reps):
    import torch
    rows = []
    for n, limit, dur in SHAPES:
        forms = {}
        for name, fused in (("launch", True), ("loop", False)):
            model, env = _model(kind, n, limit, dur, h1, h2, activation, fused)
            forms[name] = (model, env, _Saved(model, env))
        times = {f"{k}_{w}": [] for k in forms for w in ("unrolls", "step")}
        episodes = {}
        for rep in range(reps + 1):  # the first pass warms up
            for name, (model, env, saved) in forms.items():
                for what, fn in (("unrolls", model._unrolls), ("step", model.training_step)):
                    saved.restore()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = fn()
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                    if rep > 0:
                        times[f"{name}_{what}"].append(dt)
                    if what == "unrolls":
                        episodes[name] = int(out[7].item())
        for _, env, _ in forms.values():
            env.close()
        model = forms["launch"][0]
        row = {"kind": kind, "h1": h1, "h2": h2, "activation": activation, "envs": n, "episode_length": limit,
               "num_unrolls": model.num_unrolls, "unroll_length": model.cfg.unroll_length, "reps": reps,
               "env_steps": model.num_unrolls * model.cfg.unroll_length * n}
        for k, v in times.items():
            row[f"{k}_ms"] = 1e3 * statistics.median(v)
            row[f"{k}_ms_all"] = [1e3 * t for t in v]
        for name in forms:
            row[f"{name}_episodes"] = episodes[name]
            row[f"{name}_unroll_share"] = row[f"{name}_unrolls_ms"] / row[f"{name}_step_ms"]
            row[f"{name}_update_ms"] = row[f"{name}_step_ms"] - row[f"{name}_unrolls_ms"]
            row[f"{name}_step_sps"] = row["env_steps"] / (1e-3 * row[f"{name}_step_ms"])
        row["loop_over_launch"] = row["loop_unrolls_ms"] / row["launch_unrolls_ms"]
        row["step_loop_over_launch"] = row["loop_step_ms"] / row["launch_step_ms"]
        rows.append(row)
    return rows


def readme(doc) -> str:
    lines = ["# The Brax learner's unrolls: one launch against the torch per-step loop", "",
             "Written by `tools/brax_unroll_bench.py`; the numbers are `bench.json`'s.", "",
             f"Device: {doc['device']}; torch {doc['torch']}. {doc['workload']}.", "",
             "(a) launch: `BraxPPO(fused_unroll=True)._unrolls()` (pack + one `quad_brax_unroll`). (b) loop: the torch "
             "`_unrolls` body, the parent commit's code, in the same process.", "",
             "| kind | policy | envs x U x L | (a) launch ms | (b) loop ms | (b) / (a) |",
             "|---|---|---|---:|---:|---:|"]
    for g in doc["rows"]:
        lines.append(f"| {g['kind']} | ({g['h1']},{g['h2']}) {g['activation']} | {g['envs']:,} x {g['num_unrolls']} x "
                     f"{g['unroll_length']} | {g['launch_unrolls_ms']:.2f} | {g['loop_unrolls_ms']:.1f} | "
                     f"{g['loop_over_launch']:.1f} |")
    lines += ["", "## The phase split of `training_step`", "",
              "Whole training steps (unrolls + statistics + 64 autograd minibatch updates) of the two models; the "
              "update is step - unrolls.", "",
              "| kind | policy | envs | step (b) ms | unrolls' share (b) | step (a) ms | unrolls' share (a) | update ms "
              "(b) / (a) | step (b) / (a) | env-steps/s (b) / (a) |",
              "|---|---|---:|---:|---:|---:|---:|---|---:|---|"]
    for g in doc["rows"]:
        lines.append(f"| {g['kind']} | ({g['h1']},{g['h2']}) {g['activation']} | {g['envs']:,} | {g['loop_step_ms']:.1f} | "
                     f"{100 * g['loop_unroll_share']:.0f} % | {g['launch_step_ms']:.1f} | "
                     f"{100 * g['launch_unroll_share']:.1f} % | {g['loop_update_ms']:.1f} / {g['launch_update_ms']:.1f} | "
                     f"{g['step_loop_over_launch']:.2f} | {g['loop_step_sps']:.3g} / {g['launch_step_sps']:.3g} |")
    lines.append("")
    losers = [g for g in doc["rows"] if g["loop_over_launch"] <= 1.0]
    if losers:
        lines.append("Rule (DESIGN 19 / 20): the launch is taken where (a) < (b). The launch LOST for: " + "; ".join(
            f"{g['kind']} ({g['h1']},{g['h2']}) {g['activation']} at {g['envs']:,} envs" for g in losers) +
            ". `ppo.fused.BRAX_UNROLL_KEEP_LOOP` must list those policies.")
    else:
        lines.append("Rule (DESIGN 19 / 20): the launch is taken where (a) < (b). It won every row, so "
                     "`ppo.fused.BRAX_UNROLL_KEEP_LOOP` is empty.")
    return "\n".join(lines + runs_section(doc.get("out_dir", OUT_DIR))) + "\n"


def runs_section(out_dir) -> list:
    """The recommended command's runs, if their logs lie in out_dir as train_<loop|fused>_s<seed>.log (train_brax's
    stdout) beside train_<..>_summary.json: wall time, the rate's range after the first step, final and best
    train_reward per seed."""
    import glob
    import re
    logs = sorted(glob.glob(os.path.join(out_dir, "train_*_s*.log")))
    if not logs:
        return []
    lines = ["", "## The recommended command, whole runs", "",
             "`train_brax --env jax_mjx_quad --num-timesteps 10000000 --episode-length 1000 --num-envs 2048 "
             "--traj-duration-seconds 10.0 --checkpoint-interval 0 --seed S [--fused-unroll]`, same box, one after the "
             "other (logs and summaries in this folder; paths in them are relative to the runs' output directory).", "",
             "| form | seed | wall s | env-steps/s after the first step | final train_reward | best train_reward |",
             "|---|---:|---:|---|---:|---:|"]
    finals = {"loop": [], "fused": []}
    for path in logs:
        form, seed = re.match(r"train_(\w+)_s(\d+)\.log", os.path.basename(path)).groups()
        pts = [(float(m.group(1)), float(m.group(2))) for m in
               re.finditer(r"train_reward=([-0-9.eE+naif]+) sps=([0-9.]+)", open(path).read())]
        rew = [r for r, _ in pts if r == r]
        sps = [s for _, s in pts[1:]]
        summ = json.load(open(path[:-4] + "_summary.json"))
        finals[form].append(rew[-1])
        lines.append(f"| {form} | {seed} | {summ['elapsed_sec']:.1f} | {min(sps) / 1e6:.2f}M - {max(sps) / 1e6:.2f}M | "
                     f"{rew[-1]:.1f} | {max(rew):.1f} |")
    if all(finals.values()):
        lo, fu = finals["loop"], finals["fused"]
        overlap = max(min(lo), min(fu)) <= min(max(lo), max(fu))
        lines += ["", f"Final returns: loop {min(lo):.1f} - {max(lo):.1f}, fused {min(fu):.1f} - {max(fu):.1f}: the ranges "
                  + ("overlap." if overlap else "do NOT overlap.")]
    return lines


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--timeout", type=float, default=300.0, help="seconds per (kind, policy) child process")
    ap.add_argument("--out-dir", default=OUT_DIR)
    ap.add_argument("--case", nargs=4, default=None, metavar=("KIND", "H1", "H2", "ACT"), help=argparse.SUPPRESS)
    ap.add_argument("--readme-only", action="store_true",
                    help="rewrite README.md from the bench.json and the training logs already in --out-dir")
    a = ap.parse_args(argv)
    if a.readme_only:
        doc = json.load(open(os.path.join(a.out_dir, "bench.json")))
        with open(os.path.join(a.out_dir, "README.md"), "w") as f:
            f.write(readme(dict(doc, out_dir=a.out_dir)))
        return 0
    if a.case is not None:  # a child: one (kind, policy), the rows as one JSON line
        print("ROWS " + json.dumps(measure(a.case[0], int(a.case[1]), int(a.case[2]), a.case[3], a.reps)), flush=True)
        return 0
    rows = []
    for kind in KINDS:
        for h1, h2, act in POLICIES:
            cmd = [sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--case", kind, str(h1), str(h2),
                   act]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
            line = next((l for l in r.stdout.splitlines() if l.startswith("ROWS ")), None)
            if r.returncode != 0 or line is None:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                raise SystemExit(f"{kind} {h1}x{h2} {act}: the measurement failed (exit {r.returncode}); stopping")
            got = json.loads(line[5:])
            rows += got
            for g in got:
                print(f"{kind} {h1}x{h2} {act} {g['envs']:5d} envs: unrolls launch {g['launch_unrolls_ms']:7.2f} ms  loop "
                      f"{g['loop_unrolls_ms']:7.1f} ms  x{g['loop_over_launch']:.1f} | step launch "
                      f"{g['launch_step_ms']:7.1f} ms  loop {g['loop_step_ms']:7.1f} ms  unrolls' share of the loop's "
                      f"step {100 * g['loop_unroll_share']:.0f} %", flush=True)
    import torch
    doc = {"workload": f"both brax kinds, BraxPPO defaults at 1,024 envs and the recommended command's 2,048, medians of "
                       f"{a.reps} runs after a warm-up, every run from the same restored state",
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "rows": rows,
           "launch_faster_everywhere": all(g["loop_over_launch"] > 1.0 for g in rows)}
    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, "bench.json"), "w") as f:
        json.dump(doc, f, indent=1)
    with open(os.path.join(a.out_dir, "README.md"), "w") as f:
        f.write(readme(dict(doc, out_dir=a.out_dir)))
    print(f"wrote {a.out_dir}/bench.json and README.md")
    return 0


if __name__ == "__main__":
    sys.exit(main())
