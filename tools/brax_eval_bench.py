"""Measure the Brax-profile policy's one-launch evaluation episodes (ppo.fused.FusedBraxActor, csrc/brax_actor.hip)
against the per-step loop they replace; writes profiles/brax_eval/bench.json and profiles/brax_eval/README.md.

Workload: both brax env kinds, episode limit 500, 128 and 65,536 envs, sampled actions (evaluation's default), for
the policies (128,128) relu (the project's training default), (256,256) silu and (512,256) tanh. The policy is
lecun-uniform with the output layer scaled by 0.1 (torque heads by a further 0.025), the thrust head's bias at the
hover thrust and the scale head's at -8, behind the nominal-state normaliser: untrained, it keeps most envs flying
for a hundred steps or more (the mean length of each form is recorded). The hover kind's reset state sits on the
floor, below its own z limit, so every episode from it ends at step 1: its envs are lifted to z = 1 before the
state is saved. Per case, after one warm-up run, `--reps` runs of each form on a host clock closed by a device
synchronize; every run of every form starts from the same restored state (set_state before each run, not timed):

  (a) launch  FusedBraxActor.episode: the whole batch of episodes in one launch
  (b) loop    torch forward on the normalised observation + NormalTanh sample + tanh + quad_step + the return /
              length bookkeeping, the host checking every 64 steps whether any env still runs -- what
              BraxPPO.evaluate and evaluate_brax run for a policy outside the MFMA family

Each (kind, policy) is measured in a child process of its own under a time limit; the first failure ends the run
(nothing is retried).

    python tools/brax_eval_bench.py [--reps 5] [--sizes 128 65536] [--timeout 300]
"""
from __future__ import annotations

import argparse
import json
import math
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
LIMIT = 500
OUT_DIR = os.path.join(REPO, "profiles", "brax_eval")


def _model(h1, h2, activation):
    import torch
    from uav_reinforcement_learning_control_amd.ppo.brax_ppo import BraxActorCritic, BraxPPOConfig
    torch.manual_seed(0)
    net = BraxActorCritic(21, 4, BraxPPOConfig(policy_hidden_sizes=(h1, h2), activation=activation))
    with torch.no_grad():
        k, b = net.policy.kernels[2], net.policy.biases[2]
        k.mul_(0.1)
        k[:, 1:4].mul_(0.025)
        b.copy_(torch.tensor([math.atanh(2.0 * 0.2227 * 9.81 / 52.0 - 1.0), 0, 0, 0, -8.0, -8.0, -8.0, -8.0]))
    mean = torch.tensor([0, 0, 1, 1, 0, 0, 0] + [0.0] * 14)
    std = torch.tensor([0.02] * 7 + [100.0] * 4 + [0.05] * 6 + [100.0] * 4)
    return net.cuda(), dict(mean=mean.cuda(), std=std.cuda())


def _loop(net, norm, e, obs, gen):
    import torch
    n, device = e.num_envs, e.device
    ret = torch.zeros(n, dtype=torch.float64, device=device)
    length = torch.zeros(n, dtype=torch.int32, device=device)
    running = torch.ones(n, dtype=torch.bool, device=device)
    with torch.no_grad():
        for t in range(e.max_episode_steps):
            logits = net.policy((obs - norm["mean"]) / norm["std"])
            act = torch.tanh(net.dist.sample_raw(logits, gen)).contiguous()
            _, rew, te, tr, _ = e.step(act, obs=obs, info="raw")
            ret += torch.where(running, rew.double(), 0.0)
            length += running.int()
            running &= ~(te | tr)
            if (t + 1) % 64 == 0 and not bool(running.any()):
                break
    return length


def measure(kind, h1, h2, activation, sizes, reps):
    import torch
    from uav_reinforcement_learning_control_amd.envs import QuadVecEnv
    from uav_reinforcement_learning_control_amd.ppo.fused import FusedBraxActor
    net, norm = _model(h1, h2, activation)
    fa = FusedBraxActor(net, norm)
    fa.pack()
    gen = torch.Generator(device="cuda")
    rows = []
    for n in sizes:
        e = QuadVecEnv(n, env=kind, device="cuda:0", seed=1, max_episode_steps=LIMIT, auto_reset=False)
        e.reset()
        start = e.get_state()
        if kind == "brax_hover":
            start["qpos"][:, 2] += 1.0
        forms = {"launch": lambda obs: fa.episode(e, deterministic=False, seed=3)["steps"],
                 "loop": lambda obs: _loop(net, norm, e, obs, gen)}
        times = {k: [] for k in forms}
        mean_len = {}
        for rep in range(reps + 1):  # the first pass warms up
            for k, fn in forms.items():
                e.set_state(**start)
                obs = e.observe().clone()
                gen.manual_seed(3)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                steps = fn(obs)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if rep > 0:
                    times[k].append(dt)
                mean_len[k] = float(steps.float().mean())
        e.close()
        row = {"kind": kind, "h1": h1, "h2": h2, "activation": activation, "envs": n, "reps": reps}
        for k in forms:
            row[f"{k}_ms"] = 1e3 * statistics.median(times[k])
            row[f"{k}_ms_all"] = [1e3 * t for t in times[k]]
            row[f"{k}_mean_length"] = mean_len[k]
        row["loop_over_launch"] = row["loop_ms"] / row["launch_ms"]
        rows.append(row)
    return rows


def readme(doc) -> str:
    lines = ["# Brax-profile evaluation: one launch against the per-step loop", "",
             "Written by `tools/brax_eval_bench.py`; the numbers are `bench.json`'s.", "",
             f"Device: {doc['device']}; torch {doc['torch']}. {doc['workload']}.", "",
             "(a) launch: `FusedBraxActor.episode` (quad_brax_episode). (b) loop: torch forward + NormalTanh sample + "
             "`quad_step` per step in the same process. There is no Brax evaluation in the parent commit to compare "
             "with, so (b) is the yardstick.", "",
             "| kind | policy | envs | (a) launch ms | (b) loop ms | (b) / (a) | mean length (a) / (b) |",
             "|---|---|---:|---:|---:|---:|---|"]
    for g in doc["rows"]:
        lines.append(f"| {g['kind']} | ({g['h1']},{g['h2']}) {g['activation']} | {g['envs']:,} | {g['launch_ms']:.2f} | "
                     f"{g['loop_ms']:.2f} | {g['loop_over_launch']:.1f} | {g['launch_mean_length']:.1f} / "
                     f"{g['loop_mean_length']:.1f} |")
    lines += ["", "The two forms draw their action noise from different generators (the launch's Philox stream, torch's "
              "generator), so their episodes differ in detail and the mean lengths are recorded per form.", ""]
    losers = [g for g in doc["rows"] if g["loop_over_launch"] <= 1.0]
    if losers:
        lines.append("Rule (DESIGN 20): the drivers take the launch where (a) < (b). The launch LOST for: " + "; ".join(
            f"{g['kind']} ({g['h1']},{g['h2']}) {g['activation']} at {g['envs']:,} envs" for g in losers) +
            ". `ppo.fused.BRAX_KEEP_LOOP` must list those policies, so the dispatch keeps the loop for them.")
    else:
        lines.append("Rule (DESIGN 20): the drivers take the launch where (a) < (b). The launch won every row, so "
                     "`ppo.fused.BRAX_KEEP_LOOP` is empty and every policy of the family flies in one launch.")
    return "\n".join(lines) + "\n"


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", nargs="+", type=int, default=[128, 65536])
    ap.add_argument("--timeout", type=float, default=300.0, help="seconds per (kind, policy) child process")
    ap.add_argument("--out-dir", default=OUT_DIR)
    ap.add_argument("--case", nargs=4, default=None, metavar=("KIND", "H1", "H2", "ACT"), help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    if a.case is not None:  # a child: one (kind, policy), the rows as one JSON line
        print("ROWS " + json.dumps(measure(a.case[0], int(a.case[1]), int(a.case[2]), a.case[3], a.sizes, a.reps)),
              flush=True)
        return 0
    rows = []
    for kind in KINDS:
        for h1, h2, act in POLICIES:
            cmd = [sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--sizes", *map(str, a.sizes),
                   "--case", kind, str(h1), str(h2), act]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
            line = next((l for l in r.stdout.splitlines() if l.startswith("ROWS ")), None)
            if r.returncode != 0 or line is None:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                raise SystemExit(f"{kind} {h1}x{h2} {act}: the measurement failed (exit {r.returncode}); stopping")
            got = json.loads(line[5:])
            rows += got
            for g in got:
                print(f"{kind} {h1}x{h2} {act} {g['envs']:6d} envs: launch {g['launch_ms']:8.2f} ms  loop "
                      f"{g['loop_ms']:8.2f} ms  x{g['loop_over_launch']:.1f}  lengths {g['launch_mean_length']:.1f} / "
                      f"{g['loop_mean_length']:.1f}", flush=True)
    import torch
    doc = {"workload": f"both brax kinds, episode limit {LIMIT}, sampled actions, medians of {a.reps} runs after a "
                       "warm-up, every run from the same restored state",
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "rows": rows,
           "launch_faster_everywhere": all(g["loop_over_launch"] > 1.0 for g in rows)}
    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, "bench.json"), "w") as f:
        json.dump(doc, f, indent=1)
    with open(os.path.join(a.out_dir, "README.md"), "w") as f:
        f.write(readme(doc))
    print(f"wrote {a.out_dir}/bench.json and README.md")
    return 0


if __name__ == "__main__":
    sys.exit(main())
