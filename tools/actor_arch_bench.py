"""Measure the general actor's one-launch episodes (ppo.fused.FusedActor, csrc/actor_arch.hip) against the
per-step loop they replace; writes profiles/actor_arch/bench.json.

Workload: hover env + RateControlWrapper, episodes of up to 512 steps from fresh resets, 1,024 and 65,536 envs,
for every arch (64,64) (96,64) (128,128) (256,256) (512,256) with ReLU and tanh. The policy is SB3's
orthogonal init (head gain 0.01) with the head bias at the hover thrust: untrained, it keeps an env flying for
about 130 steps on average (the mean length of each form is recorded).
Per case, after one warm-up run, `--reps` runs of each form on a host clock closed by a device synchronize. Every
run of every form starts from the same restored state (one reset, then set_state before each run, not timed), so
the forms fly the same episodes:

  (a) fused   FusedActor.episode: the whole batch of episodes in one launch
  (b) loop    the per-step loop evaluate_episodes ran for such a module before the general actor existed: torch
              forward + clamp + quad_step + the return / length bookkeeping, the host checking every 64 steps
              whether any env still runs
  (c) special for (128, 128, relu) only: FusedPolicy.episode, the kernel specialised to that net

Each (arch, activation) is measured in a child process of its own under a time limit; the first failure ends
the run (nothing is retried).

    python tools/actor_arch_bench.py [--reps 5] [--sizes 1024 65536] [--timeout 240]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

ARCHS = ((64, 64), (96, 64), (128, 128), (256, 256), (512, 256))
ACTIVATIONS = ("relu", "tanh")
WRAPPER = "RateControlWrapper"
STEPS = 512
OUT = os.path.join(REPO, "profiles", "actor_arch", "bench.json")


def _policy(h1, h2, activation):
    import torch
    from uav_reinforcement_learning_control_amd.ppo.policy import ActorCritic
    torch.manual_seed(0)
    pol = ActorCritic(12, 4, (h1, h2), activation=activation)
    with torch.no_grad():
        pol.action_net.bias.copy_(torch.tensor([0.2227 * 9.81 / 26.0 - 1.0, 0.0, 0.0, 0.0]))  # hover thrust
    return pol.cuda()


def _loop(policy, e, obs):
    """evaluate_episodes' per-step loop with the torch forward (its body before fused_actor_for)."""
    import torch
    n, device = e.num_envs, e.device
    out = torch.zeros(n, 4, device=device)
    ret = torch.zeros(n, dtype=torch.float64, device=device)
    length = torch.zeros(n, dtype=torch.int32, device=device)
    running = torch.ones(n, dtype=torch.bool, device=device)
    terminated = torch.zeros(n, dtype=torch.bool, device=device)
    with torch.no_grad():
        for t in range(e.max_episode_steps):
            mean, _ = policy.forward_heads(obs)
            torch.clamp(mean, -1.0, 1.0, out=out)
            _, rew, te, tr, _ = e.step(out, obs=obs, info="raw")
            ret += torch.where(running, rew.double(), 0.0)
            length += running.int()
            terminated |= running & te
            running &= ~(te | tr)
            if (t + 1) % 64 == 0 and not bool(running.any()):
                break
    return length


def measure(h1, h2, activation, sizes, reps):
    import torch
    from uav_reinforcement_learning_control_amd.envs import QuadVecEnv
    from uav_reinforcement_learning_control_amd.ppo.fused import FusedActor, FusedPolicy
    pol = _policy(h1, h2, activation)
    fa = FusedActor(pol)
    fa.pack()
    special = None
    if (h1, h2, activation) == (128, 128, "relu"):
        special = FusedPolicy(pol)
        special.pack()
    rows = []
    for n in sizes:
        e = QuadVecEnv(n, env="hover", wrapper=WRAPPER, device="cuda:0", seed=1, max_episode_steps=STEPS,
                       auto_reset=False)
        e.reset()
        start = e.get_state()
        forms = {"fused": lambda obs: fa.episode(e)["steps"], "loop": lambda obs: _loop(pol, e, obs)}
        if special is not None:
            forms["special"] = lambda obs: special.episode(e)["steps"]
        times = {k: [] for k in forms}
        mean_len = {}
        for rep in range(reps + 1):  # the first pass warms up
            for k, fn in forms.items():
                e.set_state(**start)
                obs = e.observe().clone()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                steps = fn(obs)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if rep > 0:
                    times[k].append(dt)
                mean_len[k] = float(steps.float().mean())
        e.close()
        row = {"h1": h1, "h2": h2, "activation": activation, "envs": n, "reps": reps}
        for k in forms:
            row[f"{k}_ms"] = 1e3 * statistics.median(times[k])
            row[f"{k}_ms_all"] = [1e3 * t for t in times[k]]
            row[f"{k}_mean_length"] = mean_len[k]
        row["loop_over_fused"] = row["loop_ms"] / row["fused_ms"]
        if special is not None:
            row["fused_over_special"] = row["fused_ms"] / row["special_ms"]
        rows.append(row)
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", nargs="+", type=int, default=[1024, 65536])
    ap.add_argument("--timeout", type=float, default=240.0, help="seconds per (arch, activation) child process")
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--case", nargs=3, default=None, metavar=("H1", "H2", "ACT"), help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    if a.case is not None:  # a child: one (arch, activation), the rows as one JSON line
        print("ROWS " + json.dumps(measure(int(a.case[0]), int(a.case[1]), a.case[2], a.sizes, a.reps)), flush=True)
        return 0
    rows = []
    for h1, h2 in ARCHS:
        for act in ACTIVATIONS:
            cmd = [sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--sizes", *map(str, a.sizes),
                   "--case", str(h1), str(h2), act]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
            line = next((l for l in r.stdout.splitlines() if l.startswith("ROWS ")), None)
            if r.returncode != 0 or line is None:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                raise SystemExit(f"{h1}x{h2} {act}: the measurement failed (exit {r.returncode}); stopping")
            got = json.loads(line[5:])
            rows += got
            for g in got:
                print(f"{h1}x{h2} {act} {g['envs']:6d} envs: fused {g['fused_ms']:8.2f} ms  loop {g['loop_ms']:8.2f} ms  "
                      f"x{g['loop_over_fused']:.1f}" + (f"  special {g['special_ms']:.2f} ms" if "special_ms" in g else ""),
                      flush=True)
    import torch
    doc = {"workload": f"hover + {WRAPPER}, up to {STEPS} steps per episode, medians of {a.reps} runs after a warm-up",
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "rows": rows,
           "fused_faster_everywhere": all(g["loop_over_fused"] > 1.0 for g in rows)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(f"wrote {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
