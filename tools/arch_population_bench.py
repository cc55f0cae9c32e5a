"""Measure ppo.ArchPopulationPPO against the stand-alone PPO with both arch flags; writes
profiles/arch_population/bench.json and README.md.

Workload: trial 31's hyperparameters (tests/golden/hpo_trial31.json) at 8 envs per member, hover +
RateControlWrapper: one full iteration -- a rollout of 1,024 steps, then 20 epochs x 64 minibatches of 128 rows -- after
a warm-up iteration, for the nets (64, 64) tanh, (256, 256) tanh and (512, 256) relu. For P in --sizes an
ArchPopulationPPO of P members (seeds 0..P-1) is timed, alternating in the same process with the stand-alone PPO
iteration (fused_rollout_arch + fused_update_arch: the path a seed sweep of such a net took before); rollout and update
are timed separately on a host clock closed by a device synchronize, medians of --reps.

The bar is DESIGN 18's: a 64-member iteration must take less than half of 64 stand-alone iterations. A net that misses
it is reported as such (and belongs in ppo.population.ARCH_POPULATION_KEEP_SERIAL).

    python tools/arch_population_bench.py --sizes 1 16 64 256 --reps 3 [--optimize 256]

--optimize N also times a full `optimize --search-arch --n-trials N` study at its defaults.
"""
from __future__ import annotations

import argparse
import dataclasses
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

WRAPPER = "RateControlWrapper"
NETS = (((64, 64), "tanh"), ((256, 256), "tanh"), ((512, 256), "relu"))


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def bench_net(hidden, activation, sizes, reps):
    from hpo_repro import ppo_config
    from uav_reinforcement_learning_control_amd.envs import QuadVecEnv
    from uav_reinforcement_learning_control_amd.ppo import PPO, ArchPopulationPPO
    cfg = dataclasses.replace(ppo_config(), net_arch=tuple(hidden), activation=activation, fused_rollout_arch=True,
                              fused_update_arch=True)
    solo = PPO(QuadVecEnv(8, env="hover", wrapper=WRAPPER, device="cuda:0", seed=0), cfg, seed=0)
    solo.collect_rollouts(); solo.train()  # warm-up iteration (captures the epoch graph)
    out = []
    for P in sizes:
        pop = ArchPopulationPPO([(cfg, s) for s in range(P)], n_envs=8, env="hover", wrapper=WRAPPER, device="cuda:0")
        pop.collect_rollouts(); pop.train()  # warm-up iteration
        rows = {"pop_rollout": [], "pop_update": [], "solo_rollout": [], "solo_update": []}
        for _ in range(reps):
            rows["pop_rollout"].append(_timed(pop.collect_rollouts))
            rows["pop_update"].append(_timed(pop.train))
            rows["solo_rollout"].append(_timed(solo.collect_rollouts))
            rows["solo_update"].append(_timed(solo.train))
        med = {k: statistics.median(v) for k, v in rows.items()}
        pop_it, solo_it = med["pop_rollout"] + med["pop_update"], med["solo_rollout"] + med["solo_update"]
        r = {"net_arch": list(hidden), "activation": activation, "members": P, "reps": reps, "seconds": rows,
             "median_seconds": med, "population_iteration_s": pop_it, "standalone_iteration_s": solo_it,
             "speedup_vs_serial": P * solo_it / pop_it, "env_steps_per_s": P * 8 * 1024 / pop_it}
        print(json.dumps({k: v for k, v in r.items() if k != "seconds"}), flush=True)
        out.append(r)
        pop.close()
        del pop
        torch.cuda.empty_cache()
    return out


def optimize_run(n_trials):
    """A full `optimize --search-arch --n-trials N` study at its defaults, timed."""
    import tempfile
    from uav_reinforcement_learning_control_amd import optimize as O
    with tempfile.TemporaryDirectory() as d:
        a = O.build_parser().parse_args(["--search-arch", "--n-trials", str(n_trials), "--out-dir", d])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        done = O.run_study(a, log=lambda *x: print(*x, flush=True))  # (one line per population: a long, quiet run)
        torch.cuda.synchronize()
        total = time.perf_counter() - t0
    b = O.best_trial(done)
    groups = O.group_trials(O.make_trials(n_trials, a.seed, a.n_envs, search_arch=True), a.n_jobs)
    return {"n_trials": n_trials, "n_timesteps": a.n_timesteps, "n_envs": a.n_envs, "largest_population": a.n_jobs,
            "populations": len(groups), "population_sizes": sorted(len(g) for g in groups), "seconds": total,
            "complete": sum(t.state == O.COMPLETE for t in done), "pruned": sum(t.state == O.PRUNED for t in done),
            "best_value": None if b is None else b.value, "best_trial": None if b is None else b.number,
            "best_params": None if b is None else b.params}


def readme(res) -> str:
    lines = ["# ArchPopulationPPO against the stand-alone PPO with both arch flags", "",
             f"{res['device']}, torch {res['torch']}. {res['workload']}.", "",
             "| net | members | population iteration (s) | stand-alone iteration (s) | speed-up over serial |",
             "|---|---|---|---|---|"]
    for r in res["sizes"]:
        lines.append(f"| {tuple(r['net_arch'])} {r['activation']} | {r['members']} | {r['population_iteration_s']:.3f} | "
                     f"{r['standalone_iteration_s']:.3f} | {r['speedup_vs_serial']:.1f}x |")
    lines += ["", "The bar (DESIGN 18): a 64-member iteration in less than half of 64 stand-alone iterations.", ""]
    for r in res["sizes"]:
        if r["members"] == 64:
            verdict = "meets" if r["speedup_vs_serial"] > 2.0 else "MISSES"
            lines.append(f"- {tuple(r['net_arch'])} {r['activation']}: {r['speedup_vs_serial']:.1f}x, {verdict} the bar")
    if "optimize" in res:
        o = res["optimize"]
        lines += ["", f"`optimize --search-arch --n-trials {o['n_trials']}`: {o['seconds']:.0f} s, {o['populations']} "
                      f"populations (sizes {o['population_sizes']}), {o['complete']} complete / {o['pruned']} pruned, best "
                      f"{o['best_value']} ({o['best_params']})."]
    return "\n".join(lines) + "\n"


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1, 16, 64, 256])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--optimize", type=int, default=0, metavar="N",
                    help="also time a full optimize --search-arch run of N trials")
    ap.add_argument("--out-dir", default=os.path.join(REPO, "profiles", "arch_population"))
    a = ap.parse_args(argv)
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "workload":
           "trial 31 hyperparameters, 8 envs per member, hover + RateControlWrapper: 1,024-step rollout + 20 epochs x "
           "64 minibatches of 128 rows; medians after a warm-up iteration", "sizes": []}

    def write():
        os.makedirs(a.out_dir, exist_ok=True)
        with open(os.path.join(a.out_dir, "bench.json"), "w") as f:
            json.dump(res, f, indent=1)
        with open(os.path.join(a.out_dir, "README.md"), "w") as f:
            f.write(readme(res))
        print("wrote", a.out_dir, flush=True)

    for hidden, act in NETS:
        res["sizes"] += bench_net(hidden, act, a.sizes, a.reps)
    write()  # the study below takes far longer than the sizes: keep what is measured
    if a.optimize:
        res["optimize"] = optimize_run(a.optimize)
        print(json.dumps(res["optimize"]), flush=True)
        write()
    return 0


if __name__ == "__main__":
    sys.exit(main())
