"""Measure ppo.PopulationPPO against the stand-alone PPO it replaces; writes profiles/population/bench.json.

Workload: trial 31's hyperparameters (tests/golden/hpo_trial31.json, the configuration tests/hpo_repro.py
trains) at 8 envs with RateControlWrapper: one full iteration -- a rollout of 1,024 steps, then 20 epochs x 64
minibatches of 128 rows -- after a warm-up iteration. For P in --sizes a PopulationPPO of P members (seeds
0..P-1) is timed, alternating in the same process with the stand-alone PPO iteration; rollout and update are
timed separately on a host clock closed by a device synchronize.

    python tools/population_bench.py --sizes 1 16 64 256 --reps 3 [--seeds48] [--optimize 256]

--optimize N also times a full `optimize --n-trials N` study (its defaults: 500,000 steps per trial, 8 envs,
populations of up to 64).

--seeds48 also trains 48 seeds of the configuration as one population over the hpo_repro protocol (10
evaluations of 10 deterministic episodes every 50,000 steps, each on the policy of the rollout in which the
evaluation point falls; evaluation seeds as hpo_repro's; every evaluation point is one PopulationPPO.evaluate
launch for all 48 members) and records the final evaluations' mean, to be read
beside the stand-alone band of profiles/r06/hpo_repro.json (the members are bit-identical to the stand-alone
runs, so it is the same number).
"""
from __future__ import annotations

import argparse
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


def _sync():
    torch.cuda.synchronize()


def _timed(fn):
    _sync()
    t0 = time.perf_counter()
    fn()
    _sync()
    return time.perf_counter() - t0


def _standalone(cfg, seed=0):
    from uav_reinforcement_learning_control_amd.envs import QuadVecEnv
    from uav_reinforcement_learning_control_amd.ppo import PPO
    env = QuadVecEnv(8, env="hover", wrapper=WRAPPER, device="cuda:0", seed=seed)
    return PPO(env, cfg, seed=seed)


def bench_sizes(sizes, reps):
    from hpo_repro import ppo_config
    from uav_reinforcement_learning_control_amd.ppo.population import PopulationPPO
    cfg = ppo_config()
    solo = _standalone(cfg)
    solo.collect_rollouts(); solo.train()  # warm-up iteration (captures the epoch graph)
    out = []
    for P in sizes:
        pop = PopulationPPO([(cfg, s) for s in range(P)], n_envs=8, env="hover", wrapper=WRAPPER, device="cuda:0")
        pop.collect_rollouts(); pop.train()  # warm-up iteration
        rows = {"pop_rollout": [], "pop_update": [], "solo_rollout": [], "solo_update": []}
        for _ in range(reps):
            rows["pop_rollout"].append(_timed(pop.collect_rollouts))
            rows["pop_update"].append(_timed(pop.train))
            rows["solo_rollout"].append(_timed(solo.collect_rollouts))
            rows["solo_update"].append(_timed(solo.train))
        med = {k: statistics.median(v) for k, v in rows.items()}
        pop_it, solo_it = med["pop_rollout"] + med["pop_update"], med["solo_rollout"] + med["solo_update"]
        r = {"members": P, "reps": reps, "seconds": rows, "median_seconds": med,
             "population_iteration_s": pop_it, "standalone_iteration_s": solo_it,
             "standalone_iterations_equivalent_s": P * solo_it, "speedup_vs_serial": P * solo_it / pop_it,
             "env_steps_per_s": P * 8 * 1024 / pop_it}
        print(json.dumps({k: v for k, v in r.items() if k != "seconds"}), flush=True)
        out.append(r)
        pop.close()
        del pop
        torch.cuda.empty_cache()
    return out


def seeds48(n_seeds=48):
    """tests/hpo_repro.py's GPU protocol for seeds 0..n_seeds-1 as ONE population."""
    from hpo_repro import eval_points, ppo_config
    from uav_reinforcement_learning_control_amd.ppo.population import PopulationPPO
    cfg, points = ppo_config(), eval_points()
    pop = PopulationPPO([(cfg, s) for s in range(n_seeds)], n_envs=8, env="hover", wrapper=WRAPPER, device="cuda:0")
    curves = [[] for _ in range(n_seeds)]
    _sync()
    t0 = time.perf_counter()
    t_eval = 0.0
    while len(curves[0]) < len(points):
        pop.collect_rollouts()
        while len(curves[0]) < len(points) and pop.member(0).num_timesteps >= points[len(curves[0])]:
            te = time.perf_counter()
            k = len(curves[0])
            ev = pop.evaluate(num_episodes=10, seeds=[1_000_003 * (s + 1) + k for s in range(n_seeds)])
            for s in range(n_seeds):
                curves[s].append(ev[s]["mean_reward"])
            t_eval += time.perf_counter() - te
        if len(curves[0]) == len(points):
            break
        pop.train()
    _sync()
    total = time.perf_counter() - t0
    finals = [c[-1] for c in curves]
    pop.close()
    return {"seeds": n_seeds, "seconds": total, "eval_seconds": t_eval, "seconds_per_seed": total / n_seeds,
            "final_mean": statistics.mean(finals), "final_median": statistics.median(finals),
            "final_std": statistics.pstdev(finals), "finals": finals,
            "curves": curves}


def optimize_run(n_trials=256):
    """A full `optimize --n-trials N` study (500,000 steps per trial, populations of up to 64), timed."""
    import tempfile
    from uav_reinforcement_learning_control_amd import optimize as O
    with tempfile.TemporaryDirectory() as d:
        a = O.build_parser().parse_args(["--n-trials", str(n_trials), "--out-dir", d])
        _sync()
        t0 = time.perf_counter()
        done = O.run_study(a, log=lambda *x: None)
        _sync()
        total = time.perf_counter() - t0
    b = O.best_trial(done)
    groups = O.group_trials(O.make_trials(n_trials, a.seed, a.n_envs), a.n_jobs)
    return {"n_trials": n_trials, "n_timesteps": a.n_timesteps, "n_envs": a.n_envs, "largest_population": a.n_jobs,
            "populations": len(groups), "population_sizes": [len(g) for g in groups], "seconds": total,
            "seconds_per_trial": total / n_trials,
            "complete": sum(t.state == O.COMPLETE for t in done), "pruned": sum(t.state == O.PRUNED for t in done),
            "best_value": None if b is None else b.value, "best_trial": None if b is None else b.number,
            "best_params": None if b is None else b.params}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1, 16, 64, 256])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seeds48", action="store_true")
    ap.add_argument("--optimize", type=int, default=0, metavar="N", help="also time a full optimize run of N trials")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "population", "bench.json"))
    a = ap.parse_args(argv)
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "workload":
           "trial 31 hyperparameters, 8 envs, RateControlWrapper: 1,024-step rollout + 20 epochs x 64 minibatches of 128",
           "sizes": bench_sizes(a.sizes, a.reps)}
    if a.seeds48:
        res["seeds48"] = seeds48()
        print(json.dumps({k: v for k, v in res["seeds48"].items() if k not in ("curves", "finals")}), flush=True)
    if a.optimize:
        res["optimize"] = optimize_run(a.optimize)
        print(json.dumps({k: v for k, v in res["optimize"].items() if k != "population_sizes"}), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
