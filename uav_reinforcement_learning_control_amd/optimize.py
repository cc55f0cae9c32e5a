"""Hyperparameter search for PPO hover control on populations: the counterpart of the reference's optimize.py.

    python -m uav_reinforcement_learning_control_amd.optimize --n-trials 256 --n-timesteps 500000

The reference runs an Optuna study (optimize.py:235-300): one SB3 PPO run per trial on 8 CPU envs, ten
evaluations of ten deterministic episodes, a median pruner. Here the trials are sampled up front by a seeded
random search over the same space (optimize.py:33-74, the batch clamp of :135-144), grouped by the shapes a
population must share -- (n_steps, clamped batch_size) -- and every group trains as ONE population (ppo.population_for)
(several when it exceeds --n-jobs): each step of the algorithm is one launch for all the group's trials
(DESIGN section 18). n_epochs varies inside a group (a member whose epochs are done leaves the launch's subset);
a pruned trial is deactivated and costs nothing further.

Protocol (the one tests/hpo_repro.py documents): HoverEnv + RateControlWrapper, --n-envs envs per trial, ten
evaluations of ten deterministic episodes, one every n_timesteps // 10 env steps, each on the policy of the
rollout in which the evaluation point falls; a trial's value is its last evaluation's mean reward.

Pruning restates Optuna's MedianPruner(n_startup_trials=5, n_warmup_steps=3): at an evaluation index past
the warm-up, and once five trials have completed, a trial is pruned when its best value so far is below the
median of the values reported at that index by the trials completed earlier and by the other members of its
population. A trial whose parameters turn non-finite scores NaN (optimize.py:165-175).

By default net_arch is fixed to "small" ([128, 128]) and activation_fn to "relu", the net of the specialised kernels.
--search-arch samples the reference's whole space (optimize.py:44-45): net_arch in {small, medium, large} x
activation_fn in {tanh, relu}. A population shares its arch, so the groups are then keyed on it too, and
ppo.population_for trains (small, relu) groups on PopulationPPO and the other five on ArchPopulationPPO (DESIGN
section 25). The sampler is random search, not TPE; Optuna is not a dependency, so --storage is accepted and ignored.

--deployed trains and evaluates every trial on the observation the reference's ROS2 node hands the policy (DESIGN
section 28): the trials get obs_mode="deployed" and --velocity-alpha, the groups train as ppo.deployed_population_for's
populations, and the in-study evaluations fly deployed at the trial's alpha. --search-alpha also draws the estimator's
coefficient per trial from {0.0, 0.5, 0.8, 0.95}, after every draw the sampler makes without it (so trial k's other
parameters are what they are without the flag), and appends a params_velocity_alpha column to the CSV.
"""
from __future__ import annotations

import argparse
import csv
import datetime as _dt
import json
import math
import os
import random
import statistics
import sys
import time
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

WRAPPER = "RateControlWrapper"
N_EVALUATIONS = 10
N_EVAL_EPISODES = 10
N_STEPS_CHOICES = (256, 512, 800, 1024, 2048)
BATCH_CHOICES = (64, 128, 256, 512)
N_EPOCHS_CHOICES = (3, 5, 10, 20)
NET_ARCH_NAME, ACTIVATION_NAME = "small", "relu"   # what is trained without --search-arch
NET_ARCH = {"small": [128, 128], "medium": [256, 256], "large": [512, 256]}   # the reference's optimize.py:60-64
NET_ARCH_CHOICES, ACTIVATION_CHOICES = ("small", "medium", "large"), ("tanh", "relu")
ACTIVATION_CLASS = {"relu": "ReLU", "tanh": "Tanh"}

# the columns of the reference's study_results_<study>.csv (optuna's trials_dataframe)
CSV_COLUMNS = ("number", "value", "datetime_start", "datetime_complete", "duration", "params_activation_fn",
               "params_batch_size", "params_clip_range", "params_ent_coef", "params_gae_lambda", "params_gamma_inv",
               "params_learning_rate", "params_n_epochs", "params_n_steps", "params_net_arch", "user_attrs_gamma",
               "user_attrs_net_arch_name", "state")
COMPLETE, PRUNED, WAITING = "COMPLETE", "PRUNED", "WAITING"
VELOCITY_ALPHA_CHOICES = (0.0, 0.5, 0.8, 0.95)   # --search-alpha
ALPHA_COLUMN = "params_velocity_alpha"            # appended to CSV_COLUMNS under --search-alpha


def _log_uniform(rng: random.Random, lo: float, hi: float) -> float:
    return math.exp(rng.uniform(math.log(lo), math.log(hi)))


def sample_ppo_params(rng: random.Random, n_steps_choices: Sequence[int] = N_STEPS_CHOICES,
                      search_arch: bool = False) -> dict:
    """One draw from the reference's search space (optimize.py:36-45), in its order of suggestions. search_arch: draw
    net_arch and then activation_fn after ent_coef, as the reference does; without it they are fixed and the rng is
    not advanced for them."""
    p = {
        "learning_rate": _log_uniform(rng, 1e-5, 1e-3),
        "n_steps": rng.choice(list(n_steps_choices)),
        "batch_size": rng.choice(BATCH_CHOICES),
        "n_epochs": rng.choice(N_EPOCHS_CHOICES),
        "gamma_inv": _log_uniform(rng, 0.001, 0.05),
        "gae_lambda": rng.uniform(0.9, 0.99),
        "clip_range": rng.uniform(0.1, 0.3),
        "ent_coef": _log_uniform(rng, 1e-5, 0.1),
        "net_arch": NET_ARCH_NAME,
        "activation_fn": ACTIVATION_NAME,
    }
    if search_arch:
        p["net_arch"] = rng.choice(NET_ARCH_CHOICES)
        p["activation_fn"] = rng.choice(ACTIVATION_CHOICES)
    return p


def clamp_batch_size(n_steps: int, n_envs: int, batch_size: int) -> int:
    """The minibatch a trial trains with: the sampled one if it divides the rollout buffer, else the largest
    choice below it that does, else the whole buffer as a single batch (the rule of optimize.py:135-144)."""
    rollout = int(n_steps) * int(n_envs)
    if rollout % batch_size == 0:
        return int(batch_size)
    for bs in sorted(BATCH_CHOICES, reverse=True):
        if bs <= batch_size and rollout % bs == 0:
            return bs
    return rollout


@dataclass
class Trial:
    number: int
    params: dict
    seed: int
    batch: int                      # the clamped minibatch
    state: str = WAITING
    value: float = float("nan")
    values: Dict[int, float] = field(default_factory=dict)   # evaluation index (1..10) -> mean reward
    start: Optional[_dt.datetime] = None
    end: Optional[_dt.datetime] = None
    obs_mode: str = "env"           # "deployed" under --deployed
    velocity_alpha: float = 0.8     # the estimator's coefficient of a deployed trial

    @property
    def gamma(self) -> float:
        return 1.0 - self.params["gamma_inv"]


def make_trials(n_trials: int, seed: int, n_envs: int, n_steps_choices: Sequence[int] = N_STEPS_CHOICES,
                search_arch: bool = False, deployed: bool = False, velocity_alpha: float = 0.8,
                search_alpha: bool = False) -> List[Trial]:
    """deployed: the trials collect and are evaluated on the deployed observation at velocity_alpha. search_alpha: the
    coefficient is drawn per trial from VELOCITY_ALPHA_CHOICES once every trial's other parameters are drawn -- the rng
    has then made every draw it makes without the flag, so those parameters do not depend on it -- and is recorded as
    params["velocity_alpha"]."""
    if search_alpha and not deployed:
        raise ValueError("search_alpha draws the deployed observation's coefficient: it needs deployed")
    rng = random.Random(seed)
    out = []
    for k in range(n_trials):
        p = sample_ppo_params(rng, n_steps_choices, search_arch)
        out.append(Trial(k, p, seed=int(seed) * 100_003 + k, batch=clamp_batch_size(p["n_steps"], n_envs, p["batch_size"])))
    for t in out:
        if deployed:
            t.obs_mode, t.velocity_alpha = "deployed", float(velocity_alpha)
        if search_alpha:
            t.velocity_alpha = t.params["velocity_alpha"] = rng.choice(VELOCITY_ALPHA_CHOICES)
    return out


def group_trials(trials: Sequence[Trial], cap: int) -> List[List[Trial]]:
    """Populations: trials with equal (n_steps, clamped batch, net_arch, activation_fn) together, at most `cap` per
    population, in trial order; the populations ordered by their first trial."""
    by_shape: Dict[tuple, List[Trial]] = {}
    for t in trials:
        by_shape.setdefault((t.params["n_steps"], t.batch, t.params["net_arch"], t.params["activation_fn"]), []).append(t)
    groups = []
    for ts in by_shape.values():
        for i in range(0, len(ts), max(1, int(cap))):
            groups.append(ts[i:i + max(1, int(cap))])
    groups.sort(key=lambda g: g[0].number)
    return groups


def population_sizes(groups: Sequence[Sequence[Trial]]) -> str:
    """How many populations a study trains, the largest and the median size."""
    sizes = sorted(len(g) for g in groups)
    return (f"  Populations: {len(sizes)} (largest {sizes[-1]}, median {statistics.median(sizes):g} trials)"
            if sizes else "  Populations: 0")


class MedianPruner:
    """Optuna's MedianPruner(n_startup_trials, n_warmup_steps) restated for a population."""

    def __init__(self, n_startup_trials: int = 5, n_warmup_steps: int = N_EVALUATIONS // 3):
        self.n_startup_trials, self.n_warmup_steps = n_startup_trials, n_warmup_steps

    def should_prune(self, trial: Trial, index: int, finished: Sequence[Trial], peers: Sequence[Trial]) -> bool:
        """trial has just reported values[index]. finished: trials that ended earlier (the COMPLETE ones count);
        peers: the other members of its population still running (their values[index] are already reported)."""
        done = [t for t in finished if t.state == COMPLETE]
        if len(done) < self.n_startup_trials or index <= self.n_warmup_steps:
            return False
        own = [v for i, v in trial.values.items() if i <= index and not math.isnan(v)]
        if not own:
            return True  # nothing but NaN reported so far: Optuna prunes a NaN best value
        best = max(own)
        others = [t.values[index] for t in list(done) + list(peers) if index in t.values and not math.isnan(t.values[index])]
        if not others:
            return False
        return best < statistics.median(others)


# ---- the CSV of the reference (trials_dataframe().to_csv(index=False))
def trial_row(t: Trial) -> dict:
    p = t.params
    dur = (t.end - t.start) if t.start and t.end else None
    extra = {ALPHA_COLUMN: repr(p["velocity_alpha"])} if "velocity_alpha" in p else {}
    return {**_trial_row(t, p, dur), **extra}


def _trial_row(t: Trial, p: dict, dur) -> dict:
    return {"number": t.number, "value": "" if math.isnan(t.value) else repr(float(t.value)),
            "datetime_start": t.start.strftime("%Y-%m-%d %H:%M:%S.%f") if t.start else "",
            "datetime_complete": t.end.strftime("%Y-%m-%d %H:%M:%S.%f") if t.end else "",
            "duration": "" if dur is None else f"{dur.days} days {_hms(dur)}",
            "params_activation_fn": p["activation_fn"], "params_batch_size": p["batch_size"],
            "params_clip_range": repr(p["clip_range"]), "params_ent_coef": repr(p["ent_coef"]),
            "params_gae_lambda": repr(p["gae_lambda"]), "params_gamma_inv": repr(p["gamma_inv"]),
            "params_learning_rate": repr(p["learning_rate"]), "params_n_epochs": p["n_epochs"],
            "params_n_steps": p["n_steps"], "params_net_arch": p["net_arch"], "user_attrs_gamma": repr(t.gamma),
            "user_attrs_net_arch_name": p["net_arch"], "state": t.state}


def _hms(d: _dt.timedelta) -> str:
    s = d.seconds
    return f"{s // 3600:02d}:{s % 3600 // 60:02d}:{s % 60:02d}.{d.microseconds:06d}"


def csv_columns(trials: Sequence[Trial]) -> tuple:
    """CSV_COLUMNS, with ALPHA_COLUMN appended when the trials carry a sampled velocity_alpha (--search-alpha)."""
    return CSV_COLUMNS + ((ALPHA_COLUMN,) if any("velocity_alpha" in t.params for t in trials) else ())


def write_csv(path: str, trials: Sequence[Trial]) -> None:
    with open(path, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=csv_columns(trials))
        w.writeheader()
        for t in sorted(trials, key=lambda t: t.number):
            w.writerow(trial_row(t))


def read_csv(path: str) -> List[dict]:
    """The rows of a study CSV with the numeric columns parsed (value NaN where empty)."""
    out = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            for k in ("number", "params_batch_size", "params_n_epochs", "params_n_steps"):
                r[k] = int(r[k])
            for k in ("params_clip_range", "params_ent_coef", "params_gae_lambda", "params_gamma_inv",
                      "params_learning_rate", "user_attrs_gamma"):
                r[k] = float(r[k])
            if ALPHA_COLUMN in r:
                r[ALPHA_COLUMN] = float(r[ALPHA_COLUMN])
            r["value"] = float(r["value"]) if r["value"] != "" else float("nan")
            out.append(r)
    return out


def best_trial(trials: Sequence[Trial]) -> Optional[Trial]:
    done = [t for t in trials if t.state == COMPLETE and not math.isnan(t.value)]
    return max(done, key=lambda t: t.value) if done else None


def format_best(t: Trial) -> str:
    """The best trial in the reference's "ready-to-use config for train.py" form."""
    p = t.params
    lines = ["", "=" * 60, "Best trial", "=" * 60, f"  Mean reward : {t.value:.2f}", f"  Trial number: {t.number}", "",
             "  Params:"]
    lines += [f"    {k}: {p[k]}" for k in ("learning_rate", "n_steps", "batch_size", "n_epochs", "gamma_inv", "gae_lambda",
                                          "clip_range", "ent_coef", "net_arch", "activation_fn")]
    if t.obs_mode == "deployed":  # the exported policy expects the node's estimator at this coefficient
        lines += [f"    velocity_alpha: {t.velocity_alpha}"]
    lines += ["", "  User attrs:", f"    gamma: {t.gamma}", f"    net_arch_name: {p['net_arch']}", "",
              "  Ready-to-use config for train.py:", "  " + "-" * 40, "",
              "    model = PPO(", '        policy="MlpPolicy",', "        env=vec_env,",
              f"        learning_rate={p['learning_rate']},", f"        n_steps={p['n_steps']},",
              f"        batch_size={p['batch_size']},", f"        n_epochs={p['n_epochs']},", f"        gamma={t.gamma},",
              f"        gae_lambda={p['gae_lambda']},", f"        clip_range={p['clip_range']},",
              f"        ent_coef={p['ent_coef']},", "        policy_kwargs={",
              f'            "net_arch": {NET_ARCH[p["net_arch"]]},',
              f'            "activation_fn": nn.{ACTIVATION_CLASS[p["activation_fn"]]},', "        },",
              "        verbose=1,", '        device="cpu",', "    )", ""]
    return "\n".join(lines)


# ---- the GPU part
def ppo_config(t: Trial):
    from .ppo import PPOConfig
    p = t.params
    return PPOConfig(learning_rate=p["learning_rate"], n_steps=p["n_steps"], batch_size=t.batch, n_epochs=p["n_epochs"],
                     gamma=t.gamma, gae_lambda=p["gae_lambda"], clip_range=p["clip_range"], ent_coef=p["ent_coef"],
                     net_arch=tuple(NET_ARCH[p["net_arch"]]), activation=p["activation_fn"],
                     **(dict(obs_mode="deployed", velocity_alpha=t.velocity_alpha) if t.obs_mode == "deployed" else {}))


def _non_finite_members(pop, members: Sequence[int]) -> List[int]:
    """The members whose parameters hold a NaN or an infinity (one host read for all of them)."""
    import torch
    norms = torch.stack([torch.stack(torch._foreach_norm(pop.member(m).params)).sum() for m in members])
    return [m for m, ok in zip(members, torch.isfinite(norms).tolist()) if not ok]


def save_best(pop, m: int, t: Trial, out_dir: str, n_envs: int, n_timesteps: int) -> str:
    """DIR/hover_policy_final.zip (an SB3 PPO archive of the member's policy) and DIR/config.json."""
    from .export import save_sb3_zip
    os.makedirs(out_dir, exist_ok=True)
    mem = pop.member(m)
    path = save_sb3_zip(os.path.join(out_dir, "hover_policy_final"), mem.policy, mem.opt, mem.cfg,
                        num_timesteps=mem.num_timesteps, n_envs=n_envs, batch_size=t.batch,
                        obs_low=[-1.0] * mem.obs_dim, obs_high=[1.0] * mem.obs_dim)
    cfg = {"total_timesteps": n_timesteps, "n_envs": n_envs, "wrapper": WRAPPER, "env": "hover",
           "trial": t.number, "value": t.value, "seed": t.seed,
           "ppo": {"learning_rate": t.params["learning_rate"], "n_steps": t.params["n_steps"], "batch_size": t.batch,
                   "sampled_batch_size": t.params["batch_size"], "n_epochs": t.params["n_epochs"], "gamma": t.gamma,
                   "gae_lambda": t.params["gae_lambda"], "clip_range": t.params["clip_range"],
                   "ent_coef": t.params["ent_coef"], "net_arch": NET_ARCH[t.params["net_arch"]],
                   "activation_fn": ACTIVATION_CLASS[t.params["activation_fn"]]},
           "backend": f"uav_reinforcement_learning_control_amd (MI355X kernels, {type(pop).__name__})",
           # as train --deployed records them: what the exported policy expects of the node's estimator
           **({"obs_mode": t.obs_mode, "velocity_alpha": t.velocity_alpha} if t.obs_mode == "deployed" else {})}
    with open(os.path.join(out_dir, "config.json"), "w") as f:
        json.dump(cfg, f, indent=2)
    return path


def run_population(group: Sequence[Trial], finished: List[Trial], pruner: MedianPruner, n_timesteps: int, n_envs: int,
                   device="cuda:0", save_dir: Optional[str] = None, best_so_far: float = -math.inf, log=print) -> float:
    """Train one group as a population of its arch (ppo.population_for) over the evaluation protocol; fills the trials' values / state / value and
    appends them to `finished` as they end. Returns the best completed value seen (for --save-best)."""
    from .ppo.population import deployed_population_for, population_for
    points = [(k + 1) * (n_timesteps // N_EVALUATIONS) for k in range(N_EVALUATIONS)]
    make = deployed_population_for if group[0].obs_mode == "deployed" else population_for
    pop = make([(ppo_config(t), t.seed) for t in group], n_envs=n_envs, env="hover", wrapper=WRAPPER,
                         device=device)
    now = _dt.datetime.now
    for t in group:
        t.start = now()
    running = {m: t for m, t in enumerate(group)}

    def finish(m: int, state: str, value: float) -> None:
        t = running.pop(m)
        t.state, t.value, t.end = state, value, now()
        pop.deactivate(m)
        finished.append(t)

    k = 0
    try:
        while running and k < N_EVALUATIONS:
            pop.collect_rollouts()
            steps = pop.member(next(iter(running))).num_timesteps
            while running and k < N_EVALUATIONS and steps >= points[k]:
                k += 1
                for m in _non_finite_members(pop, list(running)):
                    finish(m, COMPLETE, float("nan"))  # the reference returns NaN for such a trial
                if not running:
                    break
                ev = pop.evaluate(num_episodes=N_EVAL_EPISODES,
                                  seeds=[1_000_003 * (t.seed + 1) + (k - 1) for t in group])
                for m, t in running.items():
                    t.values[k] = ev[m]["mean_reward"]
                for m in [m for m, t in running.items()
                          if pruner.should_prune(t, k, finished, [u for n, u in running.items() if n != m])]:
                    finish(m, PRUNED, running[m].values[k])
            if k >= N_EVALUATIONS:
                break
            if running:
                pop.train()
        for m in list(running):
            t = running[m]
            value = t.values.get(N_EVALUATIONS, float("nan"))
            if save_dir and not math.isnan(value) and value > best_so_far:
                best_so_far = value
                t.value = value
                save_best(pop, m, t, save_dir, n_envs, n_timesteps)
            finish(m, COMPLETE, value)
    finally:
        pop.close()
    arch = f", {group[0].params['net_arch']} {group[0].params['activation_fn']}" if type(pop).__name__ != "PopulationPPO" else ""
    log(f"  population of {len(group)} (n_steps {group[0].params['n_steps']}, batch {group[0].batch}{arch}): "
        + ", ".join(f"#{t.number} {t.state[0]} {t.value:.1f}" for t in group))
    return best_so_far


def run_study(a, n_steps_choices: Sequence[int] = N_STEPS_CHOICES, log=print) -> List[Trial]:
    trials = make_trials(a.n_trials, a.seed, a.n_envs, n_steps_choices, getattr(a, "search_arch", False),
                         deployed=getattr(a, "deployed", False), velocity_alpha=getattr(a, "velocity_alpha", 0.8),
                         search_alpha=getattr(a, "search_alpha", False))
    groups = group_trials(trials, a.n_jobs)
    if getattr(a, "search_arch", False):  # six arch combinations make the populations about six times thinner
        log(population_sizes(groups))
    pruner = MedianPruner()
    finished: List[Trial] = []
    t0, best = time.perf_counter(), -math.inf
    for g in groups:
        if a.timeout is not None and time.perf_counter() - t0 > a.timeout:
            log(f"timeout after {time.perf_counter() - t0:.0f} s: {len(trials) - len(finished)} trials not started")
            break
        best = run_population(g, finished, pruner, a.n_timesteps, a.n_envs, device=a.device, save_dir=a.save_best,
                              best_so_far=best, log=log)
    return finished


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(
        description="Seeded random-search HPO for PPO hover control on PPO populations (the reference's optimize.py). "
                    "net_arch is fixed to small ([128, 128]) and activation_fn to relu unless --search-arch is given.")
    ap.add_argument("--n-trials", type=int, default=50, help="Number of trials")
    ap.add_argument("--n-jobs", type=int, default=64, help="Largest population: trials trained together in one launch")
    ap.add_argument("--timeout", type=int, default=None, help="No new population starts after this many seconds")
    ap.add_argument("--study-name", type=str, default=f"ppo_hover_{WRAPPER}", help="Names study_results_<study>.csv")
    ap.add_argument("--storage", type=str, default=None, help="Accepted and ignored (Optuna is not used)")
    ap.add_argument("--n-timesteps", type=int, default=500_000, help="Training steps per trial")
    ap.add_argument("--n-envs", type=int, default=8, help="Parallel training envs per trial")
    ap.add_argument("--seed", type=int, default=0, help="Seed of the sampler and of the trials")
    ap.add_argument("--save-best", metavar="DIR", default=None,
                    help="Write the best trial's hover_policy_final.zip and config.json there")
    ap.add_argument("--out-dir", default=".", help="Where study_results_<study>.csv goes")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--search-arch", action="store_true",
                    help="Also sample net_arch in {small, medium, large} and activation_fn in {tanh, relu}, the "
                         "reference's whole space; a population then shares its arch too, so populations get thinner")
    ap.add_argument("--deployed", action="store_true",
                    help="Train and evaluate every trial on the observation the ROS2 node hands the policy (the "
                         "estimator's velocity, the clipped row): deployed populations, one launch per step for all")
    ap.add_argument("--velocity-alpha", type=float, default=0.8,
                    help="The estimator's low-pass coefficient under --deployed (policy_node.py's default 0.8)")
    ap.add_argument("--search-alpha", action="store_true",
                    help="Under --deployed: also draw velocity_alpha per trial from {0.0, 0.5, 0.8, 0.95}")
    return ap


def parse_args(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    if a.search_alpha and not a.deployed:
        ap.error("--search-alpha needs --deployed")
    return a


def main(argv=None, n_steps_choices: Sequence[int] = N_STEPS_CHOICES) -> int:
    a = parse_args(argv)
    if a.storage:
        print(f"note: --storage {a.storage} is ignored (no Optuna here; results go to the CSV)")
    print(f"Starting study '{a.study_name}'")
    print(f"  Wrapper  : {WRAPPER}\n  Trials    : {a.n_trials}\n  Population: up to {a.n_jobs}")
    print(f"  Timeout   : {f'{a.timeout}s' if a.timeout else 'none'}\n  Steps/trial: {a.n_timesteps}\n"
          f"  Envs/trial : {a.n_envs}\n")
    if a.deployed:
        print(f"  Observation: deployed (velocity_alpha {'sampled per trial' if a.search_alpha else a.velocity_alpha})\n")
    t0 = time.perf_counter()
    finished = run_study(a, n_steps_choices)
    print(f"\nFinished trials: {len(finished)} in {time.perf_counter() - t0:.1f} s")
    b = best_trial(finished)
    if b is not None:
        print(format_best(b))
    os.makedirs(a.out_dir, exist_ok=True)
    path = os.path.join(a.out_dir, f"study_results_{a.study_name}.csv")
    write_csv(path, finished)
    print(f"\nResults saved to {path}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
