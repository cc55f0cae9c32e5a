"""Measure ppo.DeployedPopulationPPO against the stand-alone PPO with obs_mode="deployed"; writes
profiles/deployed_population/bench.json and README.md. Each part fills its own key of bench.json and
leaves the others as they are.

  --sizes P ...   trial 31's hyperparameters (tests/golden/hpo_trial31.json) at 8 envs per member, hover +
                  RateControlWrapper, velocity_alpha 0.8: one full iteration -- a rollout of 1,024 steps, then 20 epochs
                  x 64 minibatches of 128 rows -- after a warm-up iteration, for the nets (64, 64) tanh, (128, 128) relu
                  and (512, 256) relu. A DeployedPopulationPPO of P members (seeds 0..P-1) is timed, alternating in the
                  same process with the stand-alone deployed PPO iteration; rollout and update are timed separately on a
                  host clock closed by a device synchronize, medians of --reps. The bar is DESIGN 18's: a 64-member
                  iteration must take less than half of 64 stand-alone iterations; a net that misses it belongs in
                  ppo.population.DEPLOYED_POPULATION_KEEP_SERIAL.
  --learn         DESIGN 27's learning table as ONE population: 24 members = seeds 0..7 x velocity_alpha {0.5, 0.8, 0.95},
                  trial 31's hyperparameters, 500,000 steps each; every final policy flies 1,024 deployed evaluation
                  episodes at its own alpha, at 0.8 and at 0.95 (three launches for all members). Wall time, and the
                  return's median and range over the seeds per training alpha.
  --optimize N    one `optimize --deployed --velocity-alpha 0.95 --n-trials N` study at its defaults, timed.
  --guard DIR     (no GPU) the env-mode objects of this tree's build against a build of the parent commit's in DIR
                  (its _lib/obj): are the fat-binary sections of actor_rollout_k*_m*.o and the actor_arch objects
                  byte-identical, and, where an object gained kernels, is every kernel the parent had the same
                  instruction stream (llvm-objdump of the gfx950 code object, kernel by kernel; the parent's
                  k_pop_actor_episode<KIND, CTBR, MB> is this tree's <KIND, CTBR, QUAD_OBS_ENV, MB>).

  --guard-time PARENT.so
                  the env-mode quad_actor_episode (1,024 envs) and quad_pop_episode (16 members x 256 envs) launches of
                  this tree's library against a build of the parent commit's, hover + RateControlWrapper, from the same
                  re-seeded reset every time: one process per library and turn (the library is chosen when the process
                  starts), parent and this tree taking turns --turns times, each process the median of --reps launches.
                  The spread is the parent's own: the range of its turns' medians.

    python tools/deployed_population_bench.py --sizes 16 64 256 --reps 3 --learn --optimize 256
"""
from __future__ import annotations

import argparse
import dataclasses
import glob
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

WRAPPER = "RateControlWrapper"
NETS = (((64, 64), "tanh"), ((128, 128), "relu"), ((512, 256), "relu"))
OUT_DIR = os.path.join(REPO, "profiles", "deployed_population")
LEARN_ALPHAS, LEARN_SEEDS, EVAL_ALPHAS = (0.5, 0.8, 0.95), tuple(range(8)), (0.8, 0.95)
TOTAL_STEPS, EPISODES = 500_000, 1024
# DESIGN 27's serial table (profiles/deployed_train): the same runs one process each, and what they reached
SERIAL = {"train_s_per_run": "14-15", "runs": 24, "return_median": {"0.8": 439, "0.95": 370}}


def _timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _cfg(hidden, activation, alpha=0.8):
    from hpo_repro import ppo_config
    return dataclasses.replace(ppo_config(), net_arch=tuple(hidden), activation=activation, fused_rollout_arch=True,
                               fused_update_arch=True, obs_mode="deployed", velocity_alpha=alpha)


# ---------------------------------------------------------------- --sizes
def bench_net(hidden, activation, sizes, reps):
    import torch
    from uav_reinforcement_learning_control_amd.envs import QuadVecEnv
    from uav_reinforcement_learning_control_amd.ppo import PPO, DeployedPopulationPPO
    cfg = _cfg(hidden, activation)
    solo = PPO(QuadVecEnv(8, env="hover", wrapper=WRAPPER, device="cuda:0", seed=0), cfg, seed=0)
    solo.collect_rollouts(); solo.train()  # warm-up iteration (captures the epoch graph)
    out = []
    for P in sizes:
        pop = DeployedPopulationPPO([(cfg, s) for s in range(P)], n_envs=8, env="hover", wrapper=WRAPPER,
                                    device="cuda:0")
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
             "classes": [type(solo._fp).__name__, type(solo._learner).__name__],
             "median_seconds": med, "population_iteration_s": pop_it, "standalone_iteration_s": solo_it,
             "speedup_vs_serial": P * solo_it / pop_it, "env_steps_per_s": P * 8 * 1024 / pop_it}
        print(json.dumps({k: v for k, v in r.items() if k != "seconds"}), flush=True)
        out.append(r)
        pop.close()
        del pop
        torch.cuda.empty_cache()
    return out


# ---------------------------------------------------------------- --learn
def learn():
    import torch
    from uav_reinforcement_learning_control_amd.ppo import DeployedPopulationPPO
    spec = [(a, s) for a in LEARN_ALPHAS for s in LEARN_SEEDS]
    t0 = time.perf_counter()
    pop = DeployedPopulationPPO([(_cfg((128, 128), "relu", a), s) for a, s in spec], n_envs=8, env="hover",
                                wrapper=WRAPPER, device="cuda:0")
    built = time.perf_counter() - t0
    pop.learn(TOTAL_STEPS)
    torch.cuda.synchronize()
    train_s = time.perf_counter() - t0 - built
    seeds = [100_000 + s for _, s in spec]  # DESIGN 27's evaluation seeds
    evals, t1 = {}, time.perf_counter()
    for name, alpha in [("own", None)] + [(str(a), a) for a in EVAL_ALPHAS]:
        ev = pop.evaluate(num_episodes=EPISODES, seeds=seeds, velocity_alpha=alpha)
        evals[name] = [{"return": e["mean_reward"], "reach_limit": float(1.0 - e["terminated"].mean())} for e in ev]
    eval_s = time.perf_counter() - t1
    runs = [{"velocity_alpha": a, "seed": s, "num_timesteps": pop.member(m).num_timesteps,
             "eval": {k: v[m] for k, v in evals.items()}} for m, (a, s) in enumerate(spec)]
    pop.close()
    table = []
    for a in LEARN_ALPHAS:
        mine = [r for r in runs if r["velocity_alpha"] == a]
        row = {"train_alpha": a, "seeds": [r["seed"] for r in mine], "eval": {}}
        for k in evals:
            ret = [r["eval"][k]["return"] for r in mine]
            lim = [r["eval"][k]["reach_limit"] for r in mine]
            row["eval"][k] = {"return_median": statistics.median(ret), "return_min": min(ret), "return_max": max(ret),
                              "reach_limit_median": statistics.median(lim)}
        table.append(row)
        print(json.dumps(row), flush=True)
    return {"members": len(spec), "total_timesteps": TOTAL_STEPS, "episodes": EPISODES, "build_s": built,
            "train_s": train_s, "eval_s": eval_s, "serial": SERIAL, "table": table, "runs": runs}


# ---------------------------------------------------------------- --optimize
def optimize_run(n_trials, alpha=0.95):
    import torch
    from uav_reinforcement_learning_control_amd import optimize as O
    with tempfile.TemporaryDirectory() as d:
        a = O.parse_args(["--deployed", "--velocity-alpha", str(alpha), "--n-trials", str(n_trials), "--out-dir", d])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        done = O.run_study(a, log=lambda *x: print(*x, flush=True))  # (one line per population: a long, quiet run)
        torch.cuda.synchronize()
        total = time.perf_counter() - t0
    b = O.best_trial(done)
    groups = O.group_trials(O.make_trials(n_trials, a.seed, a.n_envs, deployed=True, velocity_alpha=alpha), a.n_jobs)
    return {"n_trials": n_trials, "velocity_alpha": alpha, "n_timesteps": a.n_timesteps, "n_envs": a.n_envs,
            "largest_population": a.n_jobs, "populations": len(groups), "population_sizes": sorted(len(g) for g in groups),
            "seconds": total, "complete": sum(t.state == O.COMPLETE for t in done),
            "pruned": sum(t.state == O.PRUNED for t in done), "best_value": None if b is None else b.value,
            "best_trial": None if b is None else b.number, "best_params": None if b is None else b.params,
            "beats_design27_370": bool(b is not None and b.value > SERIAL["return_median"]["0.95"])}


# ---------------------------------------------------------------- --guard
def _kernels(obj, work):
    """{kernel symbol: its instruction lines} of the gfx950 code object in obj's fat-binary section, and the section."""
    llvm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
    fb, co = os.path.join(work, "fb.bin"), os.path.join(work, "dev.co")
    subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fb], check=True)
    subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fb,
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], check=True)
    text = subprocess.run([os.path.join(llvm, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co],
                          capture_output=True, text=True, check=True).stdout
    ks, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^\S* ?<(\S+)>:$", line.strip())
        if m:
            cur = m.group(1)
            ks[cur] = []
        elif cur and line.strip():
            ks[cur].append(re.sub(r"//.*", "", line).strip())
    with open(fb, "rb") as f:
        return ks, f.read()


def guard(parent_obj):
    mine = os.path.join(REPO, "uav_reinforcement_learning_control_amd", "_lib", "obj")
    names = sorted(os.path.basename(f) for pat in ("actor_rollout_k*_m*.o", "actor_rollout.o", "actor_arch*.o")
                   for f in glob.glob(os.path.join(parent_obj, pat)))
    out = []
    with tempfile.TemporaryDirectory() as d:
        for n in names:
            ko, fo = _kernels(os.path.join(parent_obj, n), d)
            kn, fn = _kernels(os.path.join(mine, n), d)
            same, moved = 0, []
            for name, body in ko.items():
                twin = name
                m = re.search(r"k_pop_actor_episodeILi(\d)ELb(\d)ELi(\d)E", name)
                if twin not in kn and m:
                    twin = next((k for k in kn if f"k_pop_actor_episodeILi{m[1]}ELb{m[2]}ELi0ELi{m[3]}E" in k), None)
                if twin is not None and kn.get(twin) == body:
                    same += 1
                else:
                    moved.append(name)
            out.append({"object": n, "fatbin_identical": fo == fn, "parent_kernels": len(ko), "kernels": len(kn),
                        "parent_kernels_with_identical_instructions": same, "changed": moved})
            print(json.dumps(out[-1]), flush=True)
    return {"objects": out, "all_parent_kernels_identical": all(not o["changed"] for o in out)}


GUARD_NETS = (((64, 64), "tanh"), ((256, 256), "tanh"), ((512, 256), "relu"))  # (ArchPopulationPPO's nets)


class _TimedLib:
    """The library with quad_pop_episode timed on a host clock closed by device synchronizes."""

    def __init__(self, lib, into):
        self._lib, self._into = lib, into

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name != "quad_pop_episode":
            return fn

        def timed(*a):
            import torch
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rc = fn(*a)
            torch.cuda.synchronize()
            self._into.append(1e3 * (time.perf_counter() - t0))
            return rc
        return timed


def guard_time_child(reps):
    import torch
    from uav_reinforcement_learning_control_amd.envs import QuadVecEnv
    from uav_reinforcement_learning_control_amd.ppo import ArchPopulationPPO, PPOConfig
    from uav_reinforcement_learning_control_amd.ppo.fused import FusedActor
    rows = []
    for hidden, act in GUARD_NETS:
        cfg = PPOConfig(n_steps=32, batch_size=64, net_arch=hidden, activation=act, fused_rollout_arch=True,
                        fused_update_arch=True)
        pop = ArchPopulationPPO([(cfg, s) for s in range(16)], n_envs=8, env="hover", wrapper=WRAPPER, device="cuda:0")
        actor = FusedActor(pop.member(0).policy)
        actor.pack()
        env = QuadVecEnv(1024, env="hover", wrapper=WRAPPER, device="cuda:0", seed=1, auto_reset=False)
        single, many = [], []
        pop._lib = _TimedLib(pop._lib, many)
        for r in range(reps + 1):  # one warm-up turn first
            env.reset(seed=1)
            t = _timed(lambda: actor.episode(env))
            pop.evaluate(num_episodes=256, seeds=list(range(100, 116)))
            if r:
                single.append(1e3 * t)
        rows.append({"net_arch": list(hidden), "activation": act, "quad_actor_episode_ms": statistics.median(single),
                     "quad_pop_episode_ms": statistics.median(many[1:])})
        env.close()
        pop.close()
        torch.cuda.empty_cache()
    print("GUARDT " + json.dumps(rows), flush=True)


def guard_time(parent_lib, turns, reps):
    parent_lib = os.path.abspath(parent_lib)
    if not os.path.exists(parent_lib):
        raise SystemExit(f"--guard-time: {parent_lib} does not exist (build the parent commit's csrc with OUT=...)")
    runs = {"parent": [], "tree": []}
    for _ in range(turns):
        for who in ("parent", "tree"):
            env = dict(os.environ)
            env.pop("QUADENV_LIB", None)
            if who == "parent":
                env["QUADENV_LIB"] = parent_lib
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--guard-time-child", "--reps", str(reps)],
                                 env=env, capture_output=True, text=True, timeout=600)
            line = [ln for ln in res.stdout.splitlines() if ln.startswith("GUARDT ")]
            if res.returncode != 0 or not line:
                raise SystemExit(f"guard child ({who}) failed: {res.stderr[-600:]}")
            runs[who].append(json.loads(line[0][7:]))
    rows = []
    for k, g in enumerate(runs["tree"][0]):
        for call in ("quad_actor_episode", "quad_pop_episode"):
            p = [r[k][call + "_ms"] for r in runs["parent"]]
            t = [r[k][call + "_ms"] for r in runs["tree"]]
            row = {"net_arch": g["net_arch"], "activation": g["activation"], "call": call,
                   "parent_ms": statistics.median(p), "tree_ms": statistics.median(t), "parent_turns_ms": p,
                   "tree_turns_ms": t, "parent_spread_ms": max(p) - min(p)}
            row["gap_ms"] = row["tree_ms"] - row["parent_ms"]
            row["within_parent_spread"] = abs(row["gap_ms"]) <= row["parent_spread_ms"]
            rows.append(row)
            print(f"guard {tuple(row['net_arch'])} {row['activation']} {call}: parent {row['parent_ms']:.3f} ms, tree "
                  f"{row['tree_ms']:.3f} ms, gap {row['gap_ms']:+.3f} ms, parent's spread {row['parent_spread_ms']:.3f} ms",
                  flush=True)
    return {"turns": turns, "reps": reps, "rows": rows}


# ---------------------------------------------------------------- the record
def readme(res) -> str:
    lines = ['# DeployedPopulationPPO against the stand-alone PPO with obs_mode="deployed"', ""]
    if "sizes" in res:
        lines += [f"{res['device']}, torch {res['torch']}. {res['workload']}.", "",
                  "| net | members | population iteration (s) | rollout / update (s) | stand-alone iteration (s) | "
                  "speed-up over serial |", "|---|---|---|---|---|---|"]
        for r in res["sizes"]:
            m = r["median_seconds"]
            lines.append(f"| {tuple(r['net_arch'])} {r['activation']} | {r['members']} | "
                         f"{r['population_iteration_s']:.3f} | {m['pop_rollout']:.3f} / {m['pop_update']:.3f} | "
                         f"{r['standalone_iteration_s']:.3f} | {r['speedup_vs_serial']:.1f}x |")
        lines += ["", "The bar (DESIGN 18): a 64-member iteration in less than half of 64 stand-alone iterations.", ""]
        for r in res["sizes"]:
            if r["members"] == 64:
                ok = r["speedup_vs_serial"] > 2.0
                lines.append(f"- {tuple(r['net_arch'])} {r['activation']}: {r['speedup_vs_serial']:.1f}x, "
                             + ("meets the bar" if ok else "MISSES the bar: in DEPLOYED_POPULATION_KEEP_SERIAL"))
    if "learn" in res:
        L = res["learn"]
        lines += ["", f"## DESIGN 27's learning table as one population", "",
                  f"{L['members']} members (seeds 0-7 x velocity_alpha 0.5 / 0.8 / 0.95), (128, 128) relu, trial 31's "
                  f"hyperparameters, {L['total_timesteps']:,} steps each: {L['train_s']:.1f} s of training for all of them "
                  f"(+ {L['build_s']:.1f} s to build the members, {L['eval_s']:.1f} s for 3 x {L['members']} x "
                  f"{L['episodes']:,} evaluation episodes), beside {L['serial']['runs']} serial runs of "
                  f"{L['serial']['train_s_per_run']} s each in DESIGN 27.", "",
                  "Return over the seeds, median (min .. max), deployed evaluation:", "",
                  "| trained at alpha | flown at its own alpha | flown at 0.8 | flown at 0.95 | DESIGN 27, own alpha |",
                  "|---|---|---|---|---|"]
        for row in L["table"]:
            c = lambda k: (f"{row['eval'][k]['return_median']:.0f} ({row['eval'][k]['return_min']:.0f} .. "
                           f"{row['eval'][k]['return_max']:.0f})")
            lines.append(f"| {row['train_alpha']} | {c('own')} | {c('0.8')} | {c('0.95')} | "
                         f"{L['serial']['return_median'].get(str(row['train_alpha']), '-')} |")
    if "optimize" in res:
        o = res["optimize"]
        lines += ["", f"`optimize --deployed --velocity-alpha {o['velocity_alpha']} --n-trials {o['n_trials']}`: "
                      f"{o['seconds']:.0f} s, {o['populations']} populations (sizes {o['population_sizes']}), "
                      f"{o['complete']} complete / {o['pruned']} pruned, best {o['best_value']} (trial {o['best_trial']}: "
                      f"{o['best_params']}); " + ("it beats" if o["beats_design27_370"] else "nothing beats")
                      + " DESIGN 27's 370 for trial 31 trained at that alpha."]
    if "guard" in res:
        g = res["guard"]
        lines += ["", "## Guard on the env-mode code", "",
                  "| object | fat-binary section identical to the parent's | kernels (parent / this tree) | parent "
                  "kernels with identical instructions |", "|---|---|---|---|"]
        for o in g["objects"]:
            lines.append(f"| {o['object']} | {'yes' if o['fatbin_identical'] else 'no'} | {o['parent_kernels']} / "
                         f"{o['kernels']} | {o['parent_kernels_with_identical_instructions']} |")
        lines += ["", "Every kernel the parent commit had has the instruction stream it had: "
                      + ("yes" if g["all_parent_kernels_identical"] else "NO") + ". The objects that differ gained the "
                      "deployed instances of k_pop_actor_episode and nothing else."]
    if "guard_time" in res:
        g = res["guard_time"]
        lines += ["", f"Timed all the same, env mode, this tree's library against the parent commit's, {g['turns']} turns "
                      f"each taking turns, medians of {g['reps']} launches (quad_actor_episode: 1,024 envs; "
                      "quad_pop_episode: 16 members x 256 envs):", "",
                  "| net | call | parent (ms) | this tree (ms) | gap (ms) | parent's own spread (ms) | inside it |",
                  "|---|---|---|---|---|---|---|"]
        for r in g["rows"]:
            lines.append(f"| {tuple(r['net_arch'])} {r['activation']} | {r['call']} | {r['parent_ms']:.3f} | "
                         f"{r['tree_ms']:.3f} | {r['gap_ms']:+.3f} | {r['parent_spread_ms']:.3f} | "
                         f"{'yes' if r['within_parent_spread'] else 'no'} |")
    return "\n".join(lines) + "\n"


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="*", default=[])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--learn", action="store_true")
    ap.add_argument("--optimize", type=int, default=0, metavar="N")
    ap.add_argument("--guard", metavar="DIR", default=None)
    ap.add_argument("--guard-time", metavar="PARENT.so", default=None)
    ap.add_argument("--turns", type=int, default=3)
    ap.add_argument("--guard-time-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out-dir", default=OUT_DIR)
    a = ap.parse_args(argv)
    if a.guard_time_child:
        guard_time_child(a.reps)
        return 0
    path = os.path.join(a.out_dir, "bench.json")
    res = {}
    if os.path.exists(path):
        with open(path) as f:
            res = json.load(f)

    def write():
        os.makedirs(a.out_dir, exist_ok=True)
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
        with open(os.path.join(a.out_dir, "README.md"), "w") as f:
            f.write(readme(res))
        print("wrote", a.out_dir, flush=True)

    if a.guard:
        res["guard"] = guard(a.guard)
        write()
    if a.guard_time:
        res["guard_time"] = guard_time(a.guard_time, a.turns, a.reps)
        write()
    if a.sizes or a.learn or a.optimize:
        import torch
        res.update(device=torch.cuda.get_device_name(0), torch=torch.__version__)
    if a.sizes:
        res["workload"] = ("trial 31 hyperparameters, 8 envs per member, hover + RateControlWrapper, obs_mode deployed at "
                           "velocity_alpha 0.8: 1,024-step rollout + 20 epochs x 64 minibatches of 128 rows; medians "
                           "after a warm-up iteration, population and stand-alone taking turns in one process")
        res["sizes"] = []
        for hidden, act in NETS:
            res["sizes"] += bench_net(hidden, act, a.sizes, a.reps)
            write()
    if a.learn:
        res["learn"] = learn()
        write()
    if a.optimize:
        res["optimize"] = optimize_run(a.optimize)
        print(json.dumps(res["optimize"]), flush=True)
        write()
    return 0


if __name__ == "__main__":
    sys.exit(main())
