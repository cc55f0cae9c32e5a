#!/usr/bin/env python3
"""Timing of waypoint laps in one launch (HIP events, warmed up, 5 alternating repetitions), at 1,024 and 65,536
hover envs, the `eight` set at spacing 0.5, 2,000 steps, with a reach radius nobody meets (0 in the fused
launches, whose distance test is strict; the smallest radius quad_waypoints_update accepts in the loop), so
nobody finishes early and every form does the same work:

  wp_policy_env / wp_policy_deployed   quad_policy_waypoints, either observation mode (RateControlWrapper)
  loop                                 bar 1: evaluate_waypoints' per-step body -- quad_policy_act + quad_step +
                                       quad_waypoints_update per step, a host sync every 128 steps
  episode_policy_env / _deployed       bar 2: quad_policy_episode for the same envs and steps (no tracker)
  wp_pid_world / wp_se3                quad_ctrl_waypoints (no wrapper)
  episode_pid_world / episode_se3      bar 2 for the laws: quad_ctrl_episode

and a results table: the policy (env observation, and deployed at several alphas) against the four laws on
eight / circle / square at spacing 0.5, 256 replicas each, reach radius 0.25, 5,000 steps: laps completed,
steps, waypoints reached, mean position error. The policy is --model, or the HPO-pin configuration trained by
the tool (tools/policy_episode_bench.py's).

    python tools/waypoints_bench.py [--model policy.pt] [--out profiles/waypoints/bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

from policy_episode_bench import WRAP, _timed, train_policy  # noqa: E402
from uav_reinforcement_learning_control_amd import evaluate as EV  # noqa: E402
from uav_reinforcement_learning_control_amd.controllers import ctrl_episode, ctrl_waypoints  # noqa: E402
from uav_reinforcement_learning_control_amd.envs import QuadVecEnv  # noqa: E402
from uav_reinforcement_learning_control_amd.ppo.fused import FusedPolicy  # noqa: E402
from uav_reinforcement_learning_control_amd.utils.trajectories import make_trajectory  # noqa: E402
from uav_reinforcement_learning_control_amd.waypoints import WaypointCourse  # noqa: E402

TINY = 1e-30  # a radius no float32 position meets: quad_waypoints_update asks for one above 0


class _Side:
    """One env with its course, restorable to the state right after begin."""

    def __init__(self, n, T, wrapper, dev):
        self.env = QuadVecEnv(n, wrapper=wrapper, device=dev, seed=1, max_episode_steps=T, auto_reset=False)
        self.env.reset()
        self.course = WaypointCourse([make_trajectory("eight", spacing=0.5)], n, 0.0, dev)
        self.obs0 = self.course.begin(self.env).clone()
        self.start = self.env.get_state()
        self.trk0 = {k: v.clone() for k, v in self.course.tracker.items()}

    def restore(self):
        self.env.set_state(**self.start)
        for k, v in self.trk0.items():
            self.course.tracker[k].copy_(v)


def bench_size(policy, n: int, T: int, reps: int) -> dict:
    dev = torch.device("cuda", 0)
    fp = FusedPolicy(policy)
    fp.pack()
    pol, law = _Side(n, T, WRAP, dev), _Side(n, T, None, dev)
    done = {}
    act = EV._Actor(policy, n, dev)
    obs = torch.zeros(n, 12, device=dev)

    def loop():  # evaluate_waypoints' per-step body
        e, c = pol.env, pol.course
        c.reach_radius = TINY
        obs.copy_(pol.obs0)
        for t in range(T):
            a = act(obs)
            _, rew, te, tr, info = e.step(a, obs=obs, info="full")
            c.update(e, info["state"], rew, te, tr)
            if (t + 1) % 128 == 0 and bool((c.tracker["status"] != 0).all()):
                break
        c.reach_radius = 0.0
        done["loop"] = {"steps": c.tracker["steps"].clone()}

    def wp_policy(mode):
        def run():
            done["wp_policy_" + mode] = fp.waypoints(pol.env, pol.course, max_steps=T, obs_mode=mode)
        return run

    def ep_policy(mode):
        def run():
            done["episode_policy_" + mode] = fp.episode(pol.env, max_steps=T, obs_mode=mode)
        return run

    def wp_law(name):
        def run():
            done["wp_" + name] = ctrl_waypoints(law.env, law.course, law=name, max_steps=T)
        return run

    def ep_law(name):
        def run():
            done["episode_" + name] = ctrl_episode(law.env, law=name, max_steps=T)
        return run

    forms = [("wp_policy_env", wp_policy("env")), ("episode_policy_env", ep_policy("env")),
             ("wp_policy_deployed", wp_policy("deployed")), ("episode_policy_deployed", ep_policy("deployed")),
             ("loop", loop),
             ("wp_pid_world", wp_law("pid_world")), ("episode_pid_world", ep_law("pid_world")),
             ("wp_se3", wp_law("se3")), ("episode_se3", ep_law("se3"))]
    with torch.no_grad():
        for _, fn in forms:  # warm-up: code objects, allocator
            pol.restore(); law.restore()
            torch.cuda.synchronize()
            fn()
            torch.cuda.synchronize()
        ms = {k: [] for k, _ in forms}
        for _ in range(reps):  # alternate the forms
            for k, fn in forms:
                pol.restore(); law.restore()
                torch.cuda.synchronize()
                ms[k].append(_timed(fn))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    pairs = (("policy_env", "wp_policy_env", "episode_policy_env"), ("policy_deployed", "wp_policy_deployed",
             "episode_policy_deployed"), ("pid_world", "wp_pid_world", "episode_pid_world"), ("se3", "wp_se3", "episode_se3"))
    rec = {"envs": n, "steps": T, "reps": reps,
           "ms": {k: [round(x, 3) for x in v] for k, v in ms.items()},
           "ms_median": {k: round(v, 3) for k, v in med.items()},
           "ms_range": {k: [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()},
           "bar1_loop_over_wp_policy_env": round(med["loop"] / med["wp_policy_env"], 2),
           "bar2_wp_over_episode": {k: round(med[a] / med[b], 3) for k, a, b in pairs},
           "bar2_episode_range_over_median": {k: [round(min(ms[b]) / med[b], 3), round(max(ms[b]) / med[b], 3)]
                                              for k, _, b in pairs},
           "env_steps": {k: int(v["steps"].sum().item()) for k, v in done.items()}, "env_steps_full": n * T}
    pol.env.close(); law.env.close()
    return rec


def _row(r: dict) -> dict:
    st = np.asarray(r["status"])
    out = {"envs": int(len(st)), "laps": int((st == 1).sum()), "terminated": int((st == 2).sum()),
           "max_steps": int((st == 3).sum()), "mean_steps": float(np.mean(r["steps"])),
           "mean_lap_steps": float(np.mean(r["steps"][st == 1])) if (st == 1).any() else None,
           "mean_reached": float(np.mean(r["reached"])), "mean_pos_error": float(np.mean(r["pos_errors"]))}
    by = {}
    for name in dict.fromkeys(r["name"].tolist()):
        m = r["name"] == name
        by[name] = {"laps": int((st[m] == 1).sum()), "mean_steps": float(np.mean(r["steps"][m])),
                    "mean_reached": float(np.mean(r["reached"][m])), "n_waypoints": int(r["n_waypoints"][m][0]),
                    "mean_pos_error": float(np.mean(r["pos_errors"][m]))}
    out["by_course"] = by
    return out


def results_table(policy, alphas, replicas: int, max_steps: int) -> dict:
    kw = dict(trajectories=["eight", "circle", "square"], spacings=[0.5], reach_radius=0.25, max_steps=max_steps,
              replicas=replicas)
    rows = {"policy": EV.evaluate_waypoints(policy, wrapper=WRAP, **kw)}
    for a in alphas:
        rows[f"policy deployed a={a:g}"] = EV.evaluate_waypoints(policy, wrapper=WRAP, obs_mode="deployed",
                                                                 velocity_alpha=a, **kw)
    for law in ("pid", "se3", "smc", "lqr"):
        rows[law] = EV.evaluate_ctrl_waypoints(law, None, **kw)
    print(EV.lap_table(list(rows.items())), flush=True)
    return {"courses": "eight / circle / square at spacing 0.5", "replicas": replicas, "reach_radius": 0.25,
            "max_steps": max_steps, "rows": {k: _row(v) for k, v in rows.items()}}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--model", default=None, help="policy archive / state dict (default: train the HPO-pin configuration)")
    ap.add_argument("--envs", type=int, nargs="+", default=[1024, 65536])
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--alphas", type=float, nargs="+", default=[0.0, 0.5, 0.8, 0.95])
    ap.add_argument("--replicas", type=int, default=256)
    ap.add_argument("--lap-steps", type=int, default=5000)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "waypoints", "bench.json"))
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "waypoints_bench.py needs the GPU"
    rec = {"device": torch.cuda.get_device_name(0), "course": "eight at spacing 0.5, reach radius 0"}
    if a.model:
        policy, _ = EV.load_policy(a.model, torch.device("cuda", 0))
        rec["policy"] = os.path.basename(a.model)
    else:
        policy, secs = train_policy()
        rec["policy"] = "HPO-pin configuration, seed 0, 500k steps"
        rec["train_seconds"] = round(secs, 2)
    rec["sizes"] = [bench_size(policy, n, a.steps, a.reps) for n in a.envs]
    for s in rec["sizes"]:
        print(json.dumps({k: s[k] for k in ("envs", "ms_median", "bar1_loop_over_wp_policy_env", "bar2_wp_over_episode")}),
              flush=True)
    rec["results"] = results_table(policy, a.alphas, a.replicas, a.lap_steps)
    print(json.dumps(rec))
    if a.out:
        d = os.path.dirname(os.path.abspath(a.out))
        os.makedirs(d, exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(rec, indent=1) + "\n")
    return rec


if __name__ == "__main__":
    main()
