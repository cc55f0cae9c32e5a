#!/usr/bin/env python3
"""Timing of the PID baseline at 65,536 hover envs x 512 steps (HIP events, warmed up, alternating):

  fused     quad_pid_episode: one launch, state in registers for all 512 steps
  unfused   quad_pid_act + quad_step per step (1,024 launches), the same closed loop
  random    quad_step_random for the same N x steps: the same env work with random actions and no
            law -- the yardstick for what the law costs

and the tuner's wall time at its defaults (4,096 candidates x 16 episodes). Every timed call starts
from the same reset state (set_state is outside the timed window). Writes one JSON record.

    python tools/pid_bench.py [--envs 65536] [--steps 512] [--reps 5] [--tuner] --out profiles/pid/pid_bench.json

With --law (any of se3 smc lqr) it times the controller family instead: each law fused (quad_ctrl_episode) and
unfused (quad_ctrl_act + quad_step per step), with quad_pid_episode in its world-frame mode as the yardstick,
alternating in the same way. SE(3) runs with se3_reorthonormalize = 0 so that its episodes run their full
length (as written it loses every hover episode within ~170 steps, and a fused launch would end early).

    python tools/pid_bench.py --law se3 smc lqr --out profiles/ctrl/ctrl_bench.json
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from uav_reinforcement_learning_control_amd import _native as N  # noqa: E402
from uav_reinforcement_learning_control_amd.envs import QuadVecEnv  # noqa: E402


def _timed(fn) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)  # ms


def bench_laws(a) -> dict:
    from uav_reinforcement_learning_control_amd.controllers import CtrlParams
    n, T = a.envs, a.steps
    env = QuadVecEnv(n, device="cuda:0", seed=1, auto_reset=False)
    env.reset()
    start = env.get_state()

    def restore():
        env.set_state(**start)
        torch.cuda.synchronize()

    params = CtrlParams(se3_reorthonormalize=0.0)
    cs = torch.zeros(N.CTRL_NSTATE, n, dtype=torch.float64, device=env.device)
    s12 = torch.zeros(n, 12, device=env.device)
    ti = torch.zeros(n, 9, device=env.device)
    acts = torch.zeros(n, 4, device=env.device)
    steps_done = {}

    def pid_fused():
        steps_done["pid_world"] = env.pid_episode(mode="world_frame", max_steps=T)["steps"]

    def fused(law):
        def f():
            steps_done[law] = env.ctrl_episode(params, law=law, max_steps=T)["steps"]
        return f

    def unfused(law):
        def f():
            cs.zero_()
            env.observe(state=True)
            s12.copy_(env.state12)
            env.current_target_info(ti)
            for _ in range(T):
                env.ctrl_act(s12, ti, cs, params=params, law=law, out=acts)
                env.step(acts, info="full")
                s12.copy_(env.state12)
                ti.copy_(env.target_info)
        return f

    forms = [("pid_world_fused", pid_fused)]
    for law in a.law:
        forms += [(law + "_fused", fused(law)), (law + "_unfused", unfused(law))]
    for _, f in forms:  # warm-up
        restore()
        f()
        torch.cuda.synchronize()
    ms = {k: [] for k, _ in forms}
    for _ in range(a.reps):  # alternate the forms
        for k, f in forms:
            restore()
            ms[k].append(_timed(f))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    rec = {"envs": n, "steps": T, "reps": a.reps, "device": torch.cuda.get_device_name(0),
           "ms": {k: [round(x, 3) for x in v] for k, v in ms.items()},
           "ms_median": {k: round(v, 3) for k, v in med.items()},
           "ms_range": {k: [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()},
           "ratio_to_pid_world_fused": {k: round(v / med["pid_world_fused"], 3) for k, v in med.items()},
           "env_steps": {k: int(v.sum().item()) for k, v in steps_done.items()}, "env_steps_full": n * T,
           "note": "se3 runs with se3_reorthonormalize = 0 (full-length episodes)"}
    env.close()
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tuner", action="store_true", help="also time tune_pid at its defaults")
    ap.add_argument("--law", nargs="+", choices=["se3", "smc", "lqr"], default=None,
                    help="time these laws of the controller family against the world-frame PID instead")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "pid_bench.py needs the GPU"
    if a.law:
        rec = bench_laws(a)
        print(json.dumps(rec))
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write(json.dumps(rec, indent=1) + "\n")
        return rec
    n, T = a.envs, a.steps
    # auto_reset = 0 and the default 512-step time limit: the three forms do the same n x T env steps
    # except for envs the PID loses early (reported as env_steps_fused); random actions terminate
    # most envs early, and quad_step_random keeps stepping them, like the unfused loop
    env = QuadVecEnv(n, device="cuda:0", seed=1, auto_reset=False)
    env.reset()
    start = env.get_state()

    def restore():
        env.set_state(**start)
        torch.cuda.synchronize()

    integ = torch.zeros(6, n, dtype=torch.float64, device=env.device)
    s12 = torch.zeros(n, 12, device=env.device)
    ti = torch.zeros(n, 9, device=env.device)
    acts = torch.zeros(n, 4, device=env.device)
    steps_done = {}

    def fused():
        steps_done["fused"] = env.pid_episode(max_steps=T)["steps"]

    def unfused():
        integ.zero_()
        env.observe(state=True)
        s12.copy_(env.state12)
        env.current_target_info(ti)
        for _ in range(T):
            env.pid_act(s12, ti, integ, out=acts)
            env.step(acts, info="full")
            s12.copy_(env.state12)
            ti.copy_(env.target_info)

    # quad_step_random's time-major outputs for the whole window (obs alone: n x T x 48 B), allocated once
    ro = {"obs": torch.empty(T, n, 12, device=env.device), "reward": torch.empty(T, n, device=env.device),
          "terminated": torch.empty(T, n, dtype=torch.bool, device=env.device),
          "truncated": torch.empty(T, n, dtype=torch.bool, device=env.device)}
    rout = N.QuadStepOut(obs=ro["obs"].data_ptr(), reward=ro["reward"].data_ptr(),
                         terminated=ro["terminated"].data_ptr(), truncated=ro["truncated"].data_ptr())

    def random():
        N.check(N.lib().quad_step_random(env._h, 0, T, C.byref(rout), None, env._stream()), "quad_step_random")

    forms = (("fused", fused), ("unfused", unfused), ("random", random))
    for _, f in forms:  # warm-up: code objects, allocator
        restore()
        f()
        torch.cuda.synchronize()
    ms = {k: [] for k, _ in forms}
    for _ in range(a.reps):  # alternate the forms
        for k, f in forms:
            restore()
            ms[k].append(_timed(f))
    rec = {"envs": n, "steps": T, "reps": a.reps, "device": torch.cuda.get_device_name(0),
           "ms": {k: [round(x, 3) for x in v] for k, v in ms.items()},
           "ms_median": {k: round(float(np.median(v)), 3) for k, v in ms.items()},
           "env_steps_fused": int(steps_done["fused"].sum().item()), "env_steps_full": n * T,
           "note": "random = one quad_step_random launch of `steps` steps, which also writes obs / reward / flags "
                   "rows for every step (n x steps x 54 B) that the fused PID loop does not"}
    rec["us_per_step"] = {k: round(1e3 * v / T, 3) for k, v in rec["ms_median"].items()}
    env.close()
    if a.tuner:
        from uav_reinforcement_learning_control_amd.tune_pid import tune
        tune(candidates=64, episodes=16, generations=1)  # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = tune()
        torch.cuda.synchronize()
        rec["tuner"] = {"seconds": round(time.perf_counter() - t0, 3), "candidates": r["candidates"],
                        "episodes": r["episodes"], "generations": len(r["history"]), "history": r["history"],
                        "fresh_score": r["fresh_score"], "fresh_start_score": r["fresh_start_score"],
                        "tuning_score": r["tuning_score"], "start_tuning_score": r["start_tuning_score"],
                        "gains": r["gains"].to_dict()}
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(rec, indent=1) + "\n")
    return rec


if __name__ == "__main__":
    main()
