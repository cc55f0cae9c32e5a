#!/usr/bin/env python3
"""A/B tool (not product): SHA-256 digests of everything the general actor's and the Brax-profile policy's entry
points write (csrc/actor_arch.hip, csrc/brax_actor.hip), at small shapes, for the library QUADENV_LIB names (the
in-tree build without it) -- so a refactor of actor_core.h or of either family can be shown to give identical bits:
run it once per build and compare the lists.

Nets (32,64) (96,64) (128,128) (512,256) with every activation of each family. Per net: the packed image; the act
entry point at n = 1, 33 and 65,569 rows (one row past a full grid of 512 blocks x 4 waves x 32 rows, so the
grid-stride loop wraps) -- quad_actor_act's mean and actions, quad_brax_actor_act's logits and actions,
deterministic and sampled; and the episodes: quad_actor_episode on hover and trajectory, with and without
RateControlWrapper, in both observation modes, quad_actor_waypoints in both modes, quad_brax_episode on both brax
kinds, deterministic and sampled. Every episode run: 130 envs (two full blocks and a partial one), 64 steps,
trace_envs = 5; all metrics, all traces and the final env state are digested.

One child process under a time limit, nothing is retried.

    QUADENV_LIB=/path/libquadenv.so python tools/actor_digest.py [--out digests.json] [--timeout 540]
"""
import argparse
import hashlib
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NETS = ((32, 64), (96, 64), (128, 128), (512, 256))
ROWS = (1, 33, 512 * 4 * 32 + 33)
ENVS, STEPS, TRACE = 130, 64, 5


def _digest(*arrays):
    import numpy as np
    import torch
    h = hashlib.sha256()
    for a in arrays:
        h.update((a.detach().cpu().numpy() if torch.is_tensor(a) else np.ascontiguousarray(a)).tobytes())
    return h.hexdigest()[:16]


def _run_digest(res, env):
    return _digest(*[res[k] for k in sorted(res)], *[v for _, v in sorted(env.get_state().items())])


def child():
    sys.path.insert(0, ROOT)
    import torch
    from uav_reinforcement_learning_control_amd.envs import QuadVecEnv
    from uav_reinforcement_learning_control_amd.ppo.brax_ppo import BraxActorCritic, BraxPPOConfig
    from uav_reinforcement_learning_control_amd.ppo.fused import FusedActor, FusedBraxActor
    from uav_reinforcement_learning_control_amd.ppo.policy import ActorCritic
    from uav_reinforcement_learning_control_amd.utils.trajectories import make_trajectory
    from uav_reinforcement_learning_control_amd.waypoints import WaypointCourse
    out = {}
    gen = torch.Generator().manual_seed(5)
    obs12 = (torch.rand(ROWS[-1], 12, generator=gen) * 2 - 1).cuda()
    obs21 = (torch.rand(ROWS[-1], 21, generator=gen) * 2 - 1).cuda()

    def fresh(kind, wrapper):
        e = QuadVecEnv(ENVS, env=kind, wrapper=wrapper, device="cuda:0", seed=3, max_episode_steps=STEPS,
                       auto_reset=False)
        e.reset()
        start = e.get_state()
        if kind == "brax_hover":  # its reset state sits on the floor, below its own z limit
            start["qpos"][:, 2] += 1.0
        return e, start

    # ---- the general actor
    envs = {(k, w): fresh(k, w) for k in ("hover", "trajectory") for w in (None, "RateControlWrapper")}
    for h1, h2 in NETS:
        for act in ("relu", "tanh"):
            torch.manual_seed(0)
            pol = ActorCritic(12, 4, (h1, h2), activation=act)
            with torch.no_grad():
                pol.action_net.bias.copy_(torch.tensor([0.2227 * 9.81 / 26.0 - 1.0, 0.0, 0.0, 0.0]))  # hover thrust
            fa = FusedActor(pol.cuda())
            fa.pack()
            tag = f"actor {h1}x{h2} {act}"
            out[f"{tag} image"] = _digest(fa.packed)
            for n in ROWS:
                mean, a = torch.zeros(n, 4, device="cuda"), torch.zeros(n, 4, device="cuda")
                fa.act(obs12[:n].contiguous(), a, mean)
                out[f"{tag} act n={n}"] = _digest(mean, a)
            for (kind, wrapper), (e, start) in envs.items():
                for mode in ("env", "deployed"):
                    e.set_state(**start)
                    res = fa.episode(e, max_steps=STEPS, obs_mode=mode, trace_envs=TRACE)
                    out[f"{tag} episode {kind} {wrapper} {mode}"] = _run_digest(res, e)
            e, start = envs[("hover", "RateControlWrapper")]
            for mode in ("env", "deployed"):
                e.set_state(**start)
                course = WaypointCourse([make_trajectory("eight", spacing=0.5)], ENVS, 0.25, "cuda:0")
                course.begin(e)
                res = fa.waypoints(e, course, max_steps=STEPS, obs_mode=mode, trace_envs=TRACE)
                out[f"{tag} waypoints {mode}"] = _digest(_run_digest(res, e).encode(),
                                                         *[v for _, v in sorted(course.tracker.items())])
    for e, _ in envs.values():
        e.close()

    # ---- the Brax-profile policy
    envs = {k: fresh(k, None) for k in ("brax_hover", "brax_jax_mjx")}
    mean = torch.tensor([0, 0, 1, 1, 0, 0, 0] + [0.0] * 14)
    std = torch.tensor([0.02] * 7 + [100.0] * 4 + [0.05] * 6 + [100.0] * 4)
    for h1, h2 in NETS:
        for act in ("relu", "tanh", "silu"):
            torch.manual_seed(0)
            net = BraxActorCritic(21, 4, BraxPPOConfig(policy_hidden_sizes=(h1, h2), activation=act))
            with torch.no_grad():
                k, b = net.policy.kernels[2], net.policy.biases[2]
                k.mul_(0.1)
                b.copy_(torch.tensor([math.atanh(2.0 * 0.2227 * 9.81 / 52.0 - 1.0), 0, 0, 0, -2.0, -2.0, -2.0, -2.0]))
            fb = FusedBraxActor(net.cuda(), dict(mean=mean.cuda(), std=std.cuda()))
            fb.pack()
            tag = f"brax {h1}x{h2} {act}"
            out[f"{tag} image"] = _digest(fb.packed)
            for n in ROWS:
                for det in (True, False):
                    lg, a = torch.zeros(n, 8, device="cuda"), torch.zeros(n, 4, device="cuda")
                    fb.act(obs21[:n].contiguous(), a, lg, deterministic=det, seed=7, env_id_base=11, noise_step=3)
                    out[f"{tag} act n={n} {'det' if det else 'sampled'}"] = _digest(lg, a)
            for kind, (e, start) in envs.items():
                for det in (True, False):
                    e.set_state(**start)
                    res = fb.episode(e, max_steps=STEPS, deterministic=det, seed=3, trace_envs=TRACE, noise_step0=2)
                    out[f"{tag} episode {kind} {'det' if det else 'sampled'}"] = _run_digest(res, e)
    for e, _ in envs.values():
        e.close()
    torch.cuda.synchronize()
    print("DIGESTS " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--out", default=None, help="also write {library, digests} as JSON")
    ap.add_argument("--timeout", type=float, default=540.0, help="seconds for the child process")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child()
        return 0
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True,
                       timeout=a.timeout)
    line = next((l for l in r.stdout.splitlines() if l.startswith("DIGESTS ")), None)
    if r.returncode != 0 or line is None:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"the digest run failed (exit {r.returncode})")
    digests = json.loads(line[8:])
    lib = os.environ.get("QUADENV_LIB", "in-tree build")
    print(f"== {lib}: {len(digests)} digests")
    for k, v in digests.items():
        print(f"{k:55s} {v}")
    print("ALL " + hashlib.sha256(json.dumps(digests, sort_keys=True).encode()).hexdigest()[:16])
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"library": lib, "digests": digests}, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
