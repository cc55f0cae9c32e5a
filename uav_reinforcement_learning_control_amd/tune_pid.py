"""Population tuner for the cascaded PID baseline (the reference's auto_tune_pid.py, batched).

The reference evaluates one candidate gain set on five episodes per iteration and nudges it by rule.
Here one fused launch (``quad_pid_episode``) flies every candidate of a generation on the same
episodes: candidates x episodes envs, candidate-major, so a wave's lanes share a gain set. The
search moves the six quantities the reference's tuner moves, inside its clamps
(auto_tune_pid.py:211-219): yaw kp and kd, yaw torque scale, rate ki, and xy and z kp; the score is
its ``compute_performance_score`` averaged over the episodes.

  * Candidate 0 of the first generation is the starting gain set; each later generation carries the
    best so far forward as its candidate 0, so the best tuning score never decreases.
  * Candidates are drawn log-normally around the current elites, the spread shrinking by generation.
  * After the last generation the top few candidates (those that did not score below the starting
    gains on the tuning episodes) are re-scored on a fresh, larger set of episodes; that fresh score
    is the one reported, so it is not biased upward by the selection on the tuning episodes.

HoverEnv only: every candidate must fly the same start states and targets, which are copied into
the envs; the trajectory kind's spline is tied to each env's own reset draw.

    python -m uav_reinforcement_learning_control_amd.tune_pid --out pid_gains_tuned.json

``--law se3 | smc | lqr`` runs the same search on one of the other controllers (``quad_ctrl_episode``): the six
searched quantities are gains all laws share, the law's own parameters (the LQR row, the super-twisting
constants, ``se3_reorthonormalize``) stay at the starting set's values. The default is the PID.
"""
from __future__ import annotations

import argparse
import time
from typing import Optional

import numpy as np
import torch

from . import _native as N
from .controllers import (CtrlParams, PIDGains, ctrl_episode, gains_from_vector, params_from_vector, pid_episode,
                          pid_score)
from .envs import QuadVecEnv

# (QuadPidGains field, low, high): auto_tune_pid.py:211-219
SEARCH = (("kp_yaw", 10.0, 80.0), ("kd_yaw", 5.0, 30.0), ("yaw_torque_scale", 0.2, 0.8),
          ("ki_rate_torque", 0.01, 0.04), ("kp_xy", 1.5, 4.0), ("kp_z", 2.0, 6.0))
_COLS = [N.PID_GAIN_FIELDS.index(f) for f, _, _ in SEARCH]
_LO = np.array([lo for _, lo, _ in SEARCH])
_HI = np.array([hi for _, _, hi in SEARCH])


class _Arena:
    """candidates x episodes hover envs that fly the same `episodes` resets for every candidate."""

    def __init__(self, candidates: int, episodes: int, seed: int, max_episode_steps: Optional[int], device,
                 law: str = "pid"):
        self.law = law
        src = QuadVecEnv(episodes, device=device, seed=seed, max_episode_steps=max_episode_steps, auto_reset=False)
        src.reset()
        st = src.get_state()
        src.close()
        self.c, self.e = candidates, episodes
        self.env = QuadVecEnv(candidates * episodes, device=device, seed=seed, max_episode_steps=max_episode_steps,
                              auto_reset=False)
        # candidate-major: env c * episodes + e starts from reset e
        self.start = {k: np.tile(v, (candidates,) + (1,) * (v.ndim - 1)) for k, v in st.items()}
        self.set_of = torch.arange(candidates, device=self.env.device, dtype=torch.int32).repeat_interleave(episodes)

    def scores(self, table: np.ndarray) -> np.ndarray:
        """Mean total_score of each candidate (rows of `table`, [candidates, 22]; 33 for the other laws) over
        the episodes."""
        self.env.set_state(**self.start)
        if self.law == "pid":
            m = pid_episode(self.env, table, set_of=self.set_of)
        else:
            m = ctrl_episode(self.env, table, set_of=self.set_of, law=self.law)
        return pid_score(m)["total_score"].reshape(self.c, self.e).mean(dim=1).cpu().numpy()

    def close(self):
        self.env.close()


def _population(rng: np.random.Generator, base: np.ndarray, elites: np.ndarray, n: int, sigma: float) -> np.ndarray:
    """[n, 22]: row 0 = elites[0] (carried forward); the others log-normal around elites, in turn."""
    pop = np.tile(base, (n, 1))
    pop[0, _COLS] = elites[0]
    for i in range(1, n):
        x = elites[(i - 1) % len(elites)] * np.exp(sigma * rng.standard_normal(len(_COLS)))
        pop[i, _COLS] = np.clip(x, _LO, _HI)
    return pop


def tune(start: Optional[PIDGains] = None, candidates: int = 4096, episodes: int = 16, generations: int = 8,
         n_elites: int = 8, final_top: int = 8, final_episodes: Optional[int] = None, sigma: float = 0.35,
         max_episode_steps: Optional[int] = None, seed: int = 0, device="cuda", out: Optional[str] = None,
         verbose: bool = False, law: str = "pid") -> dict:
    """Returns {"gains": PIDGains, "tuning_score", "start_tuning_score", "fresh_score",
    "fresh_start_score", "history" (best tuning score per generation), "seconds"}; writes `out` in
    pid_gains.json's layout when given. The starting gains are clamped into the search box first."""
    if candidates < 1 or episodes < 1 or generations < 1:
        raise ValueError("candidates, episodes and generations must be >= 1")
    if law not in ("pid", "se3", "smc", "lqr"):
        raise ValueError("law must be pid, se3, smc or lqr")
    t0 = time.perf_counter()
    if law == "pid":
        start = start or PIDGains()
    else:  # the 33-number parameter set; its first 22 columns are the PID's, so _COLS holds
        start = start if isinstance(start, CtrlParams) else CtrlParams(**vars(start or PIDGains()))
    base = start.vector()
    base[_COLS] = np.clip(base[_COLS], _LO, _HI)
    rng = np.random.default_rng(seed)
    arena = _Arena(candidates, episodes, seed, max_episode_steps, device, law)
    elites = base[_COLS][None, :]
    history, start_score, pop, sc = [], None, None, None
    for g in range(generations):
        pop = _population(rng, base, elites, candidates, sigma * (0.7 ** g))
        sc = arena.scores(pop)
        if g == 0:
            start_score = float(sc[0])
        order = np.argsort(-sc, kind="stable")  # ties: the lower index, so the carried best stays
        elites = pop[order[:max(1, min(n_elites, candidates))]][:, _COLS]
        history.append(float(sc[order[0]]))
        if verbose:
            print(f"generation {g + 1}/{generations}: best {history[-1]:.4f} (start {start_score:.4f})")
    arena.close()
    # fresh, larger episodes for the top few that did not fall below the start on the tuning set
    order = np.argsort(-sc, kind="stable")
    top = [i for i in order[:max(1, final_top)] if sc[i] >= start_score]
    fe = int(final_episodes or 16 * episodes)
    fin = np.concatenate([pop[top], base[None, :]])
    fresh = _Arena(len(fin), fe, seed + 1, max_episode_steps, device, law)
    fs = fresh.scores(fin)
    fresh.close()
    k = int(np.argmax(fs[:-1]))
    best = gains_from_vector(fin[k]) if law == "pid" else params_from_vector(fin[k])
    res = {"gains": best, "tuning_score": float(sc[top[k]]), "start_tuning_score": start_score,
           "fresh_score": float(fs[k]), "fresh_start_score": float(fs[-1]), "history": history,
           "candidates": candidates, "episodes": episodes, "fresh_episodes": fe,
           "seconds": time.perf_counter() - t0}
    if out:
        best.to_json(out, notes={"auto_tuning": {"generations": generations, "candidates": candidates,
                                                 "episodes": episodes, "score": res["fresh_score"],
                                                 "score_episodes": fe, "start_score": res["fresh_start_score"]}})
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--gains", default=None, help="starting pid_gains.json (default: the reference's gains)")
    ap.add_argument("--out", default="pid_gains_tuned.json")
    ap.add_argument("--candidates", type=int, default=4096)
    ap.add_argument("--episodes", type=int, default=16)
    ap.add_argument("--generations", type=int, default=8)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--law", default="pid", choices=["pid", "se3", "smc", "lqr"],
                    help="the controller whose shared gains are tuned (default: the PID)")
    ap.add_argument("--se3-reorthonormalize", type=int, choices=[0, 1], default=1,
                    help="--law se3: 0 skips the np.linalg.qr step, with which the controller does not hover")
    a = ap.parse_args(argv)
    start = (PIDGains if a.law == "pid" else CtrlParams).from_json(a.gains) if a.gains else None
    if a.law == "se3":
        start = start or CtrlParams()
        start.se3_reorthonormalize = float(a.se3_reorthonormalize)
    r = tune(start, a.candidates, a.episodes, a.generations, seed=a.seed, out=a.out, verbose=True, law=a.law)
    print(f"score on {r['fresh_episodes']} fresh episodes: {r['fresh_score']:.4f} (starting gains "
          f"{r['fresh_start_score']:.4f}); tuning score {r['tuning_score']:.4f} (start {r['start_tuning_score']:.4f}); "
          f"{r['seconds']:.1f} s\nwrote {a.out}")
    return r


if __name__ == "__main__":
    main()
