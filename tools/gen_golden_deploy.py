#!/usr/bin/env python3
"""Generate tests/golden/golden_deploy.npz from the reference's deployed observation path, run unmodified:
ros2_ws/src/rl_drone_control/rl_drone_control/state_estimator.py (VelocityEstimator) and
observation_builder.py (build_observation). Both need only numpy.

Like gen_golden.py this runs only where the reference tree is present; only the fixture it writes is
committed.

Fixture contents
  (a) est_*: 600 VelocityEstimator.update calls per alpha of ALPHAS, state carried within runs of RUN
      calls (a fresh estimator per run). update() is handed the float32 position words as float64 arrays
      (gen_golden_pid.py's convention) and timestamps k * 0.01. Some runs hold a repeated timestamp
      (dt = 0) and a gap above max_dt, so both reset branches are recorded beside the first-call one.
      Recorded per call: pos, t, the returned velocity, and the estimator's state after the call
      (prev_pos 3, prev_time, velocity 3, has_prev).
  (b) obs_*: 600 build_observation calls: drone_pos, target_pos, attitude, linear_vel (float64, as the
      estimator returns it), angular_vel and the returned observation. A third of the components lie
      outside their bounds, some exactly on a bound. Position and target components are 0 or at least
      2^-20 in magnitude and at most 16, so the builder's float64 difference rounded to float32 equals
      the float32 difference of the product's law (the difference of two such float32 values is exact in
      float64, and one rounding of the exact value is what float32 subtraction returns).

Usage:  python tools/gen_golden_deploy.py  [--out tests/golden]
"""
from __future__ import annotations

import argparse
import importlib.util
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as GG  # noqa: E402  (where the reference lives)

ALPHAS = (0.0, 0.1, 0.5, 0.8, 0.95)
RUN = 50
CALLS = 600
MAX_DT = 0.1
PKG = os.path.join("ros2_ws", "src", "rl_drone_control", "rl_drone_control")


def _load(name: str):
    path = os.path.join(GG.REF, PKG, name + ".py")
    if not os.path.exists(path):
        raise SystemExit(f"gen_golden_deploy.py needs the reference tree ({path})")
    sys.dont_write_bytecode = True
    spec = importlib.util.spec_from_file_location("ref_" + name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _grid(rng, n, lo, hi):
    """float32 values in [lo, hi], each 0 or at least 2^-20 in magnitude."""
    x = rng.uniform(lo, hi, n).astype(np.float32)
    x[np.abs(x) < 2.0 ** -20] = 0.0
    return x


def estimator_calls(SE, rng) -> dict:
    out = {}
    n_runs = CALLS // RUN
    pos = np.zeros((CALLS, 3), np.float32)
    ts = np.zeros(CALLS, np.float64)
    for r in range(n_runs):
        p = _grid(rng, 3, -2.0, 2.0)
        k = int(rng.integers(0, 400))
        for j in range(RUN):
            i = r * RUN + j
            p = (p + rng.normal(0.0, 0.02, 3)).astype(np.float32)
            p[np.abs(p) < 2.0 ** -20] = 0.0
            if j > 0:
                k += 1
                if r % 3 == 1 and j == 17:
                    k -= 1      # a repeated timestamp: dt = 0
                if r % 3 == 2 and j == 23:
                    k += 11     # a gap of 0.12 s > max_dt
                if r % 4 == 3 and j == 31:
                    k += 9      # a gap of exactly 10 steps (0.1 s up to rounding): the boundary compare
            pos[i] = p
            ts[i] = k * 0.01
    out["est_pos"], out["est_t"] = pos, ts
    out["est_alphas"] = np.array(ALPHAS, np.float64)
    out["est_max_dt"] = np.float64(MAX_DT)
    out["est_run"] = np.int32(RUN)
    vel = np.zeros((len(ALPHAS), CALLS, 3), np.float64)
    state = np.zeros((len(ALPHAS), CALLS, 8), np.float64)
    for a, alpha in enumerate(ALPHAS):
        for i in range(CALLS):
            if i % RUN == 0:
                est = SE.VelocityEstimator(alpha=alpha, max_dt=MAX_DT)
            v = est.update(pos[i].astype(np.float64), float(ts[i]))
            vel[a, i] = v
            state[a, i, 0:3] = est._prev_pos
            state[a, i, 3] = est._prev_time
            state[a, i, 4:7] = est._velocity
            state[a, i, 7] = 1.0
    out["est_vel"], out["est_state"] = vel, state
    return out


def builder_calls(OB, rng) -> dict:
    lo, hi = OB.OBS_BOUNDS_LOW.astype(np.float64), OB.OBS_BOUNDS_HIGH.astype(np.float64)
    n = CALLS
    # the raw 12 components; a third outside their bounds, some exactly on one
    raw = np.zeros((n, 12), np.float64)
    for j in range(12):
        x = rng.uniform(lo[j], hi[j], n)
        outside = rng.random(n) < 1.0 / 3.0
        x[outside] = np.where(rng.random(outside.sum()) < 0.5, lo[j] - rng.uniform(0.0, 1.0, outside.sum()) * (hi[j] - lo[j]),
                              hi[j] + rng.uniform(0.0, 1.0, outside.sum()) * (hi[j] - lo[j]))
        on = rng.random(n) < 0.04
        x[on] = np.where(rng.random(on.sum()) < 0.5, lo[j], hi[j])
        raw[:, j] = x
    target = np.stack([_grid(rng, n, -2.0, 2.0) for _ in range(3)], axis=1)
    # drone_pos so that target - drone_pos is (about) the wanted relative position, on the same grid
    drone = (target.astype(np.float64) - raw[:, 0:3]).astype(np.float32)
    drone[np.abs(drone) < 2.0 ** -20] = 0.0
    on_rel = rng.random(n) < 0.04  # relative position exactly on a bound: target at +-2, the drone at -+2 (or 0)
    for i in np.nonzero(on_rel)[0]:
        s = 1.0 if rng.random() < 0.5 else -1.0
        target[i, 0:2] = 2.0 * s
        drone[i, 0:2] = -2.0 * s
        target[i, 2] = 2.0 * s
        drone[i, 2] = 0.0
    att = raw[:, 3:6].astype(np.float32)
    ang = raw[:, 9:12].astype(np.float32)
    vel = raw[:, 6:9].copy()  # float64: the estimator's return type
    obs = np.zeros((n, 12), np.float32)
    for i in range(n):
        obs[i] = OB.build_observation(drone[i].astype(np.float64), target[i].astype(np.float64), att[i].astype(np.float64),
                                      vel[i], ang[i].astype(np.float64))
    assert obs.dtype == np.float32
    return {"obs_drone_pos": drone, "obs_target": target, "obs_attitude": att, "obs_linear_vel": vel,
            "obs_angular_vel": ang, "obs_out": obs,
            "obs_low": OB.OBS_BOUNDS_LOW.astype(np.float32), "obs_high": OB.OBS_BOUNDS_HIGH.astype(np.float32)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(GG.REPO, "tests", "golden"))
    a = ap.parse_args()
    SE, OB = _load("state_estimator"), _load("observation_builder")
    rng = np.random.default_rng(20240516)
    d = estimator_calls(SE, rng)
    d.update(builder_calls(OB, rng))
    path = os.path.join(a.out, "golden_deploy.npz")
    np.savez_compressed(path, **d)
    clipped = float(np.mean(np.abs(d["obs_out"]) == 1.0))
    print(f"wrote {path} ({os.path.getsize(path)} bytes); {100 * clipped:.1f}% of the observation components at +-1")


if __name__ == "__main__":
    main()
