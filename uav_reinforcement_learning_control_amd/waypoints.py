"""Waypoint courses for the lap evaluators (evaluate.py:440-612 evaluate_trajectory, batched).

``WaypointCourse`` owns what the native lap calls read and write: the float64 waypoint table
([n_sets, max_points, 3] + counts), the env -> set map and the per-env tracker arrays (wp_idx, reached,
laps, steps, status, total_reward). ``begin`` places every env on its first waypoint
(``quad_waypoints_begin``); ``update`` is one ``quad_waypoints_update`` of the per-step loop; the fused
launches (``controllers.ctrl_waypoints``, ``FusedPolicy.waypoints``) take the course's ``run`` struct.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from . import _native as N

TRACKER_FIELDS = ("wp_idx", "reached", "laps", "steps", "status", "total_reward")
STATUS = {0: "running", 1: "lap", 2: "terminated", 3: "max steps"}


class WaypointCourse:
    """`sets`: float64 [n_k, 3] arrays; env i follows sets[set_of[i]] (default i % len(sets))."""

    def __init__(self, sets: Sequence, n: int, reach_radius: float = 0.25, device="cuda", set_of=None):
        self.device = torch.device(device)
        self.n = int(n)
        sets = [np.asarray(p, np.float64).reshape(-1, 3) for p in sets]
        if not sets or min(len(p) for p in sets) < 1:
            raise ValueError("every waypoint set needs at least one point")
        self.max_points = max(len(p) for p in sets)
        pts = np.zeros((len(sets), self.max_points, 3), np.float64)
        for k, p in enumerate(sets):
            pts[k, :len(p)] = p
        self.points = torch.from_numpy(pts).to(self.device)
        self.counts = torch.tensor([len(p) for p in sets], dtype=torch.int32, device=self.device)
        if set_of is None:
            set_of = torch.arange(self.n, dtype=torch.int32) % len(sets)
        so = torch.as_tensor(set_of).to(dtype=torch.int32)
        if tuple(so.shape) != (self.n,) or int(so.min()) < 0 or int(so.max()) >= len(sets):
            raise ValueError(f"set_of must have shape ({self.n},) and values in [0, {len(sets)})")
        self.set_of = so.to(self.device).contiguous()
        self.reach_radius = float(reach_radius)
        self.tracker = {k: torch.zeros(self.n, dtype=torch.float64 if k == "total_reward" else torch.int32,
                                       device=self.device) for k in TRACKER_FIELDS}

    def table(self, reach_radius: Optional[float] = None) -> N.QuadWaypoints:
        return N.QuadWaypoints(points=self.points.data_ptr(), counts=self.counts.data_ptr(),
                               set_of=self.set_of.data_ptr(), max_points=self.max_points,
                               reach_radius=self.reach_radius if reach_radius is None else float(reach_radius))

    def state(self) -> N.QuadWaypointState:
        return N.QuadWaypointState(**{k: v.data_ptr() for k, v in self.tracker.items()})

    def run(self, trace_reward: Optional[torch.Tensor] = None, trace_wp_idx: Optional[torch.Tensor] = None):
        return N.QuadWaypointRun(w=self.table(), s=self.state(),
                                 trace_reward=None if trace_reward is None else trace_reward.data_ptr(),
                                 trace_wp_idx=None if trace_wp_idx is None else trace_wp_idx.data_ptr())

    def begin(self, env, obs: Optional[torch.Tensor] = None) -> torch.Tensor:
        """quad_waypoints_begin (call env.reset() first): returns the first observation [N, obs_dim]."""
        if env.num_envs != self.n:
            raise ValueError(f"the course is for {self.n} envs, the env has {env.num_envs}")
        obs = torch.zeros(self.n, env.obs_dim, device=self.device) if obs is None else obs
        # the start reads no radius; quad_waypoints_begin asks for a positive one
        w, st = self.table(self.reach_radius if self.reach_radius > 0 else 1.0), self.state()
        N.check(N.lib().quad_waypoints_begin(env._h, C.byref(w), C.byref(st), C.c_void_p(obs.data_ptr()),
                                             env._stream()), "quad_waypoints_begin")
        return obs

    def update(self, env, state12, reward, terminated, truncated) -> None:
        """quad_waypoints_update after one env.step of the per-step loop."""
        w, st = self.table(), self.state()
        N.check(N.lib().quad_waypoints_update(env._h, C.byref(w), C.byref(st), C.c_void_p(state12.data_ptr()),
                                              C.c_void_p(reward.data_ptr()), C.c_void_p(terminated.data_ptr()),
                                              C.c_void_p(truncated.data_ptr()), env._stream()),
                "quad_waypoints_update")

    def result(self) -> dict:
        """The tracker arrays on the host."""
        return {k: v.cpu().numpy() for k, v in self.tracker.items()}


__all__ = ["WaypointCourse", "TRACKER_FIELDS", "STATUS"]
