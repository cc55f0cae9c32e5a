"""The rollout policy as MFMA kernels (csrc/policy.hip via quad_policy_pack / quad_policy_act /
quad_rollout_post), bound to a torch ActorCritic.

One rollout step of SB3 OnPolicyAlgorithm.collect_rollouts (the learner the reference's
train.py:50-68 configures) becomes three launches -- policy (both MLPs on MFMA, Gaussian sample,
log-prob, clip, buffer rows), env step, epilogue (TimeLimit bootstrap, episode_starts, Monitor
statistics) -- instead of ~25 torch kernels. The torch ActorCritic stays the trained model;
`pack()` refreshes the kernels' copy of its parameters (call it after each update).

`FusedPolicy` is the 12-128-128 ReLU net of the training kernels. `FusedActor` is the deterministic actor of any
other supported architecture (quad_actor_*: 12-H1-H2-4, ReLU or tanh) for evaluation episodes and waypoint laps;
`fused_actor_for(policy)` picks between the two. `FusedActorCritic` is the rollout policy of that family (policy and
value net, quad_actor_critic_* / quad_actor_rollout) behind FusedPolicy's interface; `fused_policy_for(policy)` picks
between it and `FusedPolicy`. `FusedBraxActor` is the Brax profile's policy (quad_brax_*:
21-H1-H2-8 behind the running statistics, ReLU / tanh / SiLU, NormalTanh sampling) for evaluation episodes of the
brax env kinds and for the learner's unrolls (sample, unroll). `FusedBraxLearner` is the Brax profile's minibatch
gradient and Adam step (quad_brax_ppo_grad, quad_clip_adam) for (128, 128) ReLU policy and value nets;
`FusedBraxArchLearner` is the same for every two-hidden-layer net of the Brax actor's family (quad_brax_ppo_arch_grad),
and `fused_brax_learner_for` chooses between them.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from .. import _native as N
from .policy import ActorCritic


def _p(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _need(t: torch.Tensor, shape, dtype, dev, name):
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous() or t.device != dev:
        raise ValueError(f"{name}: expected contiguous {dtype} {tuple(shape)} on {dev}, got "
                         f"{t.dtype} {tuple(t.shape)} on {t.device}")


def _ordered(policy: ActorCritic):
    """The parameters in QuadPolicyParams' (and QuadPolicyGrads') field order."""
    ex = policy.mlp_extractor
    return [ex.policy_net[0].weight, ex.policy_net[0].bias, ex.policy_net[2].weight, ex.policy_net[2].bias,
            policy.action_net.weight, policy.action_net.bias,
            ex.value_net[0].weight, ex.value_net[0].bias, ex.value_net[2].weight, ex.value_net[2].bias,
            policy.value_net.weight, policy.value_net.bias, policy.log_std]


def current_stream(device) -> C.c_void_p:
    """torch's current stream of `device`, as the entry points take it."""
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class Workspace:
    """A grow-only uint8 device buffer for a kernel family's scratch. reserve() replaces the allocation when more
    bytes are needed, so a hipGraph that captured a launch is keyed on (ptr, nbytes), which the launch took."""

    def __init__(self, device):
        self.device, self.buf, self.ptr, self.nbytes = device, None, 0, 0

    def reserve(self, nbytes: int) -> None:
        if self.nbytes < nbytes:
            self.buf = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
            self.ptr, self.nbytes = self.buf.data_ptr(), int(nbytes)


def _episode_run(env, dev, T: int, M: int, obs_mode, alpha, alpha_all, max_dt, est_state, laps: bool):
    """The result tensors and the QuadPolicyRun of one fused episode / lap launch (FusedPolicy.episode's rules)."""
    n = env.num_envs
    res = {k: torch.zeros(n, dtype=getattr(torch, dt), device=dev) for k, dt in N.PID_METRIC_FIELDS}
    res["vel_err_sq"] = torch.zeros(n, dtype=torch.float64, device=dev)
    if M > 0 and T > 0:
        for k, w in (("actions", 4), ("obs", 12), ("state12", 12), ("vel_est", 3)):
            res[k] = torch.zeros(T, M, w, dtype=torch.float32, device=dev)
        if laps:
            res["rewards"] = torch.zeros(T, M, dtype=torch.float32, device=dev)
            res["flown_wp"] = torch.zeros(T, M, dtype=torch.int32, device=dev)
    if alpha is not None:
        alpha = torch.as_tensor(alpha, dtype=torch.float64, device=dev).contiguous()
        _need(alpha, (n,), torch.float64, dev, "alpha")
    if est_state is not None:
        _need(est_state, (N.EST_NSTATE, n), torch.float64, dev, "est_state")
    tr = lambda k: res[k].data_ptr() if k in res else None
    run = N.QuadPolicyRun(obs_mode=N.OBS_MODES[obs_mode], max_steps=T, trace_envs=M,
                          est=N.QuadVelEst(alpha=_p(alpha), alpha_all=float(alpha_all), max_dt=float(max_dt),
                                           state=_p(est_state)),
                          est_dt=float(env.dt), trace_actions=tr("actions"), trace_state12=tr("state12"),
                          trace_obs=tr("obs"), trace_vel_est=tr("vel_est"),
                          metrics=N.QuadPidMetrics(**{k: res[k].data_ptr() for k, _ in N.PID_METRIC_FIELDS}),
                          vel_err_sq=res["vel_err_sq"].data_ptr())
    run._keep = (alpha, est_state)  # the launch reads them: alive as long as the descriptor
    return res, run


class FusedPolicy:
    """Packed fp32 image of an ActorCritic (12 -> 128 -> 128 -> 4 / 1) for the MFMA kernels."""

    @staticmethod
    def _check_shapes(policy: ActorCritic) -> None:
        ex = policy.mlp_extractor
        shapes = [tuple(l.weight.shape) for l in (ex.policy_net[0], ex.policy_net[2], ex.value_net[0],
                                                  ex.value_net[2], policy.action_net, policy.value_net)]
        if shapes != [(128, 12), (128, 128), (128, 12), (128, 128), (4, 128), (1, 128)]:
            raise ValueError(f"the MFMA policy kernels are built for 12-128-128-(4|1) nets, got {shapes}")
        if getattr(policy, "activation", "relu") != "relu":
            raise ValueError(f"the MFMA policy kernels are built for ReLU nets, got {policy.activation!r}")

    def __init__(self, policy: ActorCritic):
        self._check_shapes(policy)
        self.policy = policy
        self.device = policy.log_std.device
        if self.device.type != "cuda":
            raise N.QuadError("FusedPolicy needs the policy on a ROCm GPU")
        L = N.lib()
        self.packed = torch.empty(L.quad_policy_packed_floats(), dtype=torch.float32, device=self.device)

    @torch.no_grad()
    def pack(self) -> None:
        ts = _ordered(self.policy)
        for t in ts:
            if not t.is_contiguous() or t.dtype != torch.float32:
                raise ValueError("policy parameters must be contiguous float32")
        prm = N.QuadPolicyParams(*[t.data_ptr() for t in ts])
        N.check(N.lib().quad_policy_pack(C.byref(prm), _p(self.packed), current_stream(self.device)),
                "quad_policy_pack")

    def act(self, obs: torch.Tensor, actions_env: torch.Tensor, *, actions=None, log_prob=None,
            value=None, obs_copy=None, last_start=None, episode_starts=None,
            cursor: Optional[torch.Tensor] = None, rows: int = 1, seed: int = 0,
            env_id_base: int = 0, deterministic: bool = False,
            epilogue: Optional[N.QuadRolloutPost] = None) -> None:
        """quad_policy_act: row buffers are [rows, N, ...] (row t % rows, t = cursor[0]); with
        `epilogue` (from make_epilogue) the pending previous step is finished in the same launch
        and the cursor advances."""
        n, dev, f32 = obs.shape[0], self.device, torch.float32
        _need(obs, (n, 12), f32, dev, "obs")
        _need(actions_env, (n, 4), f32, dev, "actions_env")
        for t, shp, name in ((actions, (rows, n, 4), "actions"), (log_prob, (rows, n), "log_prob"),
                             (value, (rows, n), "value"), (obs_copy, (rows, n, 12), "obs_copy"),
                             (last_start, (n,), "last_start"), (episode_starts, (rows, n), "episode_starts")):
            if t is not None:
                _need(t, shp, f32, dev, name)
        if cursor is not None:
            _need(cursor, (4,), torch.int32, dev, "cursor")
        a = N.QuadPolicyAct(obs=obs.data_ptr(), actions_env=actions_env.data_ptr(),
                            actions=_p(actions), log_prob=_p(log_prob), value=_p(value),
                            obs_copy=_p(obs_copy), last_start=_p(last_start),
                            episode_starts=_p(episode_starts), cursor=_p(cursor), rows=int(rows),
                            deterministic=int(bool(deterministic)), seed=int(seed) & (2**64 - 1),
                            env_id_base=int(env_id_base),
                            epilogue=C.pointer(epilogue) if epilogue is not None else None)
        self._launch_act(a, n)

    def _launch_act(self, a: N.QuadPolicyAct, n: int) -> None:
        N.check(N.lib().quad_policy_act(_p(self.packed), C.byref(a), n, current_stream(self.device)), "quad_policy_act")

    def _launch_post(self, epilogue: N.QuadRolloutPost, cursor: torch.Tensor) -> None:
        N.check(N.lib().quad_rollout_post(_p(self.packed), C.byref(epilogue), _p(cursor), epilogue._n,
                                          current_stream(self.device)), "quad_rollout_post")

    def _launch_rollout(self, env, r: N.QuadRollout) -> None:
        N.check(N.lib().quad_rollout(env._h, _p(self.packed), C.byref(r), current_stream(self.device)), "quad_rollout")

    def value(self, obs: torch.Tensor, out: torch.Tensor, scratch: torch.Tensor) -> torch.Tensor:
        """V(obs) [N] into out ([1, N]) on the MFMA kernel: per-row results do not depend on the
        batch (no GEMM tiling choice), so a rank's shard bootstraps exactly as in one process.
        `scratch` ([N, 4]) receives the deterministic actions."""
        self.act(obs, scratch, value=out, rows=1, deterministic=True)
        return out[0]

    def make_epilogue(self, reward, terminated, truncated, terminal_obs, buf_rew, last_start, ep_ret,
                      ep_len, stats, rows: int, gamma: float) -> N.QuadRolloutPost:
        """The QuadRolloutPost of a rollout (buffers are referenced, not copied: keep them alive)."""
        n, dev, f32 = reward.shape[0], self.device, torch.float32
        _need(reward, (n,), f32, dev, "reward")
        _need(terminated, (n,), torch.bool, dev, "terminated")
        _need(truncated, (n,), torch.bool, dev, "truncated")
        _need(terminal_obs, (n, 12), f32, dev, "terminal_obs")
        _need(buf_rew, (rows, n), f32, dev, "buf_rew")
        for t, name in ((last_start, "last_start"), (ep_ret, "ep_ret"), (ep_len, "ep_len")):
            _need(t, (n,), f32, dev, name)
        _need(stats, (N.POLICY_STAT_SLOTS, 3), torch.float64, dev, "stats")
        e = N.QuadRolloutPost(reward=reward.data_ptr(), terminated=terminated.data_ptr(),
                              truncated=truncated.data_ptr(), terminal_obs=terminal_obs.data_ptr(),
                              buf_rew=buf_rew.data_ptr(), last_start=last_start.data_ptr(),
                              ep_ret=ep_ret.data_ptr(), ep_len=ep_len.data_ptr(),
                              stats=stats.data_ptr(), rows=int(rows), gamma=float(gamma))
        e._n = n
        return e

    def post(self, epilogue: N.QuadRolloutPost, cursor: torch.Tensor) -> None:
        """quad_rollout_post: finish the pending step (end of a rollout)."""
        _need(cursor, (4,), torch.int32, self.device, "cursor")
        self._launch_post(epilogue, cursor)

    def rollout(self, env, **rollout) -> None:
        """quad_rollout: `steps` whole rollout steps (policy + env step + bootstrap + statistics)
        of `env` (a QuadVecEnv: hover/trajectory, no wrapper or RateControlWrapper, auto-reset) in
        one launch; step t = t0 + s writes row t % rows of the [rows, N, ...] buffers. Keyword arguments: obs_copy,
        actions, log_prob, value, episode_starts, rewards, last_obs, last_start, ep_ret, ep_len, stats, t0, steps,
        seed, gamma, deterministic = False."""
        self._rollout_with(self._launch_rollout, env, **rollout)

    def _rollout_with(self, launch, env, *, obs_copy, actions, log_prob, value, episode_starts, rewards, last_obs,
                      last_start, ep_ret, ep_len, stats, t0: int, steps: int, seed: int, gamma: float,
                      deterministic: bool = False) -> None:
        """rollout's checks and descriptor, handed to launch(env, QuadRollout)."""
        n, dev, f32 = env.num_envs, self.device, torch.float32
        rows = rewards.shape[0]
        for t, shp, name in ((obs_copy, (rows, n, 12), "obs_copy"), (actions, (rows, n, 4), "actions"),
                             (log_prob, (rows, n), "log_prob"), (value, (rows, n), "value"),
                             (episode_starts, (rows, n), "episode_starts"), (rewards, (rows, n), "rewards"),
                             (last_obs, (n, 12), "last_obs"), (last_start, (n,), "last_start"),
                             (ep_ret, (n,), "ep_ret"), (ep_len, (n,), "ep_len")):
            _need(t, shp, f32, dev, name)
        _need(stats, (N.POLICY_STAT_SLOTS, 3), torch.float64, dev, "stats")
        r = N.QuadRollout(obs_copy=obs_copy.data_ptr(), actions=actions.data_ptr(),
                          log_prob=log_prob.data_ptr(), value=value.data_ptr(),
                          episode_starts=episode_starts.data_ptr(), rewards=rewards.data_ptr(),
                          last_obs=last_obs.data_ptr(), last_start=last_start.data_ptr(),
                          ep_ret=ep_ret.data_ptr(), ep_len=ep_len.data_ptr(), stats=stats.data_ptr(),
                          rows=int(rows), t0=int(t0), steps=int(steps),
                          deterministic=int(bool(deterministic)), seed=int(seed) & (2**64 - 1),
                          gamma=float(gamma))
        launch(env, r)

    def episode(self, env, *, max_steps: Optional[int] = None, obs_mode="env", alpha=None, alpha_all: float = 0.8,
                max_dt: float = 0.1, trace_envs: int = 0, est_state: Optional[torch.Tensor] = None) -> dict:
        """quad_policy_episode: the deterministic policy's whole episodes from the envs' current state (call
        env.reset() first) in one launch. Every env runs to its first terminated / truncated step or
        `max_steps` (default: the env's max_episode_steps) and is then frozen, not reset. obs_mode "env": the
        policy sees the env's observation and the deployed velocity estimator runs beside it; "deployed": the
        policy sees what the reference's ROS2 node would feed it (estimated velocity, clipped). `alpha`: one
        low-pass coefficient per env ([N] float64) or None for `alpha_all`. Returns device tensors: the
        QuadPidMetrics fields and "vel_err_sq" ([N]); with trace_envs = M > 0 also "actions" [T, M, 4], "obs"
        and "state12" [T, M, 12] and "vel_est" [T, M, 3] of the first M envs (rows past an env's last step
        stay zero)."""
        res, run = _episode_run(env, self.device, int(env.max_episode_steps if max_steps is None else max_steps),
                                int(trace_envs), obs_mode, alpha, alpha_all, max_dt, est_state, laps=False)
        N.check(N.lib().quad_policy_episode(env._h, _p(self.packed), C.byref(run), current_stream(self.device)),
                "quad_policy_episode")
        return res

    def waypoints(self, env, course, *, max_steps: int = 5000, obs_mode="env", alpha=None, alpha_all: float = 0.8,
                  max_dt: float = 0.1, trace_envs: int = 0, est_state: Optional[torch.Tensor] = None) -> dict:
        """quad_policy_waypoints: the deterministic policy's waypoint laps on a hover `env` in one launch.
        `course`: a WaypointCourse after course.begin(env) (or an earlier run: the tracker carries on). Every env
        whose tracker status is 0 flies until it completes its lap, terminates, truncates or `max_steps` pass.
        obs_mode "env": the policy sees the step's own observation (one step stale after a switch, as the
        reference's loop has it); "deployed": the ROS2 node's observation, rebuilt with the new target. Returns
        episode()'s tensors (status PID_LAP where the lap was completed) and, with trace_envs = M > 0, also
        "rewards" [T, M] and "flown_wp" [T, M] (the waypoint each step flew toward). The tracker arrays are
        course.tracker."""
        res, run = _episode_run(env, self.device, int(max_steps), int(trace_envs), obs_mode, alpha, alpha_all, max_dt,
                                est_state, laps=True)
        wr = course.run(res.get("rewards"), res.get("flown_wp"))
        N.check(N.lib().quad_policy_waypoints(env._h, _p(self.packed), C.byref(run), C.byref(wr),
                      current_stream(self.device)), "quad_policy_waypoints")
        return res


class FusedActor:
    """The deterministic actor of an ActorCritic of any supported architecture (12 -> H1 -> H2 -> 4, H1 a multiple
    of 32 up to 512, H2 in {64, 128, 256}, ReLU or tanh) on the general MFMA actor (csrc/actor_arch.h, quad_actor_*):
    the forward path only -- act, whole episodes and waypoint laps in one launch. The critic is not packed."""

    @staticmethod
    def arch_of(policy) -> N.QuadActorArch:
        """The module's QuadActorArch; ValueError for a net outside the family."""
        net = policy.mlp_extractor.policy_net
        lin = [m for m in net if isinstance(m, torch.nn.Linear)]
        shapes = [tuple(l.weight.shape) for l in lin] + [tuple(policy.action_net.weight.shape)]
        act = getattr(policy, "activation", "relu")
        ok = (len(lin) == 2 and len(net) == 4 and shapes[0][1] == 12 and shapes[2] == (4, shapes[1][0])
              and shapes[1][1] == shapes[0][0] and shapes[0][0] % 32 == 0 and 32 <= shapes[0][0] <= N.ACTOR_MAX_H1
              and shapes[1][0] in N.ACTOR_H2 and act in N.ACTFNS)
        if not ok:
            raise ValueError("the general MFMA actor flies 12-H1-H2-4 nets (H1 a multiple of 32 up to 512, H2 in "
                             f"{N.ACTOR_H2}, relu / tanh), got {shapes} {act!r}")
        return N.QuadActorArch(h1=shapes[0][0], h2=shapes[1][0], activation=N.ACTFNS[act])

    def __init__(self, policy: ActorCritic):
        self.arch = self.arch_of(policy)
        self.policy = policy
        self.device = policy.log_std.device
        if self.device.type != "cuda":
            raise N.QuadError("FusedActor needs the policy on a ROCm GPU")
        nf = N.lib().quad_actor_packed_floats(C.byref(self.arch))
        if nf <= 0:
            raise N.QuadError("quad_actor_packed_floats rejected the architecture")
        self.packed = torch.empty(nf, dtype=torch.float32, device=self.device)

    @torch.no_grad()
    def pack(self) -> None:
        pol, net = self.policy, self.policy.mlp_extractor.policy_net
        ts = [net[0].weight, net[0].bias, net[2].weight, net[2].bias, pol.action_net.weight, pol.action_net.bias]
        for t in ts:
            if not t.is_contiguous() or t.dtype != torch.float32:
                raise ValueError("policy parameters must be contiguous float32")
        prm = N.QuadActorParams(*[t.data_ptr() for t in ts])
        N.check(N.lib().quad_actor_pack(C.byref(self.arch), C.byref(prm), _p(self.packed), current_stream(self.device)),
                "quad_actor_pack")

    def act(self, obs: torch.Tensor, actions_env: torch.Tensor, mean: Optional[torch.Tensor] = None, *,
            deterministic: bool = True) -> None:
        """quad_actor_act: actions_env = clip(mean(obs), -1, 1), and the mean itself into `mean` unless None."""
        if not deterministic:
            raise ValueError("FusedActor is the deterministic actor: sampling runs on FusedPolicy or in torch")
        n, dev, f32 = obs.shape[0], self.device, torch.float32
        _need(obs, (n, 12), f32, dev, "obs")
        _need(actions_env, (n, 4), f32, dev, "actions_env")
        if mean is not None:
            _need(mean, (n, 4), f32, dev, "mean")
        N.check(N.lib().quad_actor_act(C.byref(self.arch), _p(self.packed), _p(obs), _p(mean), _p(actions_env), n,
                                       current_stream(self.device)), "quad_actor_act")

    def episode(self, env, *, max_steps: Optional[int] = None, obs_mode="env", alpha=None, alpha_all: float = 0.8,
                max_dt: float = 0.1, trace_envs: int = 0, est_state: Optional[torch.Tensor] = None) -> dict:
        """quad_actor_episode: FusedPolicy.episode with this actor (the same arguments, the same tensors)."""
        res, run = _episode_run(env, self.device, int(env.max_episode_steps if max_steps is None else max_steps),
                                int(trace_envs), obs_mode, alpha, alpha_all, max_dt, est_state, laps=False)
        N.check(N.lib().quad_actor_episode(env._h, C.byref(self.arch), _p(self.packed), C.byref(run),
                      current_stream(self.device)), "quad_actor_episode")
        return res

    def waypoints(self, env, course, *, max_steps: int = 5000, obs_mode="env", alpha=None, alpha_all: float = 0.8,
                  max_dt: float = 0.1, trace_envs: int = 0, est_state: Optional[torch.Tensor] = None) -> dict:
        """quad_actor_waypoints: FusedPolicy.waypoints with this actor."""
        res, run = _episode_run(env, self.device, int(max_steps), int(trace_envs), obs_mode, alpha, alpha_all, max_dt,
                                est_state, laps=True)
        wr = course.run(res.get("rewards"), res.get("flown_wp"))
        N.check(N.lib().quad_actor_waypoints(env._h, C.byref(self.arch), _p(self.packed), C.byref(run), C.byref(wr),
                                             current_stream(self.device)), "quad_actor_waypoints")
        return res


_ARCH_ROLLOUT_FAMILY = ("the general MFMA rollout collects 12-H1-H2-(4|1) policy and value nets of the same widths "
                        f"(H1 a multiple of 32 up to 512, H2 in {N.ACTOR_H2}, relu / tanh)")


class FusedActorCritic(FusedPolicy):
    """Packed image of an ActorCritic of any member of the general actor's family (policy net 12 -> H1 -> H2 -> 4 and
    value net 12 -> H1 -> H2 -> 1 of the same widths and activation) for the rollout kernels of
    csrc/actor_rollout.hip (quad_actor_critic_* / quad_actor_rollout). FusedPolicy's interface and argument checks
    (pack, act, value, make_epilogue, post, rollout) on this family's launches. The forward-only launches (episode,
    waypoints) are FusedActor's."""

    @staticmethod
    def arch_of(policy) -> N.QuadActorArch:
        """The module's QuadActorArch, the value net's shapes checked too; ValueError outside the family."""
        try:
            arch = FusedActor.arch_of(policy)
            vnet = policy.mlp_extractor.value_net
            vlin = [m for m in vnet if isinstance(m, torch.nn.Linear)]
            shapes = [tuple(l.weight.shape) for l in vlin] + [tuple(policy.value_net.weight.shape)]
            ok = len(vlin) == 2 and len(vnet) == 4 and shapes == [(arch.h1, 12), (arch.h2, arch.h1), (1, arch.h2)]
        except (ValueError, AttributeError, IndexError, TypeError) as e:
            raise ValueError(f"{_ARCH_ROLLOUT_FAMILY}: {e}") from None
        if not ok:
            raise ValueError(f"{_ARCH_ROLLOUT_FAMILY}, got value net {shapes}")
        return arch

    def __init__(self, policy: ActorCritic):
        self.arch = self.arch_of(policy)
        self.policy = policy
        self.device = policy.log_std.device
        if self.device.type != "cuda":
            raise N.QuadError("FusedActorCritic needs the policy on a ROCm GPU")
        nf = N.lib().quad_actor_critic_packed_floats(C.byref(self.arch))
        if nf <= 0:
            raise N.QuadError("quad_actor_critic_packed_floats rejected the architecture")
        self.packed = torch.empty(nf, dtype=torch.float32, device=self.device)

    @torch.no_grad()
    def pack(self) -> None:
        ts = _ordered(self.policy)
        for t in ts:
            if not t.is_contiguous() or t.dtype != torch.float32:
                raise ValueError("policy parameters must be contiguous float32")
        prm = N.QuadPolicyParams(*[t.data_ptr() for t in ts])
        N.check(N.lib().quad_actor_critic_pack(C.byref(self.arch), C.byref(prm), _p(self.packed),
                                               current_stream(self.device)), "quad_actor_critic_pack")

    def _launch_act(self, a: N.QuadPolicyAct, n: int) -> None:
        N.check(N.lib().quad_actor_critic_act(C.byref(self.arch), _p(self.packed), C.byref(a), n,
                                              current_stream(self.device)), "quad_actor_critic_act")

    def _launch_post(self, epilogue: N.QuadRolloutPost, cursor: torch.Tensor) -> None:
        N.check(N.lib().quad_actor_critic_post(C.byref(self.arch), _p(self.packed), C.byref(epilogue), _p(cursor),
                                               epilogue._n, current_stream(self.device)), "quad_actor_critic_post")

    def _launch_rollout(self, env, r: N.QuadRollout) -> None:
        N.check(N.lib().quad_actor_rollout(env._h, C.byref(self.arch), _p(self.packed), C.byref(r),
                                           current_stream(self.device)), "quad_actor_rollout")

    def rollout_deployed(self, env, *, est_state: torch.Tensor, alpha=None, alpha_all: float = 0.8,
                         max_dt: float = 0.1, **rollout) -> None:
        """quad_actor_rollout_deployed: rollout() with the policy acting on the deployed observation (the velocity
        of the reference node's estimator, the row clipped to [-1, 1]). est_state float64 [8, N] holds the
        envs' estimators, read and written (start it with env.deploy_obs_rows after env.reset()); alpha float64 [N]
        or None for alpha_all; last_obs is the deployed row in hand. The other arguments are rollout()'s."""
        n, dev = env.num_envs, self.device
        _need(est_state, (N.EST_NSTATE, n), torch.float64, dev, "est_state")
        if alpha is not None:
            _need(alpha, (n,), torch.float64, dev, "alpha")
        est = N.QuadVelEst(alpha=_p(alpha), alpha_all=float(alpha_all), max_dt=float(max_dt), state=_p(est_state))
        L = N.need_deployed()
        launch = lambda e, r: N.check(L.quad_actor_rollout_deployed(e._h, C.byref(self.arch), _p(self.packed), C.byref(r),
                                                                    C.byref(est), float(e.dt),
                                                                    current_stream(self.device)),
                                      "quad_actor_rollout_deployed")
        self._rollout_with(launch, env, **rollout)

    def episode(self, *a, **k):
        raise NotImplementedError("FusedActorCritic collects rollouts; episodes fly on FusedActor (fused_actor_for)")

    waypoints = episode


def fused_policy_for(policy):
    """The fused rollout policy of `policy`: a FusedPolicy for the 12-128-128 ReLU net (its own kernels, the bits
    every existing path has), a FusedActorCritic for any other member of the family; ValueError naming the family
    outside it."""
    try:
        FusedPolicy._check_shapes(policy)
    except (ValueError, AttributeError, IndexError, TypeError):
        FusedActorCritic.arch_of(policy)
        return FusedActorCritic(policy)
    return FusedPolicy(policy)


# ((H1, H2), activation, num_envs) the drivers keep on the torch per-step rollout because the one-launch form did not
# beat it in profiles/arch_rollout/bench.json (by 19's to 23's rule)
ARCH_ROLLOUT_KEEP_TORCH = frozenset()


def arch_rollout_keeps_torch(hidden, activation: str, num_envs: int) -> bool:
    """Is this row in ARCH_ROLLOUT_KEEP_TORCH? The one place that forms the set's key (the driver asks before it
    builds the policy; arch_rollout_supported asks for a built one)."""
    return (tuple(int(x) for x in hidden), activation, int(num_envs)) in ARCH_ROLLOUT_KEEP_TORCH


def arch_rollout_supported(policy, env) -> bool:
    """The fused rollout of a net of the general family where quad_actor_rollout drives the env (rollout_supported),
    the policy and value nets are members, and the row is not in ARCH_ROLLOUT_KEEP_TORCH."""
    if not rollout_supported(env):
        return False
    try:
        arch = FusedActorCritic.arch_of(policy)
    except ValueError:
        return False
    return (policy.log_std.device.type == "cuda"
            and not arch_rollout_keeps_torch((arch.h1, arch.h2), getattr(policy, "activation", "relu"), env.num_envs))


def fused_actor_for(policy):
    """The fused forward of `policy`: a FusedPolicy for the 12-128-128 ReLU net (the specialised kernels, the bits
    every existing path has), a FusedActor for any other member of the family; ValueError outside it."""
    try:
        FusedPolicy._check_shapes(policy)
    except (ValueError, AttributeError, IndexError, TypeError):
        return FusedActor(policy)
    return FusedPolicy(policy)


def _net_supported(policy) -> bool:
    try:
        FusedPolicy._check_shapes(policy)
    except (ValueError, AttributeError, IndexError, TypeError):
        try:
            FusedActor.arch_of(policy)
        except (ValueError, AttributeError, IndexError, TypeError):
            return False
    return policy.log_std.device.type == "cuda"


def episode_supported(policy, env) -> bool:
    """quad_policy_episode / quad_actor_episode fly a 12-H1-H2-4 actor of the supported family (FusedActor; the
    12-128-128-4 ReLU net on its own kernels) on hover / trajectory envs (12-D obs), with or without
    RateControlWrapper; the handle's auto-reset setting does not matter."""
    cfg = getattr(env, "cfg", None)
    return (cfg is not None and getattr(env, "_h", None) is not None
            and cfg.env_kind in (N.ENV_HOVER, N.ENV_TRAJ) and cfg.wrapper in (N.WRAP_NONE, N.WRAP_CTBR)
            and _net_supported(policy))


def waypoints_supported(policy, env) -> bool:
    """quad_policy_waypoints / quad_actor_waypoints: episode_supported on a hover env (a switch overwrites the
    target register)."""
    return episode_supported(policy, env) and env.cfg.env_kind == N.ENV_HOVER


def rollout_supported(env) -> bool:
    """quad_rollout drives hover / trajectory envs (12-D obs) with SB3 auto-reset."""
    cfg = getattr(env, "cfg", None)
    return (cfg is not None and getattr(env, "_h", None) is not None and cfg.auto_reset == 1
            and cfg.env_kind in (N.ENV_HOVER, N.ENV_TRAJ) and cfg.wrapper in (N.WRAP_NONE, N.WRAP_CTBR))


def _brax_parts(net_or_params, activation=None, min_std=None):
    """([w0, b0, w1, b1, w2, b2], activation, min_std) of a BraxActorCritic, a BraxMLP, or a flax policy-params dict
    ({"params": {"hidden_i": {"kernel" [in, out], "bias"}}}); kernels stay in flax's [in, out] layout."""
    pol = getattr(net_or_params, "policy", net_or_params)
    if isinstance(pol, dict):
        p = pol.get("params", pol)
        names = sorted(p, key=lambda k: int(k.rsplit("_", 1)[1]))
        ts = [torch.as_tensor(p[k][f]) for k in names for f in ("kernel", "bias")]
        return ts, activation, min_std
    act = {v: k for k, v in _brax_act_table().items()}.get(pol.act, activation)
    ms = getattr(getattr(net_or_params, "dist", None), "min_std", min_std)
    return [t for k, b in zip(pol.kernels, pol.biases) for t in (k.detach(), b.detach())], act, ms


def _brax_act_table():
    from .brax_ppo import _ACT
    return _ACT


def brax_arch_of(policy_sizes, activation) -> N.QuadBraxActorArch:
    """The QuadBraxActorArch of hidden sizes (H1, H2) and an activation name; ValueError outside the family."""
    s = tuple(int(x) for x in policy_sizes)
    ok = (len(s) == 2 and s[0] % 32 == 0 and 32 <= s[0] <= N.ACTOR_MAX_H1 and s[1] in N.ACTOR_H2
          and activation in N.BRAX_ACTFNS)
    if not ok:
        raise ValueError("the MFMA Brax actor flies 21-H1-H2-8 nets (H1 a multiple of 32 up to 512, H2 in "
                         f"{N.ACTOR_H2}, relu / tanh / silu), got {s} {activation!r}")
    return N.QuadBraxActorArch(h1=s[0], h2=s[1], activation=N.BRAX_ACTFNS[activation])


def brax_episode_supported(policy_sizes, activation, env) -> bool:
    """quad_brax_episode flies a two-hidden-layer Brax policy of the supported family on a brax env kind."""
    cfg = getattr(env, "cfg", None)
    if cfg is None or getattr(env, "_h", None) is None or cfg.env_kind not in (N.ENV_BRAX_HOVER, N.ENV_BRAX_TRAJ):
        return False
    try:
        brax_arch_of(policy_sizes, activation)
    except (ValueError, TypeError):
        return False
    return True


# (hidden sizes, activation) the drivers keep on the per-step loop because the launch lost to it in
# profiles/brax_eval/bench.json (DESIGN 20's rule, 19's): none of the measured sizes did
BRAX_KEEP_LOOP = frozenset()


def brax_launch_chosen(policy_sizes, activation, env) -> bool:
    """The drivers' dispatch: the one-launch episode where it is supported and did not lose to the loop."""
    return (brax_episode_supported(policy_sizes, activation, env)
            and (tuple(int(x) for x in policy_sizes), activation) not in BRAX_KEEP_LOOP)


# (hidden sizes, activation) for which the launch did not beat the torch unroll loop in
# profiles/brax_unroll/bench.json (by 19's and 20's rule): it won every measured row
BRAX_UNROLL_KEEP_LOOP = frozenset()


def brax_unroll_supported(policy_sizes, activation, env) -> bool:
    """quad_brax_unroll collects the learner's unrolls where quad_brax_episode flies, on an env that resets itself;
    (sizes, activation) in BRAX_UNROLL_KEEP_LOOP stay on the torch loop."""
    return (brax_episode_supported(policy_sizes, activation, env) and env.cfg.auto_reset == 1
            and (tuple(int(x) for x in policy_sizes), activation) not in BRAX_UNROLL_KEEP_LOOP)


class FusedBraxActor:
    """The Brax-profile policy (ppo/brax_ppo.py BraxActorCritic.policy, two hidden layers) with its running-statistics
    normaliser on MFMA (csrc/brax_actor.h, quad_brax_*): act on observation rows, and whole evaluation episodes of a
    brax env kind in one launch.

    net_or_params: a BraxActorCritic / BraxMLP, or the flax policy-params dict of a saved archive (then give
    `activation`, and `min_std` if it is not 0.001). norm: a RunningStats, or a mapping with "mean" and "std"."""

    def __init__(self, net_or_params, norm, activation: Optional[str] = None, min_std: Optional[float] = None,
                 device=None):
        self.source, self.norm = net_or_params, norm
        ts, act, ms = _brax_parts(net_or_params, activation, min_std)
        if len(ts) != 6:
            raise ValueError(f"the MFMA Brax actor flies two hidden layers, got {len(ts) // 2 - 1}")
        if tuple(ts[0].shape)[0] != N.BRAX_OBS or tuple(ts[4].shape)[1] != N.BRAX_LOGITS:
            raise ValueError(f"expected a 21 -> .. -> 8 policy, got {[tuple(t.shape) for t in ts[::2]]}")
        self.arch = brax_arch_of((ts[0].shape[1], ts[2].shape[1]), act)
        self.min_std = 0.001 if ms is None else float(ms)
        self.device = torch.device(device) if device is not None else (
            ts[0].device if ts[0].device.type == "cuda" else torch.device("cuda", torch.cuda.current_device()))
        if self.device.type != "cuda":
            raise N.QuadError("FusedBraxActor needs a ROCm GPU")
        nf = N.lib().quad_brax_actor_packed_floats(C.byref(self.arch))
        if nf <= 0:
            raise N.QuadError("quad_brax_actor_packed_floats rejected the architecture")
        self.packed = torch.empty(nf, dtype=torch.float32, device=self.device)
        self._noise_step = 0

    def _mean_std(self):
        g = (lambda k: self.norm[k]) if isinstance(self.norm, dict) else (lambda k: getattr(self.norm, k))
        return g("mean"), g("std")

    @torch.no_grad()
    def pack(self) -> None:
        """Refresh the kernels' copy of the parameters and of the normaliser (call after an update)."""
        ts = _brax_parts(self.source)[0] + list(self._mean_std())
        ts = [torch.as_tensor(t).to(device=self.device, dtype=torch.float32).contiguous() for t in ts]
        prm = N.QuadBraxActorParams(*[t.data_ptr() for t in ts], min_std=self.min_std)
        N.check(N.lib().quad_brax_actor_pack(C.byref(self.arch), C.byref(prm), _p(self.packed),
                      current_stream(self.device)), "quad_brax_actor_pack")
        self._packed_from = ts  # the launch reads them: alive until the next pack

    def act(self, obs: torch.Tensor, actions_env: torch.Tensor, logits: Optional[torch.Tensor] = None, *,
            deterministic: bool = True, seed: int = 0, env_id_base: int = 0, noise_step: int = 0) -> None:
        """quad_brax_actor_act: actions_env = tanh(loc) or tanh(loc + scale z), and the logits unless None."""
        n, dev, f32 = obs.shape[0], self.device, torch.float32
        _need(obs, (n, N.BRAX_OBS), f32, dev, "obs")
        _need(actions_env, (n, 4), f32, dev, "actions_env")
        if logits is not None:
            _need(logits, (n, N.BRAX_LOGITS), f32, dev, "logits")
        N.check(N.lib().quad_brax_actor_act(C.byref(self.arch), _p(self.packed), _p(obs), _p(logits), _p(actions_env),
                                            n, int(bool(deterministic)), int(seed) & (2**64 - 1),
                                            int(env_id_base) & (2**64 - 1), int(noise_step) & 0xFFFFFFFF,
                                            current_stream(self.device)), "quad_brax_actor_act")

    def episode(self, env, *, max_steps: Optional[int] = None, deterministic: bool = False, seed: int = 0,
                trace_envs: int = 0, noise_step0: int = 0) -> dict:
        """quad_brax_episode: whole episodes from the envs' current state (call env.reset() first) in one launch.
        Every env runs to its first terminated / truncated step or `max_steps` (default: the env's episode length)
        and is then frozen, not reset. Returns device tensors: the QuadBraxMetrics fields ([N]) and, with
        trace_envs = M > 0, "actions" [T, M, 4], "obs" [T, M, 21], "pos" and "target" [T, M, 3] of the first M envs
        (rows past an env's last step stay zero)."""
        n, dev = env.num_envs, self.device
        T, M = int(env.max_episode_steps if max_steps is None else max_steps), int(trace_envs)
        res = {k: torch.zeros(n, dtype=getattr(torch, dt), device=dev) for k, dt in N.BRAX_METRIC_FIELDS}
        if M > 0 and T > 0:
            for k, w in (("actions", 4), ("obs", N.BRAX_OBS), ("pos", 3), ("target", 3)):
                res[k] = torch.zeros(T, M, w, dtype=torch.float32, device=dev)
        tr = lambda k: res[k].data_ptr() if k in res else None
        run = N.QuadBraxRun(max_steps=T, trace_envs=M, deterministic=int(bool(deterministic)),
                            noise_step0=int(noise_step0) & 0xFFFFFFFF, seed=int(seed) & (2**64 - 1),
                            metrics=N.QuadBraxMetrics(**{k: res[k].data_ptr() for k, _ in N.BRAX_METRIC_FIELDS}),
                            trace_actions=tr("actions"), trace_obs=tr("obs"), trace_pos=tr("pos"),
                            trace_target=tr("target"))
        N.check(N.lib().quad_brax_episode(env._h, C.byref(self.arch), _p(self.packed), C.byref(run),
                      current_stream(self.device)), "quad_brax_episode")
        return res

    def sample(self, obs: torch.Tensor, actions_env: torch.Tensor, raw: torch.Tensor, log_prob: torch.Tensor,
               logits: Optional[torch.Tensor] = None, *, seed: int = 0, env_id_base: int = 0,
               noise_step: int = 0) -> None:
        """quad_brax_actor_sample: raw = loc + scale z, log_prob = NormalTanh.log_prob(logits, raw),
        actions_env = tanh(raw) (act's bits for deterministic=False), and the logits unless None."""
        n, dev, f32 = obs.shape[0], self.device, torch.float32
        _need(obs, (n, N.BRAX_OBS), f32, dev, "obs")
        _need(actions_env, (n, 4), f32, dev, "actions_env")
        _need(raw, (n, 4), f32, dev, "raw")
        _need(log_prob, (n,), f32, dev, "log_prob")
        if logits is not None:
            _need(logits, (n, N.BRAX_LOGITS), f32, dev, "logits")
        N.check(N.lib().quad_brax_actor_sample(C.byref(self.arch), _p(self.packed), _p(obs), _p(logits), _p(raw),
                                               _p(log_prob), _p(actions_env), n, int(seed) & (2**64 - 1),
                                               int(env_id_base) & (2**64 - 1), int(noise_step) & 0xFFFFFFFF,
                                               current_stream(self.device)), "quad_brax_actor_sample")

    def unroll(self, env, *, num_unrolls: int, unroll_length: int, seed: int = 0, noise_step0: int = 0,
               ep_ret: torch.Tensor, stats: Optional[torch.Tensor] = None) -> dict:
        """quad_brax_unroll: num_unrolls x unroll_length steps of BraxPPO._unrolls from the envs' current state in one
        launch (the env resets itself: auto_reset). ep_ret [N] f32 carries the running episode returns between calls.
        Returns device tensors with _unrolls' shapes -- obs [U, L, N, 21], nxt [U, N, 21], raw [U, L, N, 4], logp,
        rew, disc, trunc [U, L, N], views of the launch's time-major buffers -- and finished (episodes) and ret_sum
        (float64, their returns' sum), reduced from the slots. stats [POLICY_STAT_SLOTS, 2] float64, if given, is
        accumulated into and not zeroed."""
        U, L, n, dev, f32 = int(num_unrolls), int(unroll_length), env.num_envs, self.device, torch.float32
        T = U * L
        _need(ep_ret, (n,), f32, dev, "ep_ret")
        if stats is None:
            stats = torch.zeros(N.POLICY_STAT_SLOTS, 2, dtype=torch.float64, device=dev)
        else:
            _need(stats, (N.POLICY_STAT_SLOTS, 2), torch.float64, dev, "stats")
        before = stats.sum(0)
        e = lambda *shape: torch.empty(*shape, dtype=f32, device=dev)
        buf = dict(obs=e(T, n, N.BRAX_OBS), raw=e(T, n, 4), log_prob=e(T, n), reward=e(T, n), discount=e(T, n),
                   truncation=e(T, n), next_obs=e(U, n, N.BRAX_OBS))
        u = N.QuadBraxUnroll(**{k: t.data_ptr() for k, t in buf.items()}, ep_ret=ep_ret.data_ptr(),
                             stats=stats.data_ptr(), steps=T, unroll_length=L,
                             noise_step0=int(noise_step0) & 0xFFFFFFFF, seed=int(seed) & (2**64 - 1))
        N.check(N.lib().quad_brax_unroll(env._h, C.byref(self.arch), _p(self.packed), C.byref(u),
                      current_stream(self.device)), "quad_brax_unroll")
        tot = stats.sum(0) - before
        v = lambda k, *tail: buf[k].view(U, L, n, *tail)
        return dict(obs=v("obs", N.BRAX_OBS), nxt=buf["next_obs"], raw=v("raw", 4), logp=v("log_prob"),
                    rew=v("reward"), disc=v("discount"), trunc=v("truncation"), finished=tot[1], ret_sum=tot[0])


# (num_envs, num_minibatches, unroll_length) for which the fused update did not beat the torch update in
# profiles/brax_update/bench.json (by 19's to 21's rule): it won every measured row
BRAX_UPDATE_KEEP_TORCH = frozenset()

_BRAX_UPDATE_FAMILY = ("the fused Brax update (quad_brax_ppo_grad) trains policy and value nets with hidden sizes "
                       f"{N.BRAX_PPO_HIDDEN} and relu, unroll_length in [1, {N.BRAX_PPO_MAX_L}]")


def brax_update_family(cfg) -> None:
    """ValueError naming the family unless cfg's nets and unroll length are quad_brax_ppo_grad's."""
    sizes = (tuple(int(x) for x in cfg.policy_hidden_sizes), tuple(int(x) for x in cfg.value_hidden_sizes))
    if (sizes != (N.BRAX_PPO_HIDDEN, N.BRAX_PPO_HIDDEN) or cfg.activation != "relu"
            or not 1 <= int(cfg.unroll_length) <= N.BRAX_PPO_MAX_L):
        raise ValueError(f"{_BRAX_UPDATE_FAMILY}, got policy {sizes[0]}, value {sizes[1]}, {cfg.activation!r}, "
                         f"unroll_length {cfg.unroll_length}")


def brax_update_supported(cfg, env=None) -> bool:
    """The fused update where its family holds and it did not lose to the torch update (BRAX_UPDATE_KEEP_TORCH)."""
    try:
        brax_update_family(cfg)
    except (ValueError, TypeError, AttributeError):
        return False
    if env is not None and getattr(env, "device", torch.device("cpu")).type != "cuda":
        return False
    return (int(cfg.num_envs), int(cfg.num_minibatches), int(cfg.unroll_length)) not in BRAX_UPDATE_KEEP_TORCH


class FusedBraxLearner:
    """The gradient of ppo/brax_ppo.py brax_ppo_loss in four launches (csrc/brax_learner.hip, quad_brax_ppo_grad) and
    the Adam step in two (quad_clip_adam), bound to a BraxActorCritic, its RunningStats and a BraxPPOConfig.

    grads() gathers a minibatch of trajectories straight from the time-major unroll buffers and overwrites the
    parameters' .grad tensors; adam_step() updates the parameters through the state tensors of `opt` (the learner's
    own torch.optim.Adam), so opt.state_dict() and checkpoints stay what they are."""

    entry = "quad_brax_ppo_grad"             # the C entry point grads() calls
    _family, _check = _BRAX_UPDATE_FAMILY, staticmethod(brax_update_family)

    def __init__(self, net, norm, cfg, opt: Optional[torch.optim.Adam] = None, seed: int = 0):
        self._check(cfg)
        self.net, self.norm, self.cfg, self.opt, self.seed = net, norm, cfg, opt, int(seed)
        self.params = [*net.policy.kernels, *net.policy.biases, *net.value.kernels, *net.value.biases]
        shapes = [tuple(p.shape) for p in self.params]
        (p1, p2), (v1, v2) = self.sizes = self._sizes(cfg)
        want = [(N.BRAX_OBS, p1), (p1, p2), (p2, N.BRAX_LOGITS), (p1,), (p2,), (N.BRAX_LOGITS,),
                (N.BRAX_OBS, v1), (v1, v2), (v2, 1), (v1,), (v2,), (1,)]
        if shapes != want:
            raise ValueError(f"{self._family} on 21-D observations and 4-D actions, got {shapes}")
        self.device = self.params[0].device
        if self.device.type != "cuda":
            raise N.QuadError(f"{type(self).__name__} needs the nets on a ROCm GPU")
        for p in self.params:
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise ValueError("parameters must be contiguous float32")
        self._ws = Workspace(self.device)
        self._adam = None

    @staticmethod
    def _sizes(cfg):
        return N.BRAX_PPO_HIDDEN, N.BRAX_PPO_HIDDEN

    def _workspace_bytes(self, prm, mb: int, L: int) -> int:
        return int(N.lib().quad_brax_ppo_workspace_bytes(mb, L))

    def _ordered(self, ts):
        """[k0, k1, k2, b0, b1, b2] of each net -> w0, b0, w1, b1, w2, b2 of the policy, then of the value net."""
        return [ts[6 * n + 3 * j + i] for n in range(2) for i in range(3) for j in range(2)]

    def grads(self, buffers: dict, index: torch.Tensor, *, entropy_noise: Optional[torch.Tensor] = None,
              noise_step: int = 0, stats: Optional[torch.Tensor] = None, diag: Optional[dict] = None) -> None:
        """quad_brax_ppo_grad on the minibatch of trajectories `index` ([mb] int64, each in [0, U * N)) of `buffers`:
        obs [U, L, N, 21], nxt [U, N, 21], raw [U, L, N, 4], logp, rew, disc, trunc [U, L, N] (FusedBraxActor.unroll's
        and BraxPPO._unrolls' tensors). entropy_noise [L, mb, 4] is the entropy sample's z; None draws it from
        Philox(seed; trajectory, noise_step * L + t). stats [3] receives policy_loss, v_loss, entropy_loss. diag, a
        dict, receives "values" [L + 1, mb], "vs", "advantages" [L, mb] and "noise" [L, mb, 4]. The gradients
        overwrite the parameters' .grad (created when absent)."""
        prm, b, grd = self.describe(buffers, index, entropy_noise=entropy_noise, noise_step=noise_step, stats=stats,
                                    diag=diag)
        N.check(getattr(N.lib(), self.entry)(C.byref(prm), C.byref(b), C.byref(grd), self._ws.ptr, self._ws.nbytes,
                                             current_stream(self.device)), self.entry)

    def describe(self, buffers: dict, index: torch.Tensor, *, entropy_noise=None, noise_step: int = 0, stats=None,
                 diag: Optional[dict] = None):
        """grads' checked arguments as (QuadBraxPPOParams, QuadBraxPPOBatch, QuadBraxPPOGrads); sizes self._ws."""
        dev, f32, c = self.device, torch.float32, self.cfg
        obs = buffers["obs"]
        U, L, n = (int(x) for x in obs.shape[:3])
        mb = int(index.shape[0])
        for k, shp in (("obs", (U, L, n, N.BRAX_OBS)), ("nxt", (U, n, N.BRAX_OBS)), ("raw", (U, L, n, 4)),
                       ("logp", (U, L, n)), ("rew", (U, L, n)), ("disc", (U, L, n)), ("trunc", (U, L, n))):
            _need(buffers[k], shp, f32, dev, k)
        _need(index, (mb,), torch.int64, dev, "index")
        if entropy_noise is not None:
            _need(entropy_noise, (L, mb, 4), f32, dev, "entropy_noise")
        if stats is not None:
            _need(stats, (3,), f32, dev, "stats")
        out = {}
        if diag is not None:
            e = lambda *s: torch.empty(*s, dtype=f32, device=dev)
            out = dict(values=e(L + 1, mb), vs=e(L, mb), advantages=e(L, mb), noise=e(L, mb, 4))
            diag.update(out)
        for p in self.params:
            if p.grad is None:
                p.grad = torch.empty_like(p)
            elif not p.grad.is_contiguous():
                raise ValueError("every parameter needs a contiguous .grad")
        mean, std = self.norm.mean, self.norm.std
        _need(mean, (N.BRAX_OBS,), f32, dev, "mean")
        _need(std, (N.BRAX_OBS,), f32, dev, "std")
        (p1, p2), (v1, v2) = self.sizes
        prm = N.QuadBraxPPOParams(*[p.data_ptr() for p in self._ordered(self.params)], mean.data_ptr(),
                                  std.data_ptr(), float(self.net.dist.min_std), p1, p2, v1, v2,
                                  N.BRAX_ACTFNS[c.activation])
        need = self._workspace_bytes(prm, mb, L)
        if need <= 0:
            raise ValueError(f"{self.entry}: a minibatch of {mb} trajectories of {L} steps is outside its limits")
        self._ws.reserve(max(need, 16))
        grd = N.QuadBraxPPOGrads(*[p.grad.data_ptr() for p in self._ordered(self.params)])
        b = N.QuadBraxPPOBatch(
            obs=obs.data_ptr(), next_obs=buffers["nxt"].data_ptr(), raw=buffers["raw"].data_ptr(),
            log_prob=buffers["logp"].data_ptr(), reward=buffers["rew"].data_ptr(),
            discount=buffers["disc"].data_ptr(), truncation=buffers["trunc"].data_ptr(), index=index.data_ptr(),
            entropy_noise=_p(entropy_noise), noise_out=_p(out.get("noise")), values=_p(out.get("values")),
            vs=_p(out.get("vs")), advantages=_p(out.get("advantages")), stats=_p(stats), U=U, L=L, N=n, mb=mb,
            clipping_epsilon=float(c.clipping_epsilon), entropy_cost=float(c.entropy_cost),
            discounting=float(c.discounting), gae_lambda=float(c.gae_lambda), reward_scaling=float(c.reward_scaling),
            normalize_advantage=int(bool(c.normalize_advantage)), noise_step=int(noise_step) & 0xFFFFFFFF,
            seed=self.seed & (2**64 - 1))
        b._keep = (mean, std, entropy_noise, stats, out)  # the launches read them: alive as long as the descriptor
        return prm, b, grd

    def adam_step(self) -> None:
        """opt.step() of the learner's Adam (optax defaults: no clipping, eps 1e-8) as quad_clip_adam on the
        optimizer's own state tensors."""
        if self.opt is None:
            raise ValueError(f"{type(self).__name__}.adam_step needs the optimizer (opt=...)")
        if self._adam is None:
            from .learner import FusedAdam
            self._adam = FusedAdam(self.opt, 0.0)
        self._adam.step()


# (num_envs, num_minibatches, unroll_length, (policy sizes, value sizes, activation)) for which the general family's
# fused update did not beat the torch update in profiles/brax_arch_update/bench.json (by 19's to 22's rule)
BRAX_ARCH_UPDATE_KEEP_TORCH = frozenset()

_BRAX_UPDATE_ARCH_FAMILY = ("the general fused Brax update (quad_brax_ppo_arch_grad) trains two-hidden-layer policy and "
                            f"value nets (h1, h2), each h1 a multiple of 32 in [32, {N.BRAX_PPO_ARCH_MAX_H1}], each h2 in "
                            f"{N.BRAX_PPO_ARCH_H2}, one of relu / tanh / silu, unroll_length in [1, {N.BRAX_PPO_MAX_L}]")


def _brax_arch_sizes(cfg):
    return (tuple(int(x) for x in cfg.policy_hidden_sizes), tuple(int(x) for x in cfg.value_hidden_sizes))


def brax_update_arch_family(cfg) -> None:
    """ValueError naming the family unless cfg's nets, activation and unroll length are quad_brax_ppo_arch_grad's."""
    sizes = _brax_arch_sizes(cfg)
    ok = all(len(s) == 2 and s[0] % 32 == 0 and 32 <= s[0] <= N.BRAX_PPO_ARCH_MAX_H1 and s[1] in N.BRAX_PPO_ARCH_H2
             for s in sizes)
    if not ok or cfg.activation not in N.BRAX_ACTFNS or not 1 <= int(cfg.unroll_length) <= N.BRAX_PPO_MAX_L:
        raise ValueError(f"{_BRAX_UPDATE_ARCH_FAMILY}, got policy {sizes[0]}, value {sizes[1]}, {cfg.activation!r}, "
                         f"unroll_length {cfg.unroll_length}")


def brax_update_arch_supported(cfg, env=None) -> bool:
    """The general fused update where its family holds and it did not lose to the torch update
    (BRAX_ARCH_UPDATE_KEEP_TORCH)."""
    try:
        brax_update_arch_family(cfg)
    except (ValueError, TypeError, AttributeError):
        return False
    if env is not None and getattr(env, "device", torch.device("cpu")).type != "cuda":
        return False
    key = (int(cfg.num_envs), int(cfg.num_minibatches), int(cfg.unroll_length), (*_brax_arch_sizes(cfg), cfg.activation))
    return key not in BRAX_ARCH_UPDATE_KEEP_TORCH


class FusedBraxArchLearner(FusedBraxLearner):
    """FusedBraxLearner for every two-hidden-layer net of the Brax actor's family (csrc/brax_learner_arch.hip,
    quad_brax_ppo_arch_grad: five launches): tanh, SiLU and ReLU, h1 up to 512, h2 up to 256, the policy's and the
    value net's sizes independent. The interface -- grads, describe, adam_step, params -- is FusedBraxLearner's."""

    entry = "quad_brax_ppo_arch_grad"
    _family, _check = _BRAX_UPDATE_ARCH_FAMILY, staticmethod(brax_update_arch_family)
    _sizes = staticmethod(_brax_arch_sizes)

    def _workspace_bytes(self, prm, mb: int, L: int) -> int:
        return int(N.lib().quad_brax_ppo_arch_workspace_bytes(C.byref(prm), mb, L))


def brax_learner_class_for(cfg):
    """FusedBraxLearner for (128, 128) ReLU policy and value nets -- the specialised kernels keep their net, as
    fused_learner_for's do -- and FusedBraxArchLearner for every other member of the general family; ValueError
    naming that family outside it."""
    brax_update_arch_family(cfg)
    special = _brax_arch_sizes(cfg) == (N.BRAX_PPO_HIDDEN, N.BRAX_PPO_HIDDEN) and cfg.activation == "relu"
    return FusedBraxLearner if special else FusedBraxArchLearner


def fused_brax_learner_for(net, norm, cfg, opt: Optional[torch.optim.Adam] = None, seed: int = 0):
    """The fused learner of a BraxActorCritic of the general family: brax_learner_class_for(cfg)'s class."""
    return brax_learner_class_for(cfg)(net, norm, cfg, opt=opt, seed=seed)
