"""A population of independent PPO learners trained in lock-step launches (quad_pop_*).

At the reference's own scale (train.py / optimize.py: 8 or 16 envs, minibatches of 128 rows) one learner's
launches occupy a handful of the GPU's 256 CUs: a hyperparameter search or a seed sweep is dozens to
thousands of such runs that differ only in a seed and a few scalars. `PopulationPPO` holds P of them -- each
a complete `PPO` (its own env handle, policy, Adam state and rollout buffers, initialised exactly as
`PPO(env, cfg, seed=s)` initialises it) -- and issues, per step of the algorithm, ONE launch that does the
step for every active member: the member is one more grid dimension of the kernel, whose blocks read their
member's argument struct from a device table and run the single kernel's body. Member m is therefore
bit-identical to the stand-alone `PPO` with the same config and seed, after any number of iterations
(tests/test_gpu_population_ppo.py).

Shared by all members: the env kind / wrapper / constants, envs per member, n_steps, the minibatch size,
net_arch (128, 128), normalize_advantage. Per member: the seed, n_epochs (a member whose epochs are done is
simply not in the launch's subset) and every scalar hyperparameter.

`ArchPopulationPPO` is the same class on the general family's kernels (tanh, other widths), and
`population_for` picks between the two by the members' arch.
"""
from __future__ import annotations

import ctypes as C
import time
from dataclasses import replace
from typing import List, Optional, Sequence, Tuple

import torch

from .. import _native as N
from ..envs import QuadVecEnv
from .fused import FusedActorCritic, FusedPolicy, arch_rollout_keeps_torch, current_stream
from .learner import ARCH_UPDATE_KEEP_TORCH, LEARNER_FAMILY, FusedArchLearner, FusedLearner
from .ppo import PPO, PPOConfig, RolloutStats


def _p(t: torch.Tensor):
    return t.data_ptr()


def refuse_deployed(who: str, k: int, cfg: PPOConfig) -> None:
    """The quad_pop_* launches collect the env's own observation: a member asking for the deployed one
    is refused by name, before anything is built."""
    if getattr(cfg, "obs_mode", "env") != "env":
        raise ValueError(f"{who}: member {k} has obs_mode={cfg.obs_mode!r}; the population launches collect the env "
                         'observation only (train it alone: PPO with obs_mode="deployed")')


class PopulationPPO:
    """P stand-alone `PPO` learners driven by population launches.

    members: a sequence of (PPOConfig, seed). All configs must agree on n_steps, the minibatch size
    (batch_size, or n_minibatches), net_arch == (128, 128), normalize_advantage and the fused flags (all on);
    n_epochs and every scalar may differ. `n_envs`, `env`, `wrapper` and `env_kwargs` describe each member's
    QuadVecEnv (seeded with the member's seed, as tests/hpo_repro.py seeds a stand-alone run)."""

    def __init__(self, members: Sequence[Tuple[PPOConfig, int]], n_envs: int = 8, env: str = "hover",
                 wrapper: Optional[str] = None, device=None, env_kwargs: Optional[dict] = None):
        members = list(members)
        if len(members) < 1:
            raise ValueError("PopulationPPO needs at least one (PPOConfig, seed)")
        c0 = members[0][0]
        total = c0.n_steps * int(n_envs)
        for k, (cfg, _) in enumerate(members):
            self._check_obs_mode(k, cfg)
            self._check_config(cfg, c0)
            if not (cfg.fused_policy and cfg.fused_rollout and cfg.fused_update):
                raise ValueError("PopulationPPO needs fused_policy, fused_rollout and fused_update")
            if cfg.n_steps != c0.n_steps:
                raise ValueError(f"members must share n_steps ({cfg.n_steps} != {c0.n_steps})")
            if (cfg.batch_size, cfg.n_minibatches) != (c0.batch_size, c0.n_minibatches):
                raise ValueError("members must share batch_size / n_minibatches")
            if cfg.normalize_advantage != c0.normalize_advantage or cfg.rollout_chunk != c0.rollout_chunk:
                raise ValueError("members must share normalize_advantage and rollout_chunk")
            if cfg.n_epochs < 1:
                raise ValueError("n_epochs must be >= 1")
        batch = int(c0.batch_size) if c0.batch_size is not None else max(1, total // c0.n_minibatches)
        if batch < 1 or batch > N.POP_MAX_BATCH:
            raise ValueError(f"minibatch of {batch} rows: the population gradient takes 1..{N.POP_MAX_BATCH}")
        if total % batch != 0:
            raise ValueError(f"the minibatch ({batch}) does not divide the rollout buffer ({c0.n_steps} x {n_envs})")
        self.batch, self.nmb, self.total = batch, total // batch, total
        self.n_steps, self.n_envs = c0.n_steps, int(n_envs)
        self.normalize_advantage = bool(c0.normalize_advantage)
        self._lib = N.lib()
        self.members: List[PPO] = []
        self._gens: List[torch.Generator] = []
        kw = dict(env_kwargs or {})
        self._env_kind, self._wrapper = env, wrapper
        self._env_kw = {k: v for k, v in kw.items() if k == "cfg_overrides"}  # what an evaluation env shares
        for cfg, seed in members:
            e = QuadVecEnv(self.n_envs, env=env, wrapper=wrapper, device=device, seed=int(seed), **kw)
            m = PPO(e, cfg, seed=int(seed))
            # exactly this population's kernel classes: its launches read that packed image and that workspace
            # (the 128-128 ReLU net's and the general family's differ in both)
            if (not m._one_launch or type(m._fp) is not self._policy_class
                    or type(m._learner) is not self._learner_class):
                raise ValueError("the env / policy is not one the fused rollout and update run")
            self.members.append(m)
            # PPO.__init__ leaves torch's default CPU generator at manual_seed(seed); the stand-alone run then
            # draws one epoch-permutation key per epoch from it. A generator of the member's own replays that.
            self._gens.append(torch.Generator().manual_seed(int(seed)))
        self.device = self.members[0].device
        self.P = P = len(self.members)
        self.active = list(range(P))
        dev = self.device
        m0 = self.members[0]
        ws = self._workspace_bytes(m0, batch)
        if ws <= 0:
            raise N.QuadError("quad_pop_workspace_bytes failed: " + self._lib.quad_last_error().decode(errors="replace"))
        ws = (ws + 255) // 256 * 256
        self._ws = torch.empty(P, ws, dtype=torch.uint8, device=dev)
        self._perm = torch.empty(P, total, dtype=torch.int64, device=dev)
        self._sums = torch.zeros(P, self.nmb, N.ADV_SUM_DOUBLES, dtype=torch.float64, device=dev)
        self._mb = torch.zeros(P, self.nmb, 4, dtype=torch.float32, device=dev)
        arr = (N.QuadPopMember * P)()
        for i, m in enumerate(self.members):
            self._fill(arr[i], m, i, ws)
        self._h = self._create(arr, P, batch)
        self._subsets = {tuple(range(P)): 0}
        self._t_host = 0
        self._started = False

    # ---- what a kernel family's population differs in (ArchPopulationPPO overrides these) ----------------
    _policy_class, _learner_class = FusedPolicy, FusedLearner
    _block_envs = 256  # envs per rollout block: block b adds its episode statistics into slot b

    def _check_obs_mode(self, k: int, cfg: PPOConfig) -> None:
        refuse_deployed(type(self).__name__, k, cfg)

    def _start_member(self, m: PPO) -> None:
        """What PPO.collect_rollouts does before a member's first rollout."""
        m.last_obs.copy_(m.env.reset())
        m.last_start.fill_(1.0)
        m._started = True

    def _eval_run(self, i: int, e: QuadVecEnv, res: dict, verr: torch.Tensor) -> N.QuadPolicyRun:
        """Member i's QuadPolicyRun for evaluate(): its rows of the metric tensors, the env's own observation."""
        return N.QuadPolicyRun(obs_mode=N.OBS_ENV, max_steps=int(e.max_episode_steps), trace_envs=0,
                               est=N.QuadVelEst(alpha=None, alpha_all=0.8, max_dt=0.1, state=None),
                               est_dt=float(e.dt), trace_actions=None, trace_state12=None, trace_obs=None,
                               trace_vel_est=None,
                               metrics=N.QuadPidMetrics(**{k: res[k][i].data_ptr() for k, _ in N.PID_METRIC_FIELDS}),
                               vel_err_sq=verr[i].data_ptr())

    def _check_config(self, cfg: PPOConfig, c0: PPOConfig) -> None:
        if tuple(cfg.net_arch) != (128, 128) or cfg.activation != "relu":
            raise ValueError(f"PopulationPPO runs the fused (128, 128) relu policy only, got net_arch "
                             f"{cfg.net_arch} {cfg.activation}")

    def _workspace_bytes(self, m0: PPO, batch: int) -> int:
        return int(self._lib.quad_pop_workspace_bytes(C.byref(m0._adam._build()), batch))

    def _create(self, arr, P: int, batch: int) -> C.c_void_p:
        h = C.c_void_p()
        N.check(self._lib.quad_pop_create(arr, P, batch, int(self.normalize_advantage), C.byref(h)), "quad_pop_create")
        return h

    # ------------------------------------------------------------------------------------
    def _fill(self, e: N.QuadPopMember, m: PPO, i: int, ws: int) -> None:
        prm, grd = m._learner._structs()
        cfg = m.cfg
        e.env = m.env._h.value
        e.params, e.grads, e.adam = prm, grd, m._adam._build()
        e.packed = _p(m._fp.packed)
        e.rollout = N.QuadRollout(obs_copy=_p(m.buf_obs), actions=_p(m.buf_act), log_prob=_p(m.buf_logp),
                                  value=_p(m.buf_val), episode_starts=_p(m.buf_start), rewards=_p(m.buf_rew),
                                  last_obs=_p(m.last_obs), last_start=_p(m.last_start), ep_ret=_p(m.ep_ret),
                                  ep_len=_p(m.ep_len), stats=_p(m._slots), rows=cfg.n_steps, t0=0, steps=1,
                                  deterministic=0, seed=m._noise_seed & (2**64 - 1), gamma=float(cfg.gamma))
        e.last_values, e.scratch_actions = _p(m._last_v), _p(m._act_env)
        e.advantages, e.returns = _p(m.buf_adv), _p(m.buf_ret)
        e.perm, e.adv_sums, e.mb_stats = _p(self._perm[i]), _p(self._sums[i]), _p(self._mb[i])
        e.workspace, e.workspace_bytes = _p(self._ws[i]), ws
        e.gae_lambda, e.clip_range = float(cfg.gae_lambda), float(cfg.clip_range)
        e.ent_coef, e.vf_coef = float(cfg.ent_coef), float(cfg.vf_coef)

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.quad_pop_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _subset(self, members: Sequence[int]) -> int:
        """The id of the launch subset `members` (registered with the library once: one small upload)."""
        key = tuple(members)
        sid = self._subsets.get(key)
        if sid is None:
            arr = (C.c_int32 * len(key))(*key)
            out = C.c_int32()
            N.check(self._lib.quad_pop_subset(self._h, arr, len(key), C.byref(out)), "quad_pop_subset")
            sid = self._subsets[key] = int(out.value)
        return sid

    # ------------------------------------------------------------------------------------
    def member(self, m: int) -> PPO:
        """Member m as the `PPO` it is: .policy, .opt, .buf_*, .num_timesteps, state_dict() -- what
        export.save_sb3_zip and train.Checkpointer take."""
        return self.members[m]

    def deactivate(self, m: int) -> None:
        """Drop member m from every later launch (a pruned trial stops costing anything)."""
        if m in self.active:
            self.active.remove(m)

    @property
    def num_timesteps(self) -> List[int]:
        return [m.num_timesteps for m in self.members]

    # ------------------------------------------------------------------------------------
    @torch.no_grad()
    def collect_rollouts(self) -> List[Optional[RolloutStats]]:
        """PPO.collect_rollouts (the one-launch path) for every active member; entry m of the result is
        member m's RolloutStats (None for an inactive member)."""
        act = list(self.active)
        out: List[Optional[RolloutStats]] = [None] * self.P
        if not act:
            return out
        L, st, h = self._lib, current_stream(self.device), self._h
        t0 = time.perf_counter()
        sid = self._subset(act)
        N.check(L.quad_pop_pack(h, sid, st), "quad_pop_pack")
        if not self._started:
            for m in self.members:
                self._start_member(m)
            self._started = True
        torch._foreach_zero_([self.members[i]._slots for i in act])
        T = self.n_steps
        chunk = max(1, min(int(self.members[0].cfg.rollout_chunk), T))
        s = 0
        while s < T:
            k = min(chunk, T - s)
            N.check(L.quad_pop_rollout(h, sid, self._t_host + s, k, st), "quad_pop_rollout")
            s += k
        self._t_host += T
        N.check(L.quad_pop_value(h, sid, st), "quad_pop_value")
        N.check(L.quad_pop_gae(h, sid, st), "quad_pop_gae")
        # the episode statistics: block b of a member's rollout adds into slot b, so with one block per member
        # (<= 256 envs; 64 in the general family) slot 0 is the sum; more blocks are summed as PPO sums them (the same
        # order)
        if self.n_envs <= self._block_envs:
            sums = torch.stack([self.members[i]._slots[0] for i in act])
        else:
            sums = torch.stack([self.members[i]._slots.sum(0) for i in act])
        rows = sums.tolist()  # the one host synchronization of the rollout
        dt = time.perf_counter() - t0
        steps = T * self.n_envs
        for i, (ret_sum, len_sum, c) in zip(act, rows):
            m = self.members[i]
            m._t_host += T
            m.num_timesteps += steps
            out[i] = RolloutStats(episodes=int(c), mean_return=ret_sum / c if c else float("nan"),
                                  mean_length=len_sum / c if c else float("nan"), env_steps=steps, seconds=dt,
                                  extra={"local_episodes": int(c), "ranks": 1})
        return out

    def train(self) -> List[Optional[dict]]:
        """PPO.train for every active member: per epoch the members that still have epochs left draw their
        permutation keys, then one launch per step of the update covers them all. Entry m of the result is
        member m's statistics dict (None for an inactive member)."""
        act = list(self.active)
        out: List[Optional[dict]] = [None] * self.P
        if not act:
            return out
        L, st, h = self._lib, current_stream(self.device), self._h
        epochs = {i: int(self.members[i].cfg.n_epochs) for i in act}
        max_e = max(epochs.values())
        # every epoch's keys, drawn per member in epoch order, uploaded once for the whole update
        keys = torch.zeros(max_e, self.P, dtype=torch.int64)
        for i in act:
            for e in range(epochs[i]):
                keys[e, i] = torch.randint(0, 2**62, (1,), dtype=torch.int64, generator=self._gens[i])
        keys = keys.to(self.device, non_blocking=True)
        hist = torch.zeros(max_e, self.P, self.nmb, 4, dtype=torch.float32, device=self.device)
        for e in range(max_e):
            sid = self._subset([i for i in act if epochs[i] > e])
            N.check(L.quad_pop_permutation(h, sid, C.c_void_p(keys[e].data_ptr()), st), "quad_pop_permutation")
            N.check(L.quad_pop_adv_stats_epoch(h, sid, st), "quad_pop_adv_stats_epoch")
            for slot in range(self.nmb):
                N.check(L.quad_pop_ppo_grad(h, sid, slot, st), "quad_pop_ppo_grad")
                N.check(L.quad_pop_clip_adam(h, sid, st), "quad_pop_clip_adam")
            hist[e].copy_(self._mb)
        means = torch.stack([hist[:epochs[i], i].reshape(-1, 4).double().mean(0) for i in act]).tolist()
        for i, a in zip(act, means):
            out[i] = dict(pg_loss=a[0], vf_loss=a[1], entropy=a[2], clip_fraction=a[3], n=epochs[i] * self.nmb)
        return out

    @torch.no_grad()
    def evaluate(self, num_episodes: int = 10, seeds: Optional[Sequence[int]] = None,
                 max_episode_steps: Optional[int] = None) -> List[Optional[dict]]:
        """Every active member's deterministic policy on `num_episodes` fresh episodes of its own, all members
        in ONE quad_pop_episode launch: what evaluate.evaluate_episodes(member.policy, num_episodes,
        seed=seeds[m]) returns for member m (the same bits). seeds: one env seed per member (default: the
        member's index). Entry m of the result is {"mean_reward", "mean_length", "rewards", "lengths",
        "terminated"} (None for an inactive member)."""
        act = list(self.active)
        out: List[Optional[dict]] = [None] * self.P
        if not act:
            return out
        seeds = list(range(self.P)) if seeds is None else [int(s) for s in seeds]
        if len(seeds) != self.P:
            raise ValueError("seeds: one per member")
        L, st, h, dev, n = self._lib, current_stream(self.device), self._h, self.device, int(num_episodes)
        # fresh evaluation handles for the ACTIVE members only (a deactivated member costs nothing), seeded as
        # evaluate_episodes seeds its env; the table takes each handle's seed as it is when attached
        envs = {i: QuadVecEnv(n, env=self._env_kind, wrapper=self._wrapper, device=dev, seed=seeds[i],
                              max_episode_steps=max_episode_steps, auto_reset=False, **self._env_kw) for i in act}
        res = {k: torch.zeros(self.P, n, dtype=getattr(torch, dt), device=dev) for k, dt in N.PID_METRIC_FIELDS}
        verr = torch.zeros(self.P, n, dtype=torch.float64, device=dev)
        arr = (N.QuadPopEval * self.P)()  # env = NULL: no entry for that member
        for i, e in envs.items():
            e.reset()
            arr[i].env = e._h.value
            arr[i].run = self._eval_run(i, e, res, verr)
        try:
            sid = self._subset(act)
            N.check(L.quad_pop_pack(h, sid, st), "quad_pop_pack")
            N.check(L.quad_pop_attach_eval(h, arr), "quad_pop_attach_eval")
            N.check(L.quad_pop_episode(h, sid, st), "quad_pop_episode")
            r, l, status = res["total_reward"].cpu().numpy(), res["steps"].cpu().numpy(), res["status"].cpu().numpy()
        finally:
            torch.cuda.synchronize(dev)
            L.quad_pop_detach_eval(h)  # the table refers to the handles closed below
            for e in envs.values():
                e.close()
        for i in act:
            out[i] = {"rewards": r[i], "lengths": l[i], "terminated": status[i] == N.PID_TERMINATED,
                      "mean_reward": float(r[i].mean()), "mean_length": float(l[i].mean())}
        return out

    def learn(self, total_timesteps: int, callback=None) -> "PopulationPPO":
        """Iterate collect_rollouts + train until every active member has total_timesteps env steps.
        callback(self, iteration, rollout_stats, train_stats) may deactivate members; returning False stops."""
        it = 0
        while self.active and min(self.members[i].num_timesteps for i in self.active) < total_timesteps:
            rs = self.collect_rollouts()
            ts = self.train()
            it += 1
            if callback is not None and callback(self, it, rs, ts) is False:
                break
        return self


def _arch_key(cfg: PPOConfig) -> tuple:
    return tuple(int(x) for x in cfg.net_arch), str(cfg.activation)


class ArchPopulationPPO(PopulationPPO):
    """`PopulationPPO` for the general actor's family: P stand-alone `PPO` learners with
    fused_rollout_arch and fused_update_arch -- policy and value nets 12 -> H1 -> H2 -> 4 / 1, H1 a multiple of 32 up
    to 512, H2 in {64, 128, 256}, relu or tanh, other than the (128, 128) relu net `PopulationPPO` runs -- driven by
    the population forms of quad_actor_critic_pack, quad_actor_rollout, quad_actor_critic_act, quad_ppo_arch_grad and
    quad_actor_episode. Every member shares the arch as it shares the other shapes; member m is bit-identical to
    `PPO(env, cfg, seed)` with both arch flags (tests/test_gpu_population_arch_ppo.py)."""

    _policy_class, _learner_class = FusedActorCritic, FusedArchLearner
    _block_envs = 64

    def _check_config(self, cfg: PPOConfig, c0: PPOConfig) -> None:
        if _arch_key(cfg) != _arch_key(c0):
            raise ValueError(f"members must share net_arch and activation ({_arch_key(cfg)} != {_arch_key(c0)})")
        if _arch_key(cfg) == ((128, 128), "relu"):
            raise ValueError("the (128, 128) relu policy trains on PopulationPPO (population_for picks the class)")
        if not (cfg.fused_rollout_arch and cfg.fused_update_arch):
            raise ValueError("ArchPopulationPPO needs fused_rollout_arch and fused_update_arch")
        hidden, act = _arch_key(cfg)
        if (len(hidden) != 2 or hidden[0] % 32 or not 32 <= hidden[0] <= N.ACTOR_MAX_H1 or hidden[1] not in N.ACTOR_H2
                or act not in N.ACTFNS):
            raise ValueError(f"ArchPopulationPPO trains {LEARNER_FAMILY}, got net_arch {cfg.net_arch} {cfg.activation}")

    def _workspace_bytes(self, m0: PPO, batch: int) -> int:
        return int(self._lib.quad_pop_arch_workspace_bytes(C.byref(m0._fp.arch), C.byref(m0._adam._build()), batch))

    def _create(self, arr, P: int, batch: int) -> C.c_void_p:
        h = C.c_void_p()
        N.check(self._lib.quad_pop_create_arch(C.byref(self.members[0]._fp.arch), arr, P, batch,
                                               int(self.normalize_advantage), C.byref(h)), "quad_pop_create_arch")
        return h


# ((H1, H2), activation) whose 64-member iteration did not take less than half of 64 stand-alone iterations in
# profiles/arch_population/bench.json (by 18's bar): population_for keeps them off the population path
ARCH_POPULATION_KEEP_SERIAL = frozenset()


def population_for(members: Sequence[Tuple[PPOConfig, int]], n_envs: int = 8, env: str = "hover",
                   wrapper: Optional[str] = None, device=None, env_kwargs: Optional[dict] = None) -> PopulationPPO:
    """The population class of `members`' arch, as fused_policy_for / fused_learner_for pick a member's kernels: a
    PopulationPPO for (128, 128) relu configs, an ArchPopulationPPO (the arch flags switched on in the configs it
    gets) for any other member of the family. ValueError outside the family, for mixed arches, and for a row the
    drivers keep off the fused path (ARCH_ROLLOUT_KEEP_TORCH, ARCH_UPDATE_KEEP_TORCH, ARCH_POPULATION_KEEP_SERIAL)."""
    members = list(members)
    if len(members) < 1:
        raise ValueError("population_for needs at least one (PPOConfig, seed)")
    for k, (cfg, _) in enumerate(members):
        refuse_deployed("population_for", k, cfg)
    keys = {_arch_key(cfg) for cfg, _ in members}
    if len(keys) != 1:
        raise ValueError(f"members must share net_arch and activation, got {sorted(keys)}")
    (hidden, act), = keys
    kw = dict(n_envs=n_envs, env=env, wrapper=wrapper, device=device, env_kwargs=env_kwargs)
    if (hidden, act) == ((128, 128), "relu"):
        return PopulationPPO(members, **kw)
    c0 = members[0][0]
    total = c0.n_steps * int(n_envs)
    batch = int(c0.batch_size) if c0.batch_size is not None else max(1, total // c0.n_minibatches)
    if (arch_rollout_keeps_torch(hidden, act, n_envs) or (hidden, act, batch) in ARCH_UPDATE_KEEP_TORCH
            or (hidden, act) in ARCH_POPULATION_KEEP_SERIAL):
        raise ValueError(f"net_arch {hidden} {act} stays off the fused population path at {n_envs} envs, minibatch "
                         f"{batch} (it did not beat the path it would replace)")
    return ArchPopulationPPO([(replace(cfg, fused_rollout_arch=True, fused_update_arch=True), seed)
                              for cfg, seed in members], **kw)


def refuse_env_mode(who: str, k: int, cfg: PPOConfig) -> None:
    """refuse_deployed's mirror image: the deployed population's rollout launch builds the deployed observation for
    every member, so a member asking for the env's own is refused by index, before anything is built."""
    if getattr(cfg, "obs_mode", "env") != "deployed":
        raise ValueError(f"{who}: member {k} has obs_mode={getattr(cfg, 'obs_mode', 'env')!r}; every member of a "
                         'deployed population collects the deployed observation (obs_mode="deployed"; an env-mode '
                         "member trains on population_for's classes)")


def _in_family(hidden: tuple, act: str) -> bool:
    return (len(hidden) == 2 and hidden[0] % 32 == 0 and 32 <= hidden[0] <= N.ACTOR_MAX_H1 and hidden[1] in N.ACTOR_H2
            and act in N.ACTFNS)


class DeployedPopulationPPO(ArchPopulationPPO):
    """`ArchPopulationPPO` for members with obs_mode="deployed" (DESIGN section 28): P stand-alone `PPO` learners that
    collect on the observation the ROS2 node hands the policy, driven by quad_pop_create_deployed's launches -- the
    rollout is quad_actor_rollout_deployed behind the member dimension, the evaluations fly quad_actor_episode in
    deployed mode. Members share the arch and the shapes as in the other populations and may differ in
    velocity_alpha and est_max_dt; each member's est_state is referenced by the library's table, not copied, and
    started as the stand-alone `PPO` starts it. Every arch of the family trains here, the (128, 128) relu net
    included: as in a stand-alone deployed `PPO` it collects on the family's kernels and updates on `FusedLearner`.
    Member m is bit-identical to `PPO(env, cfg, seed)` (tests/test_gpu_deployed_population.py)."""

    def __init__(self, members: Sequence[Tuple[PPOConfig, int]], *args, **kw):
        members = list(members)
        if members and _arch_key(members[0][0]) == ((128, 128), "relu"):
            self._learner_class = FusedLearner  # the pairing of PPO(obs_mode="deployed") for that net
        self._eval_alpha: Optional[float] = None
        super().__init__(members, *args, **kw)

    def _check_obs_mode(self, k: int, cfg: PPOConfig) -> None:
        refuse_env_mode(type(self).__name__, k, cfg)

    def _check_config(self, cfg: PPOConfig, c0: PPOConfig) -> None:
        if _arch_key(cfg) != _arch_key(c0):
            raise ValueError(f"members must share net_arch and activation ({_arch_key(cfg)} != {_arch_key(c0)})")
        hidden, act = _arch_key(cfg)
        if not _in_family(hidden, act):
            raise ValueError(f"DeployedPopulationPPO trains {LEARNER_FAMILY}, got net_arch {cfg.net_arch} "
                             f"{cfg.activation}")
        if (hidden, act) != ((128, 128), "relu") and not cfg.fused_update_arch:
            raise ValueError("DeployedPopulationPPO needs fused_update_arch for a net other than (128, 128) relu")

    def _workspace_bytes(self, m0: PPO, batch: int) -> int:
        L = N.need_deployed_population()
        return int(L.quad_pop_deployed_workspace_bytes(C.byref(m0._fp.arch), C.byref(m0._adam._build()), batch))

    def _create(self, arr, P: int, batch: int) -> C.c_void_p:
        L = N.need_deployed_population()
        dep = (N.QuadPopDeploy * P)()
        for d, m in zip(dep, self.members):
            d.est = N.QuadVelEst(alpha=None, alpha_all=float(m.cfg.velocity_alpha), max_dt=float(m.cfg.est_max_dt),
                                 state=_p(m.est_state))
            d.est_dt = float(m.env.dt)
        h = C.c_void_p()
        N.check(L.quad_pop_create_deployed(C.byref(self.members[0]._fp.arch), arr, dep, P, batch,
                                           int(self.normalize_advantage), C.byref(h)), "quad_pop_create_deployed")
        return h

    def _start_member(self, m: PPO) -> None:
        m.last_obs.copy_(m.env.reset())
        m._start_estimators()
        m.last_start.fill_(1.0)
        m._started = True

    def _eval_run(self, i: int, e: QuadVecEnv, res: dict, verr: torch.Tensor) -> N.QuadPolicyRun:
        run = super()._eval_run(i, e, res, verr)
        cfg = self.members[i].cfg
        alpha = cfg.velocity_alpha if self._eval_alpha is None else self._eval_alpha
        run.obs_mode = N.OBS_DEPLOYED
        run.est = N.QuadVelEst(alpha=None, alpha_all=float(alpha), max_dt=float(cfg.est_max_dt), state=None)
        return run

    def evaluate(self, num_episodes: int = 10, seeds: Optional[Sequence[int]] = None,
                 max_episode_steps: Optional[int] = None,
                 velocity_alpha: Optional[float] = None) -> List[Optional[dict]]:
        """PopulationPPO.evaluate with every member's episodes flown on the deployed observation, each at the member's
        own velocity_alpha and est_max_dt, in one launch: what evaluate.evaluate_episodes(member.policy, ...,
        obs_mode="deployed", velocity_alpha=alpha) returns for member m. velocity_alpha: one coefficient for all
        members instead of their own (a policy trained at one alpha flown at another)."""
        self._eval_alpha = None if velocity_alpha is None else float(velocity_alpha)
        try:
            return super().evaluate(num_episodes, seeds, max_episode_steps)
        finally:
            self._eval_alpha = None


# ((H1, H2), activation) whose 64-member deployed iteration did not take less than half of 64 stand-alone deployed
# iterations in profiles/deployed_population/bench.json (by 18's bar): deployed_population_for keeps them
# off the population path
DEPLOYED_POPULATION_KEEP_SERIAL = frozenset()


def deployed_population_for(members: Sequence[Tuple[PPOConfig, int]], n_envs: int = 8, env: str = "hover",
                            wrapper: Optional[str] = None, device=None,
                            env_kwargs: Optional[dict] = None) -> DeployedPopulationPPO:
    """population_for for members with obs_mode="deployed": a DeployedPopulationPPO of the members' arch (the arch
    flags switched on in the configs it gets, for a net other than (128, 128) relu). ValueError for an env-mode member
    (by index), outside the family, for mixed arches, and for a row the drivers keep off the fused path
    (ARCH_ROLLOUT_KEEP_TORCH -- every deployed net collects on the family's rollout --, ARCH_UPDATE_KEEP_TORCH,
    DEPLOYED_POPULATION_KEEP_SERIAL)."""
    members = list(members)
    if len(members) < 1:
        raise ValueError("deployed_population_for needs at least one (PPOConfig, seed)")
    for k, (cfg, _) in enumerate(members):
        refuse_env_mode("deployed_population_for", k, cfg)
    keys = {_arch_key(cfg) for cfg, _ in members}
    if len(keys) != 1:
        raise ValueError(f"members must share net_arch and activation, got {sorted(keys)}")
    (hidden, act), = keys
    if not _in_family(hidden, act):
        raise ValueError(f"deployed_population_for trains {LEARNER_FAMILY}, got net_arch {hidden} {act}")
    small = (hidden, act) == ((128, 128), "relu")
    c0 = members[0][0]
    total = c0.n_steps * int(n_envs)
    batch = int(c0.batch_size) if c0.batch_size is not None else max(1, total // c0.n_minibatches)
    if (arch_rollout_keeps_torch(hidden, act, n_envs) or (not small and (hidden, act, batch) in ARCH_UPDATE_KEEP_TORCH)
            or (hidden, act) in DEPLOYED_POPULATION_KEEP_SERIAL):
        raise ValueError(f"net_arch {hidden} {act} stays off the deployed population path at {n_envs} envs, minibatch "
                         f"{batch} (it did not beat the path it would replace)")
    if not small:
        members = [(replace(cfg, fused_rollout_arch=True, fused_update_arch=True), seed) for cfg, seed in members]
    return DeployedPopulationPPO(members, n_envs=n_envs, env=env, wrapper=wrapper, device=device,
                                 env_kwargs=env_kwargs)
