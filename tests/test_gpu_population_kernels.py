"""Every population launch (quad_pop_*, csrc/population.hip) against the single launches it replaces.

A population kernel is the single kernel's body behind one more grid dimension (the block reads its member's
argument struct from a device table), so member m's outputs must equal a stand-alone launch on member m's
arguments BIT FOR BIT: every comparison here is on uint32 / raw-byte views, with no tolerance.

Two identical sets of three members (different weights, env seeds, noise seeds and scalars) are built from
the same seeds; set A is driven by the population launches, set B by the single launches
(FusedPolicy.pack / rollout / value, gae, quad_permutation, FusedLearner.adv_stats_epoch / grads,
FusedAdam.step). Shapes: 8 envs per member (less than one 32-env tile: shadow lanes) and 300 (two blocks, the
second partial); minibatches of 64 / 128 / 192 / 8,192 rows (1, 2, 3 rounds and the separate-block form's
limit) gathered through a permutation of a 16,384-row buffer (16,320 rows for 192, which does not divide
16,384: a population rejects a buffer that is no multiple of the minibatch); evaluation episodes
(quad_pop_episode) of 10 envs per member with max_episode_steps 40. With members {0, 2} active, member 1 is
byte-identical before and after every launch; every rejected-argument case returns QUAD_EINVAL with a message.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

P = 3
GAMMA = (0.97, 0.99, 0.95)
LAMBDA = (0.9, 0.95, 0.8)
CLIP = (0.2, 0.1, 0.3)
ENT = (1e-4, 1e-3, 0.0)
LR = (3e-4, 1e-3, 1e-4)


class Member:
    """One member's env, policy, optimizer and buffers; two Member(i, ...) are identical."""

    def __init__(self, i, n, rows, batch, kind="hover", wrapper=None, max_steps=None, grad_scale=1.0,
                 vf_coef=0.5, max_grad_norm=0.5):
        from uav_reinforcement_learning_control_amd import _native as N
        from uav_reinforcement_learning_control_amd.envs import QuadVecEnv
        from uav_reinforcement_learning_control_amd.ppo.fused import FusedPolicy
        from uav_reinforcement_learning_control_amd.ppo.learner import FusedAdam, FusedLearner, adam_state
        from uav_reinforcement_learning_control_amd.ppo.policy import ActorCritic
        self.i, self.n, self.rows, self.batch = i, n, rows, batch
        self.env = QuadVecEnv(n, env=kind, wrapper=wrapper, device="cuda:0", seed=5 + i, max_episode_steps=max_steps)
        torch.manual_seed(100 + i)
        self.pol = ActorCritic(12, 4, (128, 128)).cuda()
        with torch.no_grad():  # small weights + small std: episodes survive long enough to truncate
            for p in self.pol.parameters():
                p.copy_(torch.randn_like(p) * (0.3 / math.sqrt(max(p.shape[-1], 1))))
            self.pol.log_std.copy_(torch.tensor([-1.5, -2.0, -2.0, -2.5]) + 0.1 * i)
        self.fp = FusedPolicy(self.pol)
        self.fp.packed.zero_()  # (allocated uninitialised) comparable before the first pack
        self.lrn = FusedLearner(self.pol, CLIP[i], ENT[i], vf_coef, True)
        self.opt = torch.optim.Adam(list(self.pol.parameters()), lr=LR[i], eps=1e-5, fused=True)
        self.adam = FusedAdam(self.opt, max_grad_norm)
        self.vf_coef = vf_coef
        self.noise_seed = 0x1234_5678_9ABC + 977 * i
        f = dict(dtype=torch.float32, device="cuda")
        total = rows * n
        g = torch.Generator(device="cuda").manual_seed(1000 + i)
        r = lambda *s: torch.randn(*s, generator=g, **f)
        self.buf = dict(obs_copy=torch.rand(rows, n, 12, generator=g, **f) * 2 - 1, actions=0.5 * r(rows, n, 4),
                        log_prob=-3.0 + 0.1 * r(rows, n), value=r(rows, n), episode_starts=torch.zeros(rows, n, **f),
                        rewards=r(rows, n), last_obs=torch.zeros(n, 12, **f), last_start=torch.ones(n, **f),
                        ep_ret=torch.zeros(n, **f), ep_len=torch.zeros(n, **f),
                        stats=torch.zeros(N.POLICY_STAT_SLOTS, 3, dtype=torch.float64, device="cuda"))
        self.adv, self.ret = r(rows, n), grad_scale * r(rows, n)
        self.last_v, self.act_env = torch.zeros(1, n, **f), torch.zeros(n, 4, **f)
        self.perm = torch.zeros(total, dtype=torch.int64, device="cuda")
        self.nmb = total // batch if total % batch == 0 else 1
        self.sums = torch.zeros(self.nmb, N.ADV_SUM_DOUBLES, dtype=torch.float64, device="cuda")
        self.mb = torch.zeros(self.nmb, 4, **f)
        self.prm, self.grd = self.lrn._structs()
        adam_state(self.opt, self.adam.params)
        self.ws = None

    def fill(self, e, batch):
        """This member's QuadPopMember."""
        from uav_reinforcement_learning_control_amd import _native as N
        L = N.lib()
        ad = self.adam._build()
        if self.ws is None:
            need = max(int(L.quad_pop_workspace_bytes(C.byref(ad), min(batch, N.POP_MAX_BATCH))), 16)
            self.ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
        b = self.buf
        e.env, e.params, e.grads, e.adam, e.packed = self.env._h.value, self.prm, self.grd, ad, self.fp.packed.data_ptr()
        e.rollout = N.QuadRollout(**{k: v.data_ptr() for k, v in b.items()}, rows=self.rows, t0=0, steps=1,
                                  deterministic=0, seed=self.noise_seed, gamma=GAMMA[self.i])
        e.last_values, e.scratch_actions = self.last_v.data_ptr(), self.act_env.data_ptr()
        e.advantages, e.returns, e.perm = self.adv.data_ptr(), self.ret.data_ptr(), self.perm.data_ptr()
        e.adv_sums, e.mb_stats = self.sums.data_ptr(), self.mb.data_ptr()
        e.workspace, e.workspace_bytes = self.ws.data_ptr(), self.ws.numel()
        e.gae_lambda, e.clip_range, e.ent_coef, e.vf_coef = LAMBDA[self.i], CLIP[self.i], ENT[self.i], self.vf_coef

    def tensors(self):
        """Everything a launch can write, by name."""
        out = dict(self.buf)
        out.update(adv=self.adv, ret=self.ret, last_v=self.last_v, act_env=self.act_env, perm=self.perm,
                   sums=self.sums, mb=self.mb, packed=self.fp.packed)
        for k, p in enumerate(self.adam.params):
            st = self.opt.state[p]
            out.update({f"p{k}": p.data, f"g{k}": p.grad, f"m{k}": st["exp_avg"], f"v{k}": st["exp_avg_sq"],
                        f"t{k}": st["step"]})
        return out

    def snapshot(self):
        torch.cuda.synchronize()
        snap = {k: v.detach().cpu().contiguous().numpy().copy() for k, v in self.tensors().items()}
        snap.update({"env_" + k: np.asarray(v).copy() for k, v in self.env.get_state().items()})
        return snap


def raw(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def assert_same(sa, sb, what, keys=None):
    for k in (keys or sa.keys()):
        a, b = raw(sa[k]), raw(sb[k])
        assert a.shape == b.shape and np.array_equal(a, b), f"{what}: {k}: {int(np.sum(a != b))} bytes differ"


class Pop:
    def __init__(self, mems, batch, normalize=1):
        from uav_reinforcement_learning_control_amd import _native as N
        self.N, self.L = N, N.lib()
        arr = (N.QuadPopMember * len(mems))()
        for e, m in zip(arr, mems):
            m.fill(e, batch)
        self.arr, self.h = arr, C.c_void_p()
        self.rc = self.L.quad_pop_create(arr, len(mems), batch, normalize, C.byref(self.h))
        self.st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def subset(self, members):
        a, out = (C.c_int32 * len(members))(*members), C.c_int32(-1)
        rc = self.L.quad_pop_subset(self.h, a, len(members), C.byref(out))
        return rc, out.value

    def call(self, name, sid, *args):
        self.N.check(getattr(self.L, "quad_pop_" + name)(self.h, sid, *args, self.st), "quad_pop_" + name)

    def close(self):
        if self.h.value:
            self.L.quad_pop_destroy(self.h)
            self.h = C.c_void_p()


def _sets(**kw):
    return [Member(i, **kw) for i in range(P)], [Member(i, **kw) for i in range(P)]


def _perm_seeds():
    return [0x0123_4567_89AB_CDEF ^ (0x9E37_79B9 * (i + 1)) for i in range(P)]


def _single_rollout_part(m, chunks):
    from uav_reinforcement_learning_control_amd.ppo.gae import gae
    m.fp.pack()
    t = 0
    for k in chunks:
        m.fp.rollout(m.env, t0=t, steps=k, seed=m.noise_seed, gamma=GAMMA[m.i], **m.buf)
        t += k
    lv = m.fp.value(m.buf["last_obs"], m.last_v, m.act_env)
    b = m.buf
    gae(b["rewards"], b["value"], b["episode_starts"], lv, b["last_start"], GAMMA[m.i], LAMBDA[m.i], m.adv, m.ret)


def _pop_rollout_part(pop, sid, chunks):
    pop.call("pack", sid)
    t = 0
    for k in chunks:
        pop.call("rollout", sid, t, k)
        t += k
    pop.call("value", sid)
    pop.call("gae", sid)


def _single_update_part(m, seed, slots):
    from uav_reinforcement_learning_control_amd import _native as N
    total, B = m.rows * m.n, m.batch
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    N.check(N.lib().quad_permutation(total, seed, m.perm.data_ptr(), st), "quad_permutation")
    m.lrn.adv_stats_epoch(m.adv.view(total), m.perm, B, m.nmb, out=m.sums)
    b = m.buf
    norms = []
    for s in range(slots):
        m.lrn.grads(b["obs_copy"].view(total, 12), b["actions"].view(total, 4), b["log_prob"].view(total),
                    m.adv.view(total), m.ret.view(total), m.perm[s * B:(s + 1) * B], m.mb[s], adv_sums=m.sums[s])
        norms.append(float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in m.adam.params))))
        m.adam.step()
    return norms


def _pop_update_part(pop, sid, seeds, slots):
    sd = torch.tensor([s - (1 << 64) if s >= (1 << 63) else s for s in seeds], dtype=torch.int64).cuda()
    pop.call("permutation", sid, C.c_void_p(sd.data_ptr()))
    pop.call("adv_stats_epoch", sid)
    for s in range(slots):
        pop.call("ppo_grad", sid, s)
        pop.call("clip_adam", sid)
    torch.cuda.synchronize()


@pytest.mark.parametrize("kind,wrapper", [("hover", None), ("hover", "RateControlWrapper"),
                                          ("trajectory", None), ("trajectory", "RateControlWrapper")])
@pytest.mark.parametrize("n", [8, 300])
@pytest.mark.parametrize("nt", ["2", "1"])
def test_rollout_value_gae_match_single_launches(kind, wrapper, n, nt, monkeypatch):
    """pack, rollout (20 steps in two chunks), bootstrap value and GAE, T = 20."""
    monkeypatch.setenv("QUADENV_ROLLOUT_NT", nt)
    T, chunks = 20, (7, 13)
    # 6 for the 8-env members (24 envs in all: the shortest limit, so that some env reaches it), 7..11 for 300
    max_steps = 6 if n == 8 else 7 + (len(kind) + (3 if wrapper else 0) + int(nt)) % 5
    A, B = _sets(n=n, rows=T, batch=T * n, kind=kind, wrapper=wrapper, max_steps=max_steps)
    for m in A + B:
        m.buf["last_obs"].copy_(m.env.reset())
    pop = Pop(A, T * n)
    assert pop.rc == 0, pop.L.quad_last_error()
    _pop_rollout_part(pop, 0, chunks)
    for m in B:
        _single_rollout_part(m, chunks)
    truncs = 0
    for a, b in zip(A, B):
        sa, sb = a.snapshot(), b.snapshot()
        assert_same(sa, sb, f"member {a.i}")
        # the case exercised what it claims: resets in every member, and time-limit bootstraps in the population
        done = np.concatenate([sb["episode_starts"][1:], sb["last_start"][None]], 0)
        assert done.sum() > 0 and sb["stats"].sum(0)[2] == done.sum()
        length = np.zeros(n)
        for t in range(T):
            length += 1
            truncs += int(np.sum((done[t] == 1) & (length == max_steps)))
            length[done[t] == 1] = 0
    assert truncs > 0
    assert not np.array_equal(raw(A[0].snapshot()["rewards"]), raw(A[1].snapshot()["rewards"]))  # members differ
    pop.close()


@pytest.mark.parametrize("n", [8, 320])
def test_permutation_matches_single_launches(n):
    """The epoch permutation of n = 8 x 20 and of n = 6,400 rows, one key per member."""
    from uav_reinforcement_learning_control_amd import _native as N
    T = 20
    A, _ = [Member(i, n=n, rows=T, batch=T * n) for i in range(P)], None
    pop = Pop(A, T * n)
    assert pop.rc == 0, pop.L.quad_last_error()
    seeds = _perm_seeds()
    sd = torch.tensor(seeds, dtype=torch.int64).cuda()
    pop.call("permutation", 0, C.c_void_p(sd.data_ptr()))
    for m, s in zip(A, seeds):
        ref = torch.zeros(T * n, dtype=torch.int64, device="cuda")
        N.check(N.lib().quad_permutation(T * n, s, ref.data_ptr(), pop.st), "quad_permutation")
        assert torch.equal(ref, m.perm) and sorted(m.perm.tolist()) == list(range(T * n))
    assert not torch.equal(A[0].perm, A[1].perm)
    pop.close()


@pytest.mark.parametrize("batch", [64, 128, 192, 8192])
def test_update_matches_single_launches(batch):
    """Permutation, advantage statistics of the epoch, then two optimizer steps (gradient = prep + sep +
    reduce, clip + Adam) on minibatch slots 0 and 1 of a 16,384-row buffer. Member 0's value targets are
    scaled so that its gradient norm exceeds max_grad_norm (clipping acts); member 1's loss weights are
    small enough that it stays below (clipping does not act)."""
    n, rows = 8, 2048
    total = n * rows
    if total % batch:  # 192 does not divide 16,384: shorten the buffer to 85 x 192 = 16,320 rows
        rows = (total // batch) * batch // n
    kw = [dict(grad_scale=100.0), dict(grad_scale=1e-3, vf_coef=1e-4, max_grad_norm=50.0), dict()]
    A = [Member(i, n=n, rows=rows, batch=batch, **kw[i]) for i in range(P)]
    B = [Member(i, n=n, rows=rows, batch=batch, **kw[i]) for i in range(P)]
    pop = Pop(A, batch)
    assert pop.rc == 0, pop.L.quad_last_error()
    seeds = _perm_seeds()
    _pop_update_part(pop, 0, seeds, 2)
    norms = [_single_update_part(m, s, 2) for m, s in zip(B, seeds)]
    assert min(norms[0]) > 0.5 and max(norms[1]) < 50.0, norms  # clipping acts on member 0, not on member 1
    for a, b in zip(A, B):
        sa, sb = a.snapshot(), b.snapshot()
        assert_same(sa, sb, f"member {a.i}")
        assert float(sb["t0"]) == 2.0 and np.abs(sb["mb"][:2]).sum() > 0 and np.abs(sb["g2"]).sum() > 0
    pop.close()


def test_members_outside_the_subset_are_untouched():
    """With members {0, 2} active, every launch leaves member 1 byte-identical (parameters, Adam state,
    buffers, env state) and members 0 and 2 equal to their single launches."""
    n, T = 8, 20
    A, B = _sets(n=n, rows=T, batch=40, max_steps=7)
    for m in A + B:
        m.buf["last_obs"].copy_(m.env.reset())
        m.fp.pack()
    pop = Pop(A, 40)
    assert pop.rc == 0, pop.L.quad_last_error()
    rc, sid = pop.subset([0, 2])
    assert rc == 0 and sid == 1
    before = A[1].snapshot()
    seeds = _perm_seeds()
    steps = [lambda: _pop_rollout_part(pop, sid, (20,)), lambda: _pop_update_part(pop, sid, seeds, 4)]
    for step in steps:
        step()
        assert_same(before, A[1].snapshot(), "inactive member 1")
    for i in (0, 2):
        _single_rollout_part(B[i], (20,))
        _single_update_part(B[i], seeds[i], 4)
        assert_same(A[i].snapshot(), B[i].snapshot(), f"member {i}")
    pop.close()


@pytest.mark.parametrize("kind,wrapper", [("hover", None), ("trajectory", "RateControlWrapper")])
def test_policy_episode_matches_single_launches(kind, wrapper):
    """quad_pop_episode: 10 envs per member, max_episode_steps 40 -- returns, lengths, every other metric and the
    final env state against FusedPolicy.episode per member; with {0, 2} active member 1's handle and metrics stay."""
    from uav_reinforcement_learning_control_amd import _native as N
    from uav_reinforcement_learning_control_amd.envs import QuadVecEnv
    n, T = 10, 40
    A = [Member(i, n=8, rows=20, batch=160, kind=kind, wrapper=wrapper) for i in range(P)]
    for m in A:
        m.fp.pack()
    mk = lambda i: QuadVecEnv(n, env=kind, wrapper=wrapper, device="cuda:0", seed=70 + i, max_episode_steps=T,
                              auto_reset=False)
    ea, eb = [mk(i) for i in range(P)], [mk(i) for i in range(P)]
    for e in ea + eb:
        e.reset()
    pop = Pop(A, 160)
    assert pop.rc == 0, pop.L.quad_last_error()
    res = {k: torch.full((P, n), -5, dtype=getattr(torch, dt), device="cuda") for k, dt in N.PID_METRIC_FIELDS}
    verr = torch.full((P, n), -5.0, dtype=torch.float64, device="cuda")
    arr = (N.QuadPopEval * P)()
    for i, e in enumerate(ea):
        arr[i].env = e._h.value
        arr[i].run = N.QuadPolicyRun(obs_mode=N.OBS_ENV, max_steps=T, trace_envs=0,
                                     est=N.QuadVelEst(alpha=None, alpha_all=0.8, max_dt=0.1, state=None),
                                     est_dt=float(e.dt),
                                     metrics=N.QuadPidMetrics(**{k: res[k][i].data_ptr() for k, _ in N.PID_METRIC_FIELDS}),
                                     vel_err_sq=verr[i].data_ptr())
    L = pop.L
    assert L.quad_pop_episode(pop.h, 0, pop.st) == N.QUAD_EINVAL and b"attach" in L.quad_last_error()
    arr[1].run.obs_mode = N.OBS_DEPLOYED
    assert L.quad_pop_attach_eval(pop.h, arr) == N.QUAD_EINVAL and b"obs_mode" in L.quad_last_error()
    arr[1].run.obs_mode = N.OBS_ENV
    arr[2].run.max_steps = T - 1
    assert L.quad_pop_attach_eval(pop.h, arr) == N.QUAD_EINVAL and b"max_steps" in L.quad_last_error()
    arr[2].run.max_steps = T
    N.check(L.quad_pop_attach_eval(pop.h, arr), "quad_pop_attach_eval")
    rc, sid = pop.subset([0, 2])
    assert rc == 0
    s1 = ea[1].get_state()
    pop.call("episode", sid)
    torch.cuda.synchronize()
    assert bool((res["steps"][1] == -5).all()) and bool((verr[1] == -5.0).all())
    for k, v in ea[1].get_state().items():
        assert np.array_equal(raw(np.asarray(v)), raw(np.asarray(s1[k]))), k
    rc, sid1 = pop.subset([1])
    assert rc == 0
    pop.call("episode", sid1)
    torch.cuda.synchronize()
    for i in range(P):
        ref = A[i].fp.episode(eb[i], max_steps=T)
        torch.cuda.synchronize()
        for k, _ in N.PID_METRIC_FIELDS:
            assert np.array_equal(raw(res[k][i].cpu().numpy()), raw(ref[k].cpu().numpy())), (i, k)
        assert np.array_equal(raw(verr[i].cpu().numpy()), raw(ref["vel_err_sq"].cpu().numpy())), i
        sa, sb = ea[i].get_state(), eb[i].get_state()
        for k in sa:
            assert np.array_equal(raw(np.asarray(sa[k])), raw(np.asarray(sb[k]))), (i, k)
    assert not np.array_equal(res["total_reward"][0].cpu().numpy(), res["total_reward"][1].cpu().numpy())
    # a member without a handle has no entry: a subset that holds it is rejected; after detach every launch is
    arr[1].env = None
    N.check(L.quad_pop_attach_eval(pop.h, arr), "quad_pop_attach_eval")
    keep = {k: v.clone() for k, v in res.items()}
    assert L.quad_pop_episode(pop.h, 0, pop.st) == N.QUAD_EINVAL and b"no evaluation handle" in L.quad_last_error()
    assert L.quad_pop_episode(pop.h, sid1, pop.st) == N.QUAD_EINVAL
    assert L.quad_pop_detach_eval(pop.h) == 0
    assert L.quad_pop_episode(pop.h, sid, pop.st) == N.QUAD_EINVAL and b"attach" in L.quad_last_error()
    torch.cuda.synchronize()
    assert all(torch.equal(keep[k], res[k]) for k in res)
    assert int(res["steps"][1].max()) <= T and int(res["steps"][1].min()) >= 1
    pop.close()


def test_rejected_arguments_launch_nothing():
    """Every rejected-argument case returns QUAD_EINVAL with a message and leaves the outputs untouched."""
    from uav_reinforcement_learning_control_amd import _native as N
    from uav_reinforcement_learning_control_amd.envs import QuadVecEnv
    n, T, batch = 8, 20, 40
    A = [Member(i, n=n, rows=T, batch=batch) for i in range(P)]
    L = N.lib()

    def rejected(mems, b, word, count=None, edit=None):
        arr = (N.QuadPopMember * len(mems))()
        for e, m in zip(arr, mems):
            m.fill(e, batch)
        if edit:
            edit(arr)
        h = C.c_void_p(1)
        rc = L.quad_pop_create(arr, len(mems) if count is None else count, b, 1, C.byref(h))
        assert rc == N.QUAD_EINVAL and not h.value, (word, rc)
        assert word.encode() in L.quad_last_error(), (word, L.quad_last_error())

    before = [m.snapshot() for m in A]
    rejected(A, batch, "P must be >= 1", count=0)
    rejected(A, 8193, "batch")
    rejected(A, 0, "batch")
    rejected(A, 48, "multiple")                                        # 160 rows, minibatch 48
    rejected(A[:2] + [Member(2, n=16, rows=T, batch=batch)], batch, "differ")   # envs per member differ
    rejected(A[:2] + [Member(2, n=n, rows=10, batch=batch)], batch, "differ")   # rows differ
    rejected(A[:2] + [Member(2, n=n, rows=T, batch=batch, wrapper="RateControlWrapper")], batch, "differ")
    rejected(A[:2] + [Member(2, n=n, rows=T, batch=batch, max_steps=9)], batch, "differ")  # constants differ
    for field in ("env", "packed", "advantages", "perm", "workspace", "last_values"):
        rejected(A, batch, "NULL", edit=lambda arr, f=field: setattr(arr[1], f, None))
    rejected(A, batch, "NULL", edit=lambda arr: setattr(arr[2].rollout, "rewards", None))
    rejected(A, batch, "NULL", edit=lambda arr: setattr(arr[0].params, "pi_w1", None))
    rejected(A, batch, "NULL", edit=lambda arr: setattr(arr[0].grads, "log_std", None))
    rejected(A, batch, "workspace too small", edit=lambda arr: setattr(arr[0], "workspace_bytes", 1024))
    rejected(A, batch, "clip_range", edit=lambda arr: setattr(arr[0], "clip_range", 0.0))
    # an env kind / wrapper quad_rollout rejects, and a handle without auto-reset
    for env, word in ((QuadVecEnv(n, wrapper="RelPosActWrapper", device="cuda:0"), "12-D"),
                      (QuadVecEnv(n, env="brax_hover", device="cuda:0"), "env_kind"),
                      (QuadVecEnv(n, device="cuda:0", auto_reset=False), "auto_reset")):
        rejected(A, batch, word, edit=lambda arr, e=env: setattr(arr[1], "env", e._h.value))
    # subsets and launch arguments of a valid population
    pop = Pop(A, batch)
    assert pop.rc == 0, L.quad_last_error()
    for members, word in (([], "empty"), ([0, 3], "out of range"), ([-1], "out of range"), ([0, 2, 0], "duplicate")):
        rc, _ = pop.subset(members)
        assert rc == N.QUAD_EINVAL and word.encode() in L.quad_last_error(), (members, L.quad_last_error())
    for name, args in (("pack", (7,)), ("rollout", (7, 0, 1)), ("rollout", (0, 0, 0)), ("rollout", (0, -1, 1)),
                       ("value", (-1,)), ("gae", (7,)), ("permutation", (0, None)), ("adv_stats_epoch", (7,)),
                       ("ppo_grad", (0, 4)), ("ppo_grad", (0, -1)), ("clip_adam", (7,))):
        rc = getattr(L, "quad_pop_" + name)(pop.h, *args, pop.st)
        assert rc == N.QUAD_EINVAL and len(L.quad_last_error()) > 0, (name, args, rc)
    for a, b in zip(before, [m.snapshot() for m in A]):
        assert_same(a, b, "after rejected calls")
    pop.close()
