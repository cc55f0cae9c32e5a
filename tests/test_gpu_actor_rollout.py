"""The general family's rollout on the GPU (csrc/actor_rollout.hip: quad_actor_critic_pack / act / post and
quad_actor_rollout, ppo/fused.py FusedActorCritic, PPOConfig.fused_rollout_arch, train --fused-arch-rollout).

1. The per-step kernel: the mean is quad_actor_act's to the bit, the value and the log-prob meet the float64 bars
   with torch fp32 as the yardstick.  2. Its noise is quad_policy_act's.  3. The one-launch rollout is
   bit-identical to the two-launch form, and  4. so is the deterministic one.  5. A refusal writes nothing.
   6. PPO collects the same bits on both forms and resumes from a checkpoint.  7. The driver learns with the flags.
"""
import copy
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

from uav_reinforcement_learning_control_amd import _native as N

pytestmark = pytest.mark.gpu

KEYS = ("obs_copy", "actions", "log_prob", "value", "episode_starts", "rewards", "last_obs", "last_start", "ep_ret",
        "ep_len")


def _policy(h1, h2, act, seed=0):
    """test_gpu_rollout._policy's recipe for an arch: small weights and a small std, so that episodes survive long
    enough to truncate."""
    from uav_reinforcement_learning_control_amd.ppo.policy import ActorCritic
    torch.manual_seed(seed)
    pol = ActorCritic(12, 4, (h1, h2), activation=act).cuda()
    with torch.no_grad():
        for p in pol.parameters():
            p.copy_(torch.randn_like(p) * (0.3 / math.sqrt(max(p.shape[-1], 1))))
        pol.log_std.copy_(torch.tensor([-1.5, -2.0, -2.0, -2.5]))
    return pol


def _fused(pol):
    from uav_reinforcement_learning_control_amd.ppo.fused import FusedActorCritic
    fp = FusedActorCritic(pol)
    fp.pack()
    return fp


def _env(n, kind, wrapper, max_steps, seed=5, base=0, **kw):
    from uav_reinforcement_learning_control_amd.envs import QuadVecEnv
    return QuadVecEnv(n, env=kind, wrapper=wrapper, device="cuda:0", seed=seed, env_id_base=base,
                      max_episode_steps=max_steps, **kw)


def _bufs(T, n):
    f = dict(dtype=torch.float32, device="cuda")
    return dict(obs_copy=torch.full((T, n, 12), -7.0, **f), actions=torch.full((T, n, 4), -7.0, **f),
                log_prob=torch.full((T, n), -7.0, **f), value=torch.full((T, n), -7.0, **f),
                episode_starts=torch.full((T, n), -7.0, **f), rewards=torch.full((T, n), -7.0, **f),
                last_obs=torch.zeros(n, 12, **f), last_start=torch.ones(n, **f),
                ep_ret=torch.zeros(n, **f), ep_len=torch.zeros(n, **f),
                stats=torch.zeros(N.POLICY_STAT_SLOTS, 3, dtype=torch.float64, device="cuda"))


def _two_launch(fp, env, b, T, seed, gamma, deterministic=False):
    """quad_actor_critic_act with the epilogue + quad_step per step, then quad_actor_critic_post. Returns the raw
    env rewards [T, n]."""
    cur = torch.zeros(4, dtype=torch.int32, device="cuda")
    act_env = torch.zeros(env.num_envs, 4, device="cuda")
    epi = fp.make_epilogue(env.reward, env.terminated, env.truncated, env.terminal_obs, b["rewards"],
                           b["last_start"], b["ep_ret"], b["ep_len"], b["stats"], T, gamma)
    raw = []
    for _ in range(T):
        fp.act(b["last_obs"], act_env, actions=b["actions"], log_prob=b["log_prob"], value=b["value"],
               obs_copy=b["obs_copy"], last_start=b["last_start"], episode_starts=b["episode_starts"],
               cursor=cur, rows=T, seed=seed, env_id_base=env.env_id_base, deterministic=deterministic,
               epilogue=epi)
        env.step(act_env, obs=b["last_obs"], info="raw")
        raw.append(env.reward.clone())
    fp.post(epi, cur)
    torch.cuda.synchronize()
    return torch.stack(raw)


def _one_launch(fp, env, b, T, seed, gamma, chunks, deterministic=False):
    t = 0
    for k in chunks:
        fp.rollout(env, t0=t, steps=k, seed=seed, gamma=gamma, deterministic=deterministic, **b)
        t += k
    assert t == T
    torch.cuda.synchronize()


def _assert_same_bits(A, B, ea, eb):
    for k in KEYS:
        a, b = A[k].cpu().numpy(), B[k].cpu().numpy()
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), \
            f"{k}: {np.sum(a.view(np.uint32) != b.view(np.uint32))} words differ"
    sa, sb = ea.get_state(), eb.get_state()
    for k, v in sa.items():
        assert np.array_equal(np.asarray(v).view(np.uint32), np.asarray(sb[k]).view(np.uint32)), k
    np.testing.assert_allclose(B["stats"].sum(0).cpu().numpy(), A["stats"].sum(0).cpu().numpy(), rtol=1e-6)


def _obs(n, seed=7):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(n, 12, generator=g) * 2 - 1).cuda()


def _act(fp, obs, *, t=0, seed=0x51F15EED, base=0, deterministic=False):
    """(actions, log_prob, value, actions_env) of one quad_actor_critic_act / quad_policy_act launch at step t."""
    n = obs.shape[0]
    f = dict(dtype=torch.float32, device="cuda")
    out = dict(actions=torch.empty(1, n, 4, **f), log_prob=torch.empty(1, n, **f), value=torch.empty(1, n, **f))
    env = torch.empty(n, 4, **f)
    cur = torch.tensor([t, 0, 0, 0], dtype=torch.int32, device="cuda")
    fp.act(obs, env, cursor=cur, rows=1, seed=seed, env_id_base=base, deterministic=deterministic, **out)
    torch.cuda.synchronize()
    assert cur.tolist() == [t, 0, 0, 0]  # read-only without an epilogue
    return out["actions"][0], out["log_prob"][0], out["value"][0], env


# ---------------------------------------------------------------- 1. per-step accuracy
@pytest.mark.parametrize("h1,h2,act", [(64, 64, "tanh"), (96, 64, "relu"), (256, 256, "tanh"), (512, 256, "relu")])
def test_per_step_mean_bits_and_float64_bars(h1, h2, act):
    """1,024 rows. The mean (deterministic = 1: actions == mean) is quad_actor_act's, bit for bit; value against
    float64 torch is within 4x torch fp32's own error; log_prob against float64 policy.log_prob on the kernel's own
    (mean, action) is within 4x torch fp32's error on the same inputs; actions_env = clip(actions).

    The RATIO lines (pytest -s) are the measured kernel error / torch fp32 error; DESIGN 24 records them."""
    from uav_reinforcement_learning_control_amd.ppo.fused import FusedActor
    pol = _policy(h1, h2, act)
    fp = _fused(pol)
    obs = _obs(1024)
    n = obs.shape[0]
    mean, lp_det, _, env_det = _act(fp, obs, deterministic=True)
    fa = FusedActor(pol)
    fa.pack()
    want_mean, want_env = torch.empty(n, 4, device="cuda"), torch.empty(n, 4, device="cuda")
    fa.act(obs, want_env, want_mean)
    assert torch.equal(mean.view(torch.int32), want_mean.view(torch.int32))
    assert torch.equal(env_det.view(torch.int32), want_env.view(torch.int32))
    # the actor half of the image is quad_actor_pack's image
    assert torch.equal(fp.packed[:fa.packed.numel()].view(torch.int32), fa.packed.view(torch.int32))
    a, lp, val, env = _act(fp, obs)
    assert torch.equal(env, a.clamp(-1, 1)) and not torch.equal(a, mean)
    p64 = copy.deepcopy(pol).double()
    with torch.no_grad():
        v64 = p64.forward_heads(obs.double())[1]
        v32 = pol.forward_heads(obs)[1]
        lp64 = p64.log_prob(mean.double(), a.double())
        lp32 = pol.log_prob(mean, a)
    err, err32 = (val.double() - v64).abs().max().item(), (v32.double() - v64).abs().max().item()
    print(f"RATIO {h1}x{h2} {act} value: err {err:.3g} torch32 {err32:.3g} ratio {err / err32:.2f}")
    assert err <= 4 * err32, (err, err32)
    err, err32 = (lp.double() - lp64).abs().max().item(), (lp32.double() - lp64).abs().max().item()
    print(f"RATIO {h1}x{h2} {act} log_prob: err {err:.3g} torch32 {err32:.3g} ratio {err / err32:.2f}")
    assert err <= 4 * err32, (err, err32)
    # the value row does not depend on the draw
    assert torch.equal(_act(fp, obs, deterministic=True)[2].view(torch.int32), val.view(torch.int32))


def test_the_clip_is_exercised_in_both_forms():
    """The recipe's actions stay inside the box (means near 0.1, sd at most 0.22), so a kernel that forgot the clip
    would pass the tests above. With log_std = (0.3, 0, -0.5, 0.2) a good share of the samples leave [-1, 1]:
    actions_env is the clip of the stored action, per step; and the one-launch form, whose envs receive its own
    clipped actions, stays bit-identical to the two-launch form, whose quad_step receives actions_env."""
    pol = _policy(64, 64, "tanh")
    with torch.no_grad():
        pol.log_std.copy_(torch.tensor([0.3, 0.0, -0.5, 0.2]))
    fp = _fused(pol)
    a, _, _, env = _act(fp, _obs(1024))
    outside = (a.abs() > 1).float().mean().item()
    assert 0.2 < outside < 0.8 and (a > 1).any() and (a < -1).any()
    assert torch.equal(env, a.clamp(-1, 1)) and env.abs().max().item() == 1.0
    n, T, seed, gamma = 40, 8, 0xABCDEF, 0.97
    ea, eb = _env(n, "hover", "RateControlWrapper", 6, base=n), _env(n, "hover", "RateControlWrapper", 6, base=n)
    A, B = _bufs(T, n), _bufs(T, n)
    A["last_obs"].copy_(ea.reset())
    B["last_obs"].copy_(eb.reset())
    _two_launch(fp, ea, A, T, seed, gamma)
    _one_launch(fp, eb, B, T, seed, gamma, (3, 5))
    _assert_same_bits(A, B, ea, eb)
    assert (B["actions"].abs() > 1).float().mean().item() > 0.2


# ---------------------------------------------------------------- 2. the noise
def test_noise_is_quad_policy_acts():
    """z = (a - mean) / sd recovered from quad_actor_critic_act on a (64, 64) tanh net and from quad_policy_act on a
    128-128 ReLU net, same seed, env ids and t: the same draw. Bound: a is the f32 rounding of mean + sd z, formed in
    at most two roundings (the product, the sum) of numbers no larger than M = max(|a|, |mean|, |a - mean|), so
    |a - (mean + sd z)| <= 2 ulp(M) and the recovered z is off by at most 2 ulp(M) / sd on each side; the test's own
    float64 sd is the same on both sides and cancels."""
    from uav_reinforcement_learning_control_amd.ppo.fused import FusedPolicy
    n, t, base, seed = 200, 12345, 977, 0xC0FFEE_1234
    obs = _obs(n, seed=9)
    fa = _fused(_policy(64, 64, "tanh"))
    fb = FusedPolicy(_policy(128, 128, "relu", seed=1))
    fb.pack()
    sd = torch.tensor([-1.5, -2.0, -2.0, -2.5], dtype=torch.float32).double().exp().cuda()
    zs, bounds = [], []
    for f in (fa, fb):
        mean = _act(f, obs, t=t, seed=seed, base=base, deterministic=True)[0].double()
        a = _act(f, obs, t=t, seed=seed, base=base)[0].double()
        zs.append((a - mean) / sd)
        M = torch.maximum(torch.maximum(a.abs(), mean.abs()), (a - mean).abs()).max().item()
        bounds.append(2 * float(np.spacing(np.float32(M))) / sd)
    bound = bounds[0] + bounds[1]
    assert ((zs[0] - zs[1]).abs() <= bound).all(), ((zs[0] - zs[1]).abs().max(0).values, bound)
    assert 0.8 < zs[0].std().item() < 1.2 and abs(zs[0].mean().item()) < 0.2   # and it is a draw
    # the draw changes with t and with env_id_base
    a0 = _act(fa, obs, t=t, seed=seed, base=base)[0]
    assert not torch.equal(a0, _act(fa, obs, t=t + 1, seed=seed, base=base)[0])
    assert not torch.equal(a0, _act(fa, obs, t=t, seed=seed, base=base + 1)[0])
    # a shard is rows k.. of the whole: same bits in every output
    k = 77
    whole, shard = _act(fa, obs, t=t, seed=seed, base=base), _act(fa, obs[k:].contiguous(), t=t, seed=seed, base=base + k)
    for w, s in zip(whole, shard):
        assert torch.equal(w[k:].view(torch.int32), s.view(torch.int32))


# ---------------------------------------------------------------- 3. one launch against two launches
CASES = [
    ((64, 64, "tanh"), "hover", None, 6, 97, (20,)),
    ((256, 256, "tanh"), "hover", "RateControlWrapper", 9, 130, (7, 13)),
    ((512, 256, "relu"), "trajectory", "RateControlWrapper", 11, 70, (5, 5, 10)),
    ((128, 128, "tanh"), "trajectory", None, 6, 33, (20,)),
    # a last block of at most 32 envs is split between its waves (policy net / value net): the cases above hold
    # one at MB = 8 (130 and 70 envs); these hold one at MB = 2 (the only block) and at MB = 4
    ((96, 64, "relu"), "hover", "RateControlWrapper", 6, 16, (9, 11)),
    ((128, 128, "tanh"), "trajectory", None, 6, 80, (20,)),
]


@pytest.mark.parametrize("arch,kind,wrapper,max_steps,n,chunks", CASES,
                         ids=[f"{a[0]}x{a[1]}-{a[2]}-{k}-{'ctbr' if w else 'none'}" for a, k, w, *_ in CASES])
def test_one_launch_rollout_is_bit_identical(arch, kind, wrapper, max_steps, n, chunks):
    T, seed, gamma = sum(chunks), 0x1234_5678_9ABC, 0.97
    fp = _fused(_policy(*arch))
    ea, eb = _env(n, kind, wrapper, max_steps, base=3 * n), _env(n, kind, wrapper, max_steps, base=3 * n)
    A, B = _bufs(T, n), _bufs(T, n)
    A["last_obs"].copy_(ea.reset())
    B["last_obs"].copy_(eb.reset())
    raw = _two_launch(fp, ea, A, T, seed, gamma)
    _one_launch(fp, eb, B, T, seed, gamma, chunks)
    _assert_same_bits(A, B, ea, eb)
    # the case exercised what it claims: resets, time-limit truncations, bootstrapped reward rows
    tb = B["stats"].sum(0).cpu().numpy()
    starts, last = B["episode_starts"].cpu().numpy(), B["last_start"].cpu().numpy()
    done = np.concatenate([starts[1:], last[None]], 0)  # done[t] = env finished at step t
    assert done.sum() > 0 and tb[2] == done.sum()
    length, truncs = np.zeros(n), np.zeros((T, n), bool)
    for t in range(T):
        length += 1
        truncs[t] = (done[t] == 1) & (length == max_steps)
        length[done[t] == 1] = 0
    assert truncs.sum() > 0
    differs = (B["rewards"] != raw).cpu().numpy()
    assert differs.any() and not differs[~truncs].any()
    assert not (B["obs_copy"] == -7).any() and not (B["value"] == -7).any()


# ---------------------------------------------------------------- 4. the deterministic rollout
def test_deterministic_rollout_is_bit_identical_and_unnoised():
    from uav_reinforcement_learning_control_amd.ppo.fused import FusedActor
    arch, kind, wrapper, max_steps, n, chunks = (256, 256, "tanh"), "hover", "RateControlWrapper", 9, 130, (7, 13)
    T, seed, gamma = sum(chunks), 0x1234_5678_9ABC, 0.97
    pol = _policy(*arch)
    fp = _fused(pol)
    ea, eb = _env(n, kind, wrapper, max_steps, base=3 * n), _env(n, kind, wrapper, max_steps, base=3 * n)
    A, B = _bufs(T, n), _bufs(T, n)
    A["last_obs"].copy_(ea.reset())
    B["last_obs"].copy_(eb.reset())
    _two_launch(fp, ea, A, T, seed, gamma, deterministic=True)
    _one_launch(fp, eb, B, T, seed, gamma, chunks, deterministic=True)
    _assert_same_bits(A, B, ea, eb)
    assert B["last_start"].sum().item() + B["episode_starts"][1:].sum().item() > 0   # episodes ended
    # no noise: the stored actions are quad_actor_act's mean of the stored observations
    fa = FusedActor(pol)
    fa.pack()
    mean, env = torch.empty(T * n, 4, device="cuda"), torch.empty(T * n, 4, device="cuda")
    fa.act(B["obs_copy"].reshape(T * n, 12), env, mean)
    assert torch.equal(mean.view(torch.int32), B["actions"].reshape(T * n, 4).view(torch.int32))
    # z = 0 exactly, so every log_prob is the same number: four terms -log_std[k] - 0.5 log(2 pi), each
    # rounded twice and summed in f32 (partial sums below 8: at most 8 half-ulps of 4.77e-7)
    lp = B["log_prob"].cpu().numpy()
    const = -float(pol.log_std.detach().double().sum()) - 4 * 0.5 * math.log(2 * math.pi)
    assert np.unique(lp).size == 1
    assert abs(float(lp.flat[0]) - const) <= 8 * 0.5 * 4.77e-7


# ---------------------------------------------------------------- 5. refusals
def test_a_refusal_launches_nothing_and_writes_nothing():
    L = N.lib()
    n, T = 40, 4
    pol = _policy(64, 64, "tanh")
    fp = _fused(pol)
    good = _env(n, "hover", None, 6)
    envs = dict(good=good, brax=_env(n, "brax_hover", None, 6), noreset=_env(n, "hover", None, 6, auto_reset=False),
                relpos=_env(n, "hover", "RelPosActWrapper", 6))
    for k, e in envs.items():
        if k != "good":
            e.reset()
    b = _bufs(T, n)
    b["last_obs"].copy_(good.reset())
    carry = {k: b[k].clone() for k in ("last_obs", "last_start", "ep_ret", "ep_len", "stats")}
    torch.cuda.synchronize()
    states = {k: e.get_state() for k, e in envs.items()}
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def roll(env="good", arch=fp.arch, packed=fp.packed.data_ptr(), **over):
        f = dict(rows=T, t0=0, steps=T, deterministic=0, seed=1, gamma=0.97, **{k: b[k].data_ptr() for k in KEYS},
                 stats=b["stats"].data_ptr())
        f.update(over)
        r = N.QuadRollout(**f)
        return L.quad_actor_rollout(envs[env]._h if env else None, C.byref(arch) if arch is not None else None, packed,
                                    C.byref(r), stream)

    refused = [roll(arch=N.QuadActorArch(h1=48, h2=64, activation=0)), roll(arch=N.QuadActorArch(h1=64, h2=64, activation=2)),
               roll(arch=N.QuadActorArch(h1=544, h2=64, activation=0)), roll(arch=None), roll(env=None),
               roll(env="brax"), roll(env="noreset"), roll(env="relpos"), roll(rows=0), roll(steps=0), roll(t0=-1),
               roll(packed=None), roll(actions=b["actions"].data_ptr() + 4), roll(packed=fp.packed.data_ptr() + 4)]
    refused += [roll(**{k: None}) for k in KEYS + ("stats",)]
    assert refused == [N.QUAD_EINVAL] * len(refused)
    # the per-step entry points' refusals
    act_env = torch.full((n, 4), -7.0, device="cuda")
    cur = torch.zeros(4, dtype=torch.int32, device="cuda")
    epi = fp.make_epilogue(good.reward, good.terminated, good.truncated, good.terminal_obs, b["rewards"],
                           b["last_start"], b["ep_ret"], b["ep_len"], b["stats"], T, 0.97)

    def act(arch=fp.arch, packed=fp.packed.data_ptr(), n_=n, **over):
        f = dict(obs=b["last_obs"].data_ptr(), actions_env=act_env.data_ptr(), actions=b["actions"].data_ptr(),
                 log_prob=b["log_prob"].data_ptr(), value=b["value"].data_ptr(), obs_copy=b["obs_copy"].data_ptr(),
                 last_start=b["last_start"].data_ptr(), episode_starts=b["episode_starts"].data_ptr(),
                 cursor=cur.data_ptr(), rows=T, deterministic=0, seed=1, env_id_base=0, epilogue=C.pointer(epi))
        f.update(over)
        a = N.QuadPolicyAct(**f)
        return L.quad_actor_critic_act(C.byref(arch), packed, C.byref(a), n_, stream)

    bad_epi = N.QuadRolloutPost.from_buffer_copy(epi)
    bad_epi.rows = T + 1
    refused = [act(arch=N.QuadActorArch(h1=48, h2=64, activation=0)), act(packed=None), act(obs=None), act(actions_env=None),
               act(n_=0), act(rows=0), act(cursor=None), act(actions=b["actions"].data_ptr() + 4),
               act(epilogue=C.pointer(bad_epi)),
               L.quad_actor_critic_post(C.byref(fp.arch), fp.packed.data_ptr(), C.byref(epi), None, n, stream),
               L.quad_actor_critic_post(C.byref(fp.arch), None, C.byref(epi), cur.data_ptr(), n, stream),
               L.quad_actor_critic_post(C.byref(fp.arch), fp.packed.data_ptr(), C.byref(epi), cur.data_ptr(), 0, stream),
               L.quad_actor_critic_pack(C.byref(fp.arch), None, fp.packed.data_ptr(), stream)]
    assert refused == [N.QUAD_EINVAL] * len(refused)
    torch.cuda.synchronize()
    for k in KEYS[:6]:
        assert (b[k] == -7).all(), k
    assert (act_env == -7).all() and cur.tolist() == [0, 0, 0, 0]
    for k, v in carry.items():
        assert torch.equal(b[k], v), k
    for name, e in envs.items():
        for k, v in e.get_state().items():
            assert np.array_equal(np.asarray(v).view(np.uint32), np.asarray(states[name][k]).view(np.uint32)), (name, k)
    # and the same arguments, unchanged, are accepted
    assert roll() == N.QUAD_OK
    torch.cuda.synchronize()
    assert not (b["rewards"] == -7).any()


# ---------------------------------------------------------------- 6. PPO wiring
def _ppo(one_launch, n=97, T=16, seed=3, env_seed=11):
    from uav_reinforcement_learning_control_amd.ppo.ppo import PPO, PPOConfig
    env = _env(n, "hover", None, 8, seed=env_seed)
    cfg = PPOConfig(net_arch=(64, 64), activation="tanh", n_steps=T, n_epochs=1, n_minibatches=4,
                    fused_rollout_arch=True, fused_rollout=one_launch)
    ppo = PPO(env, cfg, seed=seed)
    with torch.no_grad():  # a critic that is not zero, a std that keeps episodes alive
        for p in ppo.policy.parameters():
            p.copy_(torch.randn_like(p) * (0.3 / math.sqrt(max(p.shape[-1], 1))))
        ppo.policy.log_std.copy_(torch.tensor([-1.5, -2.0, -2.0, -2.5]))
    return ppo


BUFS = ("buf_obs", "buf_act", "buf_logp", "buf_val", "buf_rew", "buf_start", "buf_adv", "buf_ret")


def _restart(ppo, state, obs0):
    """Put the env, the carry tensors and both noise counters back to the start of a first rollout."""
    torch.cuda.synchronize()
    ppo.env.set_state(**state)
    ppo.last_obs.copy_(obs0)
    ppo.last_start.fill_(1.0)
    ppo.ep_ret.zero_()
    ppo.ep_len.zero_()
    ppo._cursor.zero_()
    ppo._t_host = 0


def test_ppo_collects_the_same_bits_on_every_form():
    """collect_rollouts through quad_actor_rollout (fused_rollout=True) and through the two-launch form
    (fused_rollout=False), the latter replayed from its hipGraph and eager: the same bits in all eight buffers.
    The graph capture steps the env once before the first rollout (test_gpu_rollout's note), so every form first
    collects one rollout (which captures) and is then put back to one common start: the env state and observation
    of a twin env's first reset, fresh carry tensors, noise counter 0. And the rows against an independent forward:
    float64 forward_heads of the stored observations reproduces buf_val within 4x torch fp32's error, float64
    log_prob at the stored actions reproduces buf_logp likewise."""
    from uav_reinforcement_learning_control_amd.ppo.fused import FusedActorCritic
    twin = _env(97, "hover", None, 8, seed=11)
    obs0 = twin.reset().clone()
    torch.cuda.synchronize()
    state0 = twin.get_state()
    runs = {}
    for name, one, graph in (("one", True, False), ("eager", False, False), ("graph", False, True)):
        ppo = _ppo(one)
        assert type(ppo._fp) is FusedActorCritic and ppo._one_launch == one
        assert ppo._step_fn() == ppo._rollout_step_fused
        ppo.collect_rollouts(use_graph=graph)
        assert (ppo._graph is not None) == graph
        _restart(ppo, state0, obs0)
        rs = ppo.collect_rollouts(use_graph=graph)
        torch.cuda.synchronize()
        assert rs.env_steps == 97 * 16 and rs.episodes > 0 and torch.isfinite(ppo.buf_adv).all()
        runs[name] = (ppo, rs, {k: getattr(ppo, k).clone() for k in BUFS})
    for other in ("eager", "graph"):
        for k in BUFS:
            assert torch.equal(runs["one"][2][k].view(torch.int32), runs[other][2][k].view(torch.int32)), (other, k)
        assert runs["one"][1].episodes == runs[other][1].episodes
        assert runs["one"][1].mean_return == pytest.approx(runs[other][1].mean_return, rel=1e-6)
    ppo, _, bufs = runs["one"]
    p64 = copy.deepcopy(ppo.policy).double()
    obs = bufs["buf_obs"].reshape(-1, 12)
    act = bufs["buf_act"].reshape(-1, 4)
    with torch.no_grad():
        m64, v64 = p64.forward_heads(obs.double())
        m32, v32 = ppo.policy.forward_heads(obs)
        lp64, lp32 = p64.log_prob(m64, act.double()), ppo.policy.log_prob(m32, act)
    err, err32 = (bufs["buf_val"].reshape(-1).double() - v64).abs().max().item(), (v32.double() - v64).abs().max().item()
    print(f"RATIO ppo value: err {err:.3g} torch32 {err32:.3g} ratio {err / err32:.2f}")
    assert err <= 4 * err32, (err, err32)
    err, err32 = (bufs["buf_logp"].reshape(-1).double() - lp64).abs().max().item(), (lp32.double() - lp64).abs().max().item()
    print(f"RATIO ppo log_prob: err {err:.3g} torch32 {err32:.3g} ratio {err / err32:.2f}")
    assert err <= 4 * err32, (err, err32)
    ppo.train(max_minibatches=2)  # the update runs on the buffers the launch filled


@pytest.mark.parametrize("one_launch", [True, False])
def test_ppo_resumes_with_the_bits_of_an_uninterrupted_run(one_launch):
    """state_dict -> a fresh PPO -> load_state_dict continues the noise where the first left it. A loaded PPO
    restarts its envs from a reset (SB3's PPO.load), so the uninterrupted run is made to reset too, from the same
    env state: the next rollout of both has the same bits, which it has only if the noise counter carried."""
    a = _ppo(one_launch)
    a.collect_rollouts(use_graph=False)
    a.train(max_minibatches=2)
    sd = a.state_dict()
    assert sd["noise_step"] == 16
    first = a.buf_act.clone()
    b = _ppo(one_launch)
    b.load_state_dict(copy.deepcopy(sd))
    torch.cuda.synchronize()
    b.env.set_state(**a.env.get_state())
    a._started = False
    a.ep_ret.zero_()
    a.ep_len.zero_()
    ra, rb = a.collect_rollouts(use_graph=False), b.collect_rollouts(use_graph=False)
    torch.cuda.synchronize()
    for k in BUFS:
        assert torch.equal(getattr(a, k).view(torch.int32), getattr(b, k).view(torch.int32)), k
    assert ra.episodes == rb.episodes > 0
    assert a.state_dict()["noise_step"] == b.state_dict()["noise_step"] == 32
    assert not torch.equal(first, a.buf_act)


def test_ppo_flag_honours_fused_policy_and_the_population_keeps_its_refusal(monkeypatch):
    import dataclasses
    from uav_reinforcement_learning_control_amd.ppo import population as PO
    from uav_reinforcement_learning_control_amd.ppo.fused import FusedActorCritic, arch_rollout_supported
    from uav_reinforcement_learning_control_amd.ppo.population import PopulationPPO
    from uav_reinforcement_learning_control_amd.ppo.ppo import PPO, PPOConfig
    env = _env(40, "hover", None, 8)
    cfg = PPOConfig(net_arch=(64, 64), activation="tanh", n_steps=16, n_minibatches=4, fused_rollout_arch=True)
    on = PPO(env, cfg, seed=1)
    assert type(on._fp) is FusedActorCritic and on._one_launch
    assert arch_rollout_supported(on.policy, env)
    assert not arch_rollout_supported(on.policy, _env(40, "hover", "RelPosActWrapper", 8))
    assert not arch_rollout_supported(on.policy, _env(40, "hover", None, 8, auto_reset=False))
    off = PPO(env, dataclasses.replace(cfg, fused_policy=False), seed=1)   # fused_policy off: the torch rollout
    assert off._fp is None and not off._one_launch and off._step_fn() == off._rollout_step
    # a (128, 128) tanh member would get a FusedActorCritic image and a FusedArchLearner: the population's launches
    # read the 128-128 ReLU layouts, so it refuses, by config and by the classes the member ended up with
    tanh = PPOConfig(activation="tanh", n_steps=16, n_minibatches=4, fused_rollout_arch=True, fused_update_arch=True)
    with pytest.raises(ValueError, match="relu policy only"):
        PopulationPPO([(tanh, 0)], n_envs=8)
    m = PPO(_env(8, "hover", None, 8), tanh, seed=0)
    assert m._one_launch and m._learner is not None    # what the old guard looked at, and passed
    # the second guard: a member that passes the config check but ends up on the general classes
    monkeypatch.setattr(PO, "PPO", lambda e, cfg, seed: PPO(e, tanh, seed=seed))
    with pytest.raises(ValueError, match="not one the fused rollout and update run"):
        PopulationPPO([(PPOConfig(n_steps=16, n_minibatches=4), 0)], n_envs=8)


# ---------------------------------------------------------------- 7. the driver
def test_driver_learns_with_both_flags_and_its_policy_flies(tmp_path, capsys):
    from uav_reinforcement_learning_control_amd import evaluate as EV
    from uav_reinforcement_learning_control_amd import train
    finals = []
    for rep in ("a", "b"):
        train.main(["--num-envs", "1024", "--total-timesteps", str(12 * 1024 * 64), "--n-steps", "64", "--n-epochs", "4",
                    "--n-minibatches", "8", "--learning-rate", "3e-4", "--net-arch", "64", "64", "--activation", "tanh",
                    "--fused-arch-rollout", "--fused-arch-update", "--eval-freq", "0", "--checkpoint-freq", "0",
                    "--log-dir", str(tmp_path / rep / "logs"), "--model-dir", str(tmp_path / rep / "models")])
        out = capsys.readouterr().out
        assert ("rollout: fused rollout for net (64, 64) tanh (FusedActorCritic: quad_actor_rollout, one launch per "
                "chunk)") in out
        assert "update: fused minibatch gradient for net (64, 64) tanh (FusedArchLearner: quad_ppo_arch_grad" in out
        assert "torch per-step rollout" not in out
        (run,) = os.listdir(tmp_path / rep / "models")
        mdir = tmp_path / rep / "models" / run
        cfg = json.load(open(mdir / "config.json"))
        assert cfg["fused_arch_rollout"] is True and cfg["fused_arch_update"] is True
        assert cfg["ppo"]["net_arch"] == [64, 64]
        (log,) = os.listdir(tmp_path / rep / "logs")
        rows = np.genfromtxt(tmp_path / rep / "logs" / log / "progress.csv", delimiter=",", names=True)
        ret = rows["mean_return"]
        print("mean returns", [round(float(x), 2) for x in ret])
        assert len(ret) == 12 and np.all(np.isfinite(ret))
        assert ret[-1] > ret[0]
        sd = torch.load(mdir / "policy.pt", map_location="cpu", weights_only=True)
        assert all(torch.isfinite(v).all() for v in sd.values())
        finals.append((sd, ret, str(mdir / "hover_policy_final.zip")))
    # Philox noise and a bit-reproducible gradient: the second run is the first
    assert np.array_equal(finals[0][1], finals[1][1])
    for k, v in finals[0][0].items():
        assert torch.equal(v, finals[1][0][k]), k
    r = EV.evaluate_episodes(finals[0][2], num_episodes=64, device="cuda")
    assert len(r["rewards"]) == 64 and np.all(np.isfinite(r["rewards"])) and r["mean_length"] > 0
