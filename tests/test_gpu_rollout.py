"""The one-launch rollout (quad_rollout, csrc/rollout.hip) against the two-launch form it fuses.

The two-launch form -- k_policy_act with the fused epilogue, then quad_step, then
quad_rollout_post -- is the path the rest of the GPU suite pins: its env step against the float64
oracle (test_gpu_parity.py), its policy against the torch fp32 ActorCritic and its noise against the
oracle's Philox + Box-Muller (test_gpu_policy.py). quad_rollout runs the same operations in one
launch per chunk of steps with the env state in registers, so every buffer row, the carried
last_obs / last_start / ep_ret / ep_len and the env state must agree BIT FOR BIT; the Monitor
statistics are summed in a different order (float64 per thread vs float per block) and agree to
1e-6 relative.

Cases: hover / hover + RateControlWrapper / TrajectoryFollowEnv + RateControlWrapper; short
max_episode_steps so that time-limit truncations (the critic bootstrap) occur besides
terminations; ragged N (dead lanes in the last block); rollouts split over several launches.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _policy(seed=0):
    from uav_reinforcement_learning_control_amd.ppo.policy import ActorCritic
    torch.manual_seed(seed)
    pol = ActorCritic(12, 4, (128, 128)).cuda()
    with torch.no_grad():  # small weights + small std: episodes survive long enough to truncate
        for p in pol.parameters():
            p.copy_(torch.randn_like(p) * (0.3 / math.sqrt(max(p.shape[-1], 1))))
        pol.log_std.copy_(torch.tensor([-1.5, -2.0, -2.0, -2.5]))
    return pol


def _env(n, kind, wrapper, max_steps, seed=5, base=0):
    from uav_reinforcement_learning_control_amd.envs import QuadVecEnv
    env = QuadVecEnv(n, env=kind, wrapper=wrapper, device="cuda:0", seed=seed, env_id_base=base,
                     max_episode_steps=max_steps)
    return env


def _bufs(T, n):
    f = dict(dtype=torch.float32, device="cuda")
    from uav_reinforcement_learning_control_amd import _native as N
    return dict(obs_copy=torch.full((T, n, 12), -7.0, **f), actions=torch.full((T, n, 4), -7.0, **f),
                log_prob=torch.full((T, n), -7.0, **f), value=torch.full((T, n), -7.0, **f),
                episode_starts=torch.full((T, n), -7.0, **f), rewards=torch.full((T, n), -7.0, **f),
                last_obs=torch.zeros(n, 12, **f), last_start=torch.ones(n, **f),
                ep_ret=torch.zeros(n, **f), ep_len=torch.zeros(n, **f),
                stats=torch.zeros(N.POLICY_STAT_SLOTS, 3, dtype=torch.float64, device="cuda"))


def _two_launch(fp, env, b, T, seed, gamma, deterministic=False):
    cur = torch.zeros(4, dtype=torch.int32, device="cuda")
    act_env = torch.zeros(env.num_envs, 4, device="cuda")
    epi = fp.make_epilogue(env.reward, env.terminated, env.truncated, env.terminal_obs, b["rewards"],
                           b["last_start"], b["ep_ret"], b["ep_len"], b["stats"], T, gamma)
    for _ in range(T):
        fp.act(b["last_obs"], act_env, actions=b["actions"], log_prob=b["log_prob"], value=b["value"],
               obs_copy=b["obs_copy"], last_start=b["last_start"], episode_starts=b["episode_starts"],
               cursor=cur, rows=T, seed=seed, env_id_base=env.env_id_base, deterministic=deterministic,
               epilogue=epi)
        env.step(act_env, obs=b["last_obs"], info="raw")
    fp.post(epi, cur)
    torch.cuda.synchronize()


def _one_launch(fp, env, b, T, seed, gamma, chunks, deterministic=False):
    t = 0
    for k in chunks:
        fp.rollout(env, t0=t, steps=k, seed=seed, gamma=gamma, deterministic=deterministic, **b)
        t += k
    assert t == T
    torch.cuda.synchronize()


@pytest.mark.parametrize("kind,wrapper,max_steps,n,chunks", [
    ("hover", None, 6, 1000, (20,)),
    ("hover", "RateControlWrapper", 9, 4096 + 37, (7, 13)),
    ("trajectory", "RateControlWrapper", 11, 777, (5, 5, 10)),
    ("hover", None, 512, 65536, (20,)),
])
@pytest.mark.parametrize("nt", ["2", "1"])
def test_one_launch_rollout_is_bit_identical(kind, wrapper, max_steps, n, chunks, nt, monkeypatch):
    # nt: tiles per wave of k_rollout (2 = product default; 1 = the A/B form, read per launch)
    monkeypatch.setenv("QUADENV_ROLLOUT_NT", nt)
    from uav_reinforcement_learning_control_amd.ppo.fused import FusedPolicy
    T, seed, gamma = sum(chunks), 0x1234_5678_9ABC, 0.97
    fp = FusedPolicy(_policy())
    fp.pack()
    ea, eb = _env(n, kind, wrapper, max_steps, base=3 * n), _env(n, kind, wrapper, max_steps, base=3 * n)
    A, B = _bufs(T, n), _bufs(T, n)
    A["last_obs"].copy_(ea.reset())
    B["last_obs"].copy_(eb.reset())
    _two_launch(fp, ea, A, T, seed, gamma)
    _one_launch(fp, eb, B, T, seed, gamma, chunks)
    for k in ("obs_copy", "actions", "log_prob", "value", "episode_starts", "rewards", "last_obs",
              "last_start", "ep_ret", "ep_len"):
        a, b = A[k].cpu().numpy(), B[k].cpu().numpy()
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), \
            f"{k}: {np.sum(a.view(np.uint32) != b.view(np.uint32))} words differ"
    sa, sb = ea.get_state(), eb.get_state()
    for k, v in sa.items():
        assert np.array_equal(np.asarray(v).view(np.uint32), np.asarray(sb[k]).view(np.uint32)), k
    ta, tb = A["stats"].sum(0).cpu().numpy(), B["stats"].sum(0).cpu().numpy()
    np.testing.assert_allclose(tb, ta, rtol=1e-6)
    # the case exercised what it claims: resets, and (short limits) time-limit bootstraps
    starts = B["episode_starts"].cpu().numpy()
    last = B["last_start"].cpu().numpy()
    done = np.concatenate([starts[1:], last[None]], 0)  # done[t] = env finished at step t
    assert done.sum() > 0 and tb[2] == done.sum()
    if max_steps <= T:
        length = np.zeros(n)
        truncs = 0
        for t in range(T):
            length += 1
            truncs += int(np.sum((done[t] == 1) & (length == max_steps)))
            length[done[t] == 1] = 0
        assert truncs > 0


@pytest.mark.parametrize("nt", ["2", "1"])
def test_deterministic_rollout_is_bit_identical_and_unnoised(nt, monkeypatch):
    """QuadRollout.deterministic: one launch against two launches with deterministic = 1 on both sides,
    every buffer and the env state bit for bit; the actions rows are the un-noised mean (the torch fp32
    mean of the stored observations, test_gpu_policy's 2e-5 bar; the noise's std is 0.08 .. 0.22), so
    log_prob is the constant -sum(log_std) - 4 * 0.5 log(2 pi) to f32 rounding."""
    monkeypatch.setenv("QUADENV_ROLLOUT_NT", nt)
    from uav_reinforcement_learning_control_amd.ppo.fused import FusedPolicy
    kind, wrapper, max_steps, n, chunks = "trajectory", "RateControlWrapper", 11, 777, (5, 5, 10)
    T, seed, gamma = sum(chunks), 0x1234_5678_9ABC, 0.97
    pol = _policy()
    fp = FusedPolicy(pol)
    fp.pack()
    ea, eb = _env(n, kind, wrapper, max_steps, base=3 * n), _env(n, kind, wrapper, max_steps, base=3 * n)
    A, B = _bufs(T, n), _bufs(T, n)
    A["last_obs"].copy_(ea.reset())
    B["last_obs"].copy_(eb.reset())
    _two_launch(fp, ea, A, T, seed, gamma, deterministic=True)
    _one_launch(fp, eb, B, T, seed, gamma, chunks, deterministic=True)
    for k in ("obs_copy", "actions", "log_prob", "value", "episode_starts", "rewards", "last_obs",
              "last_start", "ep_ret", "ep_len"):
        a, b = A[k].cpu().numpy(), B[k].cpu().numpy()
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), \
            f"{k}: {np.sum(a.view(np.uint32) != b.view(np.uint32))} words differ"
    sa, sb = ea.get_state(), eb.get_state()
    for k, v in sa.items():
        assert np.array_equal(np.asarray(v).view(np.uint32), np.asarray(sb[k]).view(np.uint32)), k
    np.testing.assert_allclose(B["stats"].sum(0).cpu().numpy(), A["stats"].sum(0).cpu().numpy(), rtol=1e-6)
    assert B["last_start"].sum().item() + B["episode_starts"][1:].sum().item() > 0   # episodes ended
    # no noise: the stored actions are the policy's mean of the stored observations
    with torch.no_grad():
        mean, _ = pol.forward_heads(B["obs_copy"].reshape(T * n, 12))
    a, m = B["actions"].reshape(T * n, 4).double(), mean.double()
    assert ((a - m).abs() / (1 + m.abs())).max().item() <= 2e-5
    # z = 0 exactly, so every log_prob is the same number: four terms -log_std[k] - 0.5 log(2 pi), each
    # rounded twice and summed in f32 (partial sums below 8: at most 8 half-ulps of 4.77e-7)
    lp = B["log_prob"].cpu().numpy()
    const = -float(pol.log_std.detach().double().sum()) - 4 * 0.5 * math.log(2 * math.pi)
    assert np.unique(lp).size == 1
    assert abs(float(lp.flat[0]) - const) <= 8 * 0.5 * 4.77e-7


def test_rollout_rejects_bad_arguments():
    from uav_reinforcement_learning_control_amd import _native as N
    from uav_reinforcement_learning_control_amd.ppo.fused import FusedPolicy, rollout_supported
    fp = FusedPolicy(_policy())
    fp.pack()
    n = 64
    env = _env(n, "hover", "RelPosActWrapper", 512)
    assert not rollout_supported(env)
    b = _bufs(4, n)
    with pytest.raises(N.QuadError):
        fp.rollout(env, t0=0, steps=4, seed=1, gamma=0.99, **b)  # 7-D obs: rejected by the ABI
    env2 = _env(n, "hover", None, 512)
    assert rollout_supported(env2)
    with pytest.raises(N.QuadError):
        fp.rollout(env2, t0=0, steps=0, seed=1, gamma=0.99, **b)
    with pytest.raises(ValueError):
        fp.rollout(env2, t0=0, steps=1, seed=1, gamma=0.99, **dict(b, ep_len=torch.zeros(n + 1, device="cuda")))


def test_ppo_collect_one_launch_and_two_launch():
    """PPO.collect_rollouts through quad_rollout (default) and through the graph-captured
    two-launch path: both fill the buffers, finish episodes, and feed the update. (Their rows are
    not compared: the two-launch path's graph capture steps the env once before its first rollout;
    the bit-level equivalence is test_one_launch_rollout_is_bit_identical.)"""
    from uav_reinforcement_learning_control_amd.ppo.ppo import PPO, PPOConfig
    n, T = 2048, 32
    outs = []
    for one in (False, True):
        env = _env(n, "hover", None, 512, seed=11)
        cfg = PPOConfig(n_steps=T, n_epochs=1, n_minibatches=4, fused_rollout=one)
        ppo = PPO(env, cfg, seed=3)
        assert ppo._one_launch == one
        rs = ppo.collect_rollouts()
        outs.append((rs, {k: getattr(ppo, k).clone() for k in ("buf_rew", "buf_val", "buf_logp", "buf_adv",
                                                               "buf_ret", "buf_start")}))
        assert rs.env_steps == n * T and torch.isfinite(ppo.buf_adv).all()
        ppo.train(max_minibatches=2)  # the update runs on the one-launch buffers
        rs2 = ppo.collect_rollouts()
        assert rs2.env_steps == n * T
    (ra, _), (rb, _) = outs
    assert ra.episodes > 0 and rb.episodes > 0
    assert abs(ra.mean_length - rb.mean_length) < 0.5 * max(ra.mean_length, rb.mean_length)
