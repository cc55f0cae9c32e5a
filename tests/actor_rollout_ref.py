"""A numpy model of one rollout step's bookkeeping (PPO._rollout_step, which restates SB3's
OnPolicyAlgorithm.collect_rollouts): given the policy's (mean, value) of the step's observation, the standard
normals z and what the env returned, the rows the step writes and the state it carries. The forward passes
themselves are not modelled: they come in as numbers. TEST INFRASTRUCTURE ONLY (numpy; nothing native).

Every operation is one f32 operation, in torch's order: a product and a sum are two roundings (torch does not
fuse them; the kernels' reward row r + gamma V fuses them, which is why the GPU tests compare the two kernel forms
with each other bit for bit and the kernels with float64 under a bar)."""
import math

import numpy as np

F = np.float32
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def sample(mean, std, z):
    """a = mean + std z (the unclipped action the buffer keeps)."""
    return (mean + (std[None, :] * z).astype(F)).astype(F)


def log_prob(mean, std, log_std, a):
    """policy.log_prob at the stored action: z is recomputed from a, as PPO.train does. The four terms are summed
    left to right."""
    zz = ((a - mean) / std[None, :]).astype(F)
    terms = (F(-0.5) * zz * zz - log_std[None, :] - F(HALF_LOG_2PI)).astype(F)
    lp = terms[:, 0]
    for k in range(1, terms.shape[1]):
        lp = (lp + terms[:, k]).astype(F)
    return lp


def clip(a):
    """What the env receives."""
    return np.clip(a, F(-1), F(1)).astype(F)


def step(mean, value, z, log_std, last_start, reward, terminated, truncated, terminal_value, gamma, ep_ret, ep_len,
         std=None):
    """One step. Inputs are f32 arrays ([n, 4] mean and z; [n] value, last_start, reward, terminal_value, ep_ret,
    ep_len; [4] log_std; bool [n] terminated / truncated). std: exp(log_std) if the caller has its own rounding of it.
    Returns the rows (actions, log_prob, value, episode_starts, actions_env, rewards), the carried state
    (last_start, ep_ret, ep_len) and the Monitor sums of the episodes that ended (float64 return, length, count)."""
    mean, z, log_std = mean.astype(F), z.astype(F), log_std.astype(F)
    std = np.exp(log_std).astype(F) if std is None else std.astype(F)
    a = sample(mean, std, z)
    lp = log_prob(mean, std, log_std, a)
    done = terminated | truncated
    timeout = truncated & ~terminated
    # TimeLimit bootstrap: r += gamma V(terminal_obs) where the time limit, not the env, ended the episode
    tv = np.nan_to_num(terminal_value.astype(F))
    rewards = (reward + (F(gamma) * timeout.astype(F)) * tv).astype(F)
    ret = (ep_ret + reward).astype(F)
    length = (ep_len + F(1)).astype(F)
    stats = np.array([ret[done].astype(np.float64).sum(), length[done].astype(np.float64).sum(), float(done.sum())])
    return dict(actions=a, log_prob=lp, value=value.astype(F), episode_starts=last_start.astype(F),
                actions_env=clip(a), rewards=rewards, last_start=done.astype(F),
                ep_ret=np.where(done, F(0), ret).astype(F), ep_len=np.where(done, F(0), length).astype(F),
                stats=stats)
