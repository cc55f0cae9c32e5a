"""Inputs and float64 pieces for the general Brax gradient (csrc/brax_learner_arch.hip, quad_brax_ppo_arch_grad):
tests/brax_learner_ref.py's synthetic minibatch with the policy's and the value net's hidden sizes and the activation
as arguments, and the closed-form backward of one hidden layer per activation (SiLU's from the pre-activation).
tests/test_brax_learner_arch_cpu.py checks the closed forms against autograd; tests/test_gpu_brax_learner_arch.py
builds its cases here."""
from __future__ import annotations

import torch

from brax_learner_ref import (LOG_RHO_MARGIN, FixedNoise, autograd_reference, gather, patterns,  # noqa: F401
                              reference_loss)
from uav_reinforcement_learning_control_amd.ppo.brax_ppo import _ACT, BraxActorCritic, BraxPPOConfig


def act_backward(activation: str, pre: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """dL/d(pre-activation) from g = dL/d(activation), in the kernels' forms: ReLU h > 0 and tanh 1 - h^2 from the
    activation h; SiLU sigma(x) (1 + x (1 - sigma(x))) from the pre-activation x."""
    if activation == "relu":
        return torch.where(torch.relu(pre) > 0, g, torch.zeros_like(g))
    if activation == "tanh":
        h = torch.tanh(pre)
        return g * (1.0 - h * h)
    sg = 1.0 / (1.0 + torch.exp(-pre))
    return g * (sg * (1.0 + pre * (1.0 - sg)))


def hidden_backward(activation: str, x, w, b, g):
    """(dL/dw, dL/db, dL/dx) of h = act(x @ w + b) for g = dL/dh, w in flax's [in, out] layout."""
    d = act_backward(activation, x @ w + b, g)
    return x.transpose(-1, -2) @ d, d.sum(0), d @ w.transpose(-1, -2)


def hidden_margin(net: BraxActorCritic, x, activation: str):
    """min |pre-activation| over both nets' hidden layers, per leading index of x [.., 21], with the case's
    activation between the layers."""
    out = None
    for mlp in (net.policy, net.value):
        h = x
        for k, b in list(zip(mlp.kernels, mlp.biases))[:-1]:
            pre = h @ k + b
            m = pre.abs().amin(-1)
            out = m if out is None else torch.minimum(out, m)
            h = _ACT[activation](pre)
    return out


def make_case(U: int, n: int, L: int, mb: int, seed: int, device="cpu", normalize_advantage: bool = True,
              policy_hidden_sizes=(128, 128), value_hidden_sizes=(128, 128), activation: str = "relu"):
    """tests/brax_learner_ref.py make_case for any two-hidden-layer nets and activation: the same draws in the same
    order. ReLU cases draw the minibatch from the trajectories whose float64 hidden pre-activations all lie at least
    1e-5 from zero (`dropped` is the share left out); tanh and SiLU are smooth and take every trajectory
    (dropped == 0)."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    cfg = BraxPPOConfig(unroll_length=L, normalize_advantage=normalize_advantage, activation=activation,
                        policy_hidden_sizes=tuple(policy_hidden_sizes), value_hidden_sizes=tuple(value_hidden_sizes))
    torch.manual_seed(seed)
    net = BraxActorCritic(21, 4, cfg).double()
    with torch.no_grad():
        for mlp in (net.policy, net.value):
            for b in mlp.biases:
                b.copy_(0.1 * rn(*b.shape))
    M = U * n
    obs = 2.0 * rnd(U, L, n, 21) - 1.0
    nxt = 2.0 * rnd(U, n, 21) - 1.0
    small = (torch.arange(M) % 7 == 6).view(U, n)
    obs[small[:, None, :].expand(U, L, n)] *= 0.01
    nxt[small] *= 0.01
    obs, nxt = obs.float(), nxt.float()
    mean, std = (0.2 * rn(21)).float(), (0.5 + rnd(21)).float()
    norm = lambda x: ((x - mean) / std).double()   # RunningStats.normalize in f32, then exact in f64
    with torch.no_grad():
        lg = net.policy(norm(obs))
        s = lg[..., 4:]
        f = min(1.0, 1.5 / float(s.abs().max()))   # raw scale logits within [-1.5, 1.5]: scale in about [0.2, 1.7]
        net.policy.kernels[-1][:, 4:] *= f
        net.policy.biases[-1][4:] *= f
        lg = net.policy(norm(obs))
        loc, scale = net.dist.split(lg)
        raw = (loc + scale * rn(U, L, n, 4)).float()
        lp = net.dist.log_prob(lg, raw.double())
        rho = 0.55 + 0.9 * rnd(U, L, n)
        for edge in (0.7, 1.3):
            near = (rho - edge).abs() < 4 * LOG_RHO_MARGIN
            rho = torch.where(near, rho + 8 * LOG_RHO_MARGIN, rho)
        logp = (lp - torch.log(rho)).float()
        margin = torch.minimum(hidden_margin(net, norm(obs), activation).amin(1),
                               hidden_margin(net, norm(nxt), activation)).reshape(M)
    reward = rn(U, L, n).float()
    dm, tm = patterns(L, M)
    disc = dm.view(L, U, n).transpose(0, 1).contiguous().float()
    trunc = tm.view(L, U, n).transpose(0, 1).contiguous().float()
    cand = torch.nonzero(margin >= 1e-5).flatten() if activation == "relu" else torch.arange(M)
    dropped = 1.0 - cand.numel() / M
    index = cand[torch.randperm(cand.numel(), generator=g)[:mb]].contiguous()
    z = rn(L, mb, 4).float()
    to = lambda t: t.to(device)
    return dict(cfg=cfg, net=net.to(device), mean=to(mean), std=to(std), index=to(index), z=to(z), dropped=dropped,
                buffers=dict(obs=to(obs), nxt=to(nxt), raw=to(raw), logp=to(logp), rew=to(reward), disc=to(disc),
                             trunc=to(trunc)), shape=(U, n, L, mb))
