"""Restatements for the Brax unroll's tests (csrc/brax_actor.h sample_action / log_prob, csrc/brax_unroll.hip):
NormalTanh.log_prob in float64 NumPy -- the GPU tests' yardstick, itself checked against torch's float64 on the CPU
-- and the hand-built logits case. numpy and torch on the CPU only. TEST INFRASTRUCTURE ONLY."""
import math

import numpy as np
import torch

import brax_actor_ref as B

HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
LOG2 = math.log(2.0)


def log_prob64(logits, raw, min_std=B.MIN_STD):
    """NormalTanh.log_prob(logits, raw) (ppo/brax_ppo.py) in float64 from whatever words it is given:
    sum_k -1/2 ((raw - loc) / scale)^2 - 1/2 log 2 pi - log scale - 2 (log 2 - raw - softplus(-2 raw)),
    scale = softplus(logits[4:]) + min_std."""
    lg, x = np.asarray(logits, np.float64), np.asarray(raw, np.float64)
    loc, scale = lg[..., :4], np.logaddexp(lg[..., 4:], 0.0) + min_std
    t = (x - loc) / scale
    lp = -0.5 * t * t - HALF_LOG_2PI - np.log(scale)
    det = 2.0 * (LOG2 - x - np.logaddexp(-2.0 * x, 0.0))
    return (lp - det).sum(-1)


# ---- the hand-built logits: a ReLU net with an identity normaliser whose logit q is a_q x_q + b_q of observation
# feature q (neuron q passes relu(x_q), neuron 32 + q passes relu(-x_q), layer 2 hands both on, the head takes their
# difference), so the observation rows choose the logits. loc = 8 x covers [-8, 8], where tanh saturates; the raw
# scale logit -9 + 11 x (the head BIAS carries the -9) covers [-20, 2]: at -20 softplus is 2e-9 and scale = min_std.
HAND_ARCH = (64, 64, "relu")
HAND_LOC_GAIN, HAND_SCALE_GAIN, HAND_SCALE_BIAS = 8.0, 11.0, -9.0


def hand_params():
    h1, h2, _ = HAND_ARCH
    p = {k: torch.zeros(s) for k, s in B.shapes(h1, h2).items()}
    q = torch.arange(8)
    p["w0"][q, q], p["w0"][q, 32 + q] = 1.0, -1.0
    p["w1"][torch.arange(64), torch.arange(64)] = 1.0
    gain = torch.tensor([HAND_LOC_GAIN] * 4 + [HAND_SCALE_GAIN] * 4)
    p["w2"][q, q], p["w2"][32 + q, q] = gain, -gain
    p["b2"] = torch.tensor([0.0] * 4 + [HAND_SCALE_BIAS] * 4)
    return p


def hand_obs(n=B.N_ROWS, seed=61):
    """Observation rows: features 0-7 uniform in [-1, 1], with the first rows at the corners (loc = +-8 exactly,
    raw scale logit -20 and 2)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros(n, B.OBS)
    x[:, :8] = torch.rand(n, 8, generator=g) * 2 - 1
    x[0, :8] = torch.tensor([1.0, -1.0, 1.0, -1.0, -1.0, -1.0, 1.0, 1.0])
    x[1, :8] = torch.tensor([-1.0, 1.0, -1.0, 1.0, -1.0, 1.0, -1.0, 1.0])
    x[2:34, 4:8] = -1.0   # scale = min_std over the whole range of loc
    return x.contiguous()
