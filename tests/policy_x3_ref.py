"""CPU restatement of the rollout policy's arithmetic (csrc/policy_net.h) for the precision tests:
the 12-128-128-(4|1) ReLU nets in float64, a model of the three-piece bf16 scheme with a chosen
subset of the six piece products, the seeded policies / observation sets the CPU and GPU tests share,
and the acceptance rule. torch on the CPU only; nothing of the package's native side is imported.
TEST INFRASTRUCTURE ONLY."""
import math

import numpy as np
import torch

N_ROWS = 4096
# max|got - ref64| <= FACTOR * max|torch32 - ref64| + FLOOR * max|ref64| per output tensor: the
# pre-activation factor of test_gpu_learner.test_config3_minibatch_unfiltered
FACTOR = 4.0
FLOOR = 1e-7

# HoverEnv._state_bounds (QuadCfg.term_low / term_high of the hover kind; the tests check them
# against the oracle's and the library's default configuration)
_PI = math.pi
HOVER_TERM_LOW = np.array([-2, -2, 0, -_PI, -_PI, -_PI, -10, -10, -10, -6 * _PI, -6 * _PI, -6 * _PI], np.float32)
HOVER_TERM_HIGH = np.array([2, 2, 2, _PI, _PI, _PI, 10, 10, 10, 6 * _PI, 6 * _PI, 6 * _PI], np.float32)

# parameter names, in quad_policy_pack's order (FusedPolicy.pack)
NAMES = ("pi_w0", "pi_b0", "pi_w1", "pi_b1", "act_w", "act_b",
         "vf_w0", "vf_b0", "vf_w1", "vf_b1", "val_w", "val_b", "log_std")
SHAPES = dict(pi_w0=(128, 12), pi_b0=(128,), pi_w1=(128, 128), pi_b1=(128,), act_w=(4, 128), act_b=(4,),
              vf_w0=(128, 12), vf_b0=(128,), vf_w1=(128, 128), vf_b1=(128,), val_w=(1, 128), val_b=(1,),
              log_std=(4,))

# piece products (weight piece i, activation piece j) in mfma6's order, small terms first
SIX = ((2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0))
VARIANTS = {
    "no_a2b0": tuple(t for t in SIX if t != (2, 0)),
    "no_a1b1": tuple(t for t in SIX if t != (1, 1)),
    "no_a0b2": tuple(t for t in SIX if t != (0, 2)),
    "two_piece": ((1, 1), (1, 0), (0, 1), (0, 0)),   # x = x0 + x1 only: every product with a third piece gone
}


# ---------------------------------------------------------------- policies and observation sets
def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float32)


def _orthogonal(g, rows, cols, gain):
    """torch.nn.init.orthogonal_'s construction from a seeded generator."""
    a = _randn(g, max(rows, cols), min(rows, cols)).double()
    q, r = torch.linalg.qr(a)
    q = q * torch.sign(torch.diagonal(r))
    if rows < cols:
        q = q.t()
    return (gain * q).float().contiguous()


def policy_a(seed=11):
    """tests/test_gpu_policy._policy's scale: every parameter N(0, 1 / fan_in)."""
    g = torch.Generator().manual_seed(seed)
    p = {k: _randn(g, *SHAPES[k]) / math.sqrt(SHAPES[k][-1]) for k in NAMES}
    p["log_std"] = torch.tensor([-0.3, 0.1, 0.4, -1.0])
    return p


def policy_b(seed=12):
    """tests/test_gpu_learner._policy's style: SB3's orthogonal init, biases N(0, 0.1), the action
    head x 30, mixed log_std."""
    g = torch.Generator().manual_seed(seed)
    p = {}
    for k in NAMES:
        shp = SHAPES[k]
        if len(shp) == 2:
            gain = {"act_w": 0.01 * 30.0, "val_w": 1.0}.get(k, math.sqrt(2.0))
            p[k] = _orthogonal(g, shp[0], shp[1], gain)
        else:
            p[k] = _randn(g, *shp) * 0.1
    p["log_std"] = torch.tensor([-0.4, 0.1, 0.3, -1.0])
    return p


def policy_c(seed=13):
    """Hidden-layer weights with magnitudes log-uniform over 2^-12 .. 2^2 and random signs: the
    pieces' exponents differ widely within one k-step. Biases and heads as policy_a."""
    g = torch.Generator().manual_seed(seed)
    p = policy_a(seed + 100)
    for k in ("pi_w0", "pi_w1", "vf_w0", "vf_w1"):
        e = torch.rand(*SHAPES[k], generator=g, dtype=torch.float64) * 14.0 - 12.0
        s = torch.where(torch.rand(*SHAPES[k], generator=g) < 0.5, -1.0, 1.0).double()
        p[k] = (s * torch.exp2(e)).float()
    return p


def obs_uniform(n=N_ROWS, seed=21):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, 12, generator=g, dtype=torch.float32) * 2 - 1


def obs_bounds(n=N_ROWS, seed=22):
    """Every feature over its termination range; every 7th row x 0.01 (rows near the origin)."""
    g = torch.Generator().manual_seed(seed)
    lo, hi = torch.from_numpy(HOVER_TERM_LOW), torch.from_numpy(HOVER_TERM_HIGH)
    x = lo + (hi - lo) * torch.rand(n, 12, generator=g, dtype=torch.float32)
    x[::7] *= 0.01
    return x.contiguous()


def obs_exact(n=N_ROWS, seed=23):
    """A quarter of the entries exactly 0, a quarter +-2^k (k = -6 .. 3), the rest uniform [-1, 1]."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, 12, generator=g, dtype=torch.float32) * 2 - 1
    kind = torch.randint(0, 4, (n, 12), generator=g)
    k = torch.randint(-6, 4, (n, 12), generator=g).float()
    sgn = torch.where(torch.rand(n, 12, generator=g) < 0.5, -1.0, 1.0)
    x = torch.where(kind == 0, torch.zeros(()), torch.where(kind == 1, sgn * torch.exp2(k), x))
    return x.contiguous()


def cases():
    """[(name, params, obs)]: the 3 x 3 policies and observation sets of the accuracy tests."""
    pols = (("a", policy_a()), ("b", policy_b()), ("c", policy_c()))
    sets = (("uniform", obs_uniform()), ("bounds", obs_bounds()), ("exact", obs_exact()))
    return [(f"{pn}-{on}", p, o) for pn, p in pols for on, o in sets]


def make_policy(params, device="cpu"):
    """A torch fp32 ActorCritic holding `params`."""
    from uav_reinforcement_learning_control_amd.ppo.policy import ActorCritic
    pol = ActorCritic(12, 4, (128, 128))
    ex = pol.mlp_extractor
    dst = dict(pi_w0=ex.policy_net[0].weight, pi_b0=ex.policy_net[0].bias, pi_w1=ex.policy_net[2].weight,
               pi_b1=ex.policy_net[2].bias, act_w=pol.action_net.weight, act_b=pol.action_net.bias,
               vf_w0=ex.value_net[0].weight, vf_b0=ex.value_net[0].bias, vf_w1=ex.value_net[2].weight,
               vf_b1=ex.value_net[2].bias, val_w=pol.value_net.weight, val_b=pol.value_net.bias,
               log_std=pol.log_std)
    with torch.no_grad():
        for k in NAMES:
            dst[k].copy_(params[k])
    return pol.to(device)


def noisy_actions(params, obs, seed=31):
    """f32 actions mean64 + std z with seeded z: the actions of the CPU test's log_prob."""
    g = torch.Generator().manual_seed(seed)
    mean, _ = forward64(params, obs)
    z = torch.randn(mean.shape, generator=g, dtype=torch.float64)
    return (mean + params["log_std"].double().exp() * z).float()


# ---------------------------------------------------------------- float64 reference
def _d(t):
    return torch.as_tensor(t).detach().cpu().double()


def forward64(params, obs):
    """(mean [n,4], value [n]) of the 12-128-128-(4|1) ReLU nets in float64 on the CPU."""
    x = _d(obs)
    out = []
    for w0, b0, w1, b1, w2, b2 in (("pi_w0", "pi_b0", "pi_w1", "pi_b1", "act_w", "act_b"),
                                   ("vf_w0", "vf_b0", "vf_w1", "vf_b1", "val_w", "val_b")):
        h = torch.relu(x @ _d(params[w0]).t() + _d(params[b0]))
        h = torch.relu(h @ _d(params[w1]).t() + _d(params[b1]))
        out.append(h @ _d(params[w2]).t() + _d(params[b2]))
    return out[0], out[1][:, 0]


def log_prob64(params, mean, actions):
    """The diagonal Gaussian's log-density of `actions` in float64 (ActorCritic.log_prob)."""
    ls = _d(params["log_std"])
    z = (_d(actions) - _d(mean)) / ls.exp()
    return (-0.5 * z * z - ls - 0.5 * math.log(2 * math.pi)).sum(-1)


# ---------------------------------------------------------------- the bf16x3 scheme
def split3(x):
    """Three round-to-nearest bf16 pieces of an f32 tensor, x = p0 + p1 + p2 + (<= 2^-24 |x|), each
    the bf16 of what the previous ones leave (the remainders are exact in f32). float64 tensors."""
    x = torch.as_tensor(x, dtype=torch.float32)
    p0 = x.bfloat16().float()
    r1 = x - p0
    p1 = r1.bfloat16().float()
    r2 = r1 - p1
    p2 = r2.bfloat16().float()
    return p0.double(), p1.double(), p2.double()


def _layer_x3(w, b, x, terms):
    wp, xp = split3(w), split3(x)
    acc = torch.as_tensor(b, dtype=torch.float32).expand(x.shape[0], -1)
    for i, j in SIX:
        if (i, j) in terms:
            acc = (acc.double() + xp[j] @ wp[i].t()).float()   # exact products, one f32 rounding per term
    return acc


def emulate_x3(params, obs, terms=SIX):
    """(mean, value) in f32 by the scheme policy_net.h's header states: three round-to-nearest bf16
    pieces per operand of the two hidden layers, the piece products (weight piece i, activation
    piece j) listed in `terms` in mfma6's order, exact products, f32 accumulation (one rounding per
    piece product over the whole dot product), heads in f32.

    A MODEL OF THE SCHEME, NOT OF THE HARDWARE'S ACCUMULATION: v_mfma_f32_32x32x16_bf16 sums 16
    products per instruction with its own alignment and truncation, over 1 (layer 1) or 8 (layer 2)
    k-steps per output. It tells which piece products the result needs, not the kernel's bits."""
    terms = set(terms)
    x = torch.as_tensor(obs, dtype=torch.float32).cpu()
    out = []
    for w0, b0, w1, b1, w2, b2 in (("pi_w0", "pi_b0", "pi_w1", "pi_b1", "act_w", "act_b"),
                                   ("vf_w0", "vf_b0", "vf_w1", "vf_b1", "val_w", "val_b")):
        h = torch.relu(_layer_x3(params[w0], params[b0], x, terms))
        h = torch.relu(_layer_x3(params[w1], params[b1], h, terms))
        out.append(torch.nn.functional.linear(h, params[w2].float(), params[b2].float()))
    return out[0], out[1][:, 0]


# ---------------------------------------------------------------- the acceptance rule
def errors(got, ref64, got32):
    """(err, err32, scale, ratio): max|got - ref64|, max|got32 - ref64|, max|ref64| and
    err / err32 (inf if torch fp32 is exact and got is not)."""
    r = _d(ref64)
    err = (_d(got) - r).abs().max().item()
    err32 = (_d(got32) - r).abs().max().item()
    ratio = err / err32 if err32 > 0 else (0.0 if err == 0 else math.inf)
    return err, err32, r.abs().max().item(), ratio


def within_bar(got, ref64, got32, factor=FACTOR):
    """max|got - ref64| <= factor * max|got32 - ref64| + 1e-7 * max|ref64| (NaN fails)."""
    err, err32, scale, _ = errors(got, ref64, got32)
    return err <= factor * err32 + FLOOR * scale
