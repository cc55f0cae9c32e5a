"""CPU restatement of the Brax-profile policy's arithmetic (csrc/brax_actor.h) for its tests, in the style of
actor_arch_ref: seeded parameter styles (flax [in, out] kernels), normalisers and observation sets, the float64
reference, the torch-f32 forward and the bf16x3 scheme model for the net 21 -> h1 -> h2 -> 8 with ReLU, tanh or
SiLU; scalar models of silu_f32 / softplus_f32 with the header's ulp bounds; a host restatement of the action draw;
and the closed loop's own sensitivity to the last bit of the action on the float64 oracle env. torch, numpy and the
oracle on the CPU only; nothing of the package's native side is imported. TEST INFRASTRUCTURE ONLY."""
import math
import os
import re

import numpy as np
import torch

import policy_x3_ref as R

N_ROWS = 1024
ARCHS = ((32, 64), (64, 64), (96, 64), (128, 128), (256, 256), (512, 256))
ACTIVATIONS = ("relu", "tanh", "silu")
NAMES = ("w0", "b0", "w1", "b1", "w2", "b2")  # QuadBraxActorParams' order; kernels are [in, out]
STYLES = ("a", "b", "c")
OBS_SETS = ("unit", "raw", "clip")
OBS, LOGITS = 21, 8
MIN_STD = 0.001

_HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    "uav_reinforcement_learning_control_amd", "csrc", "brax_actor.h")


def header_ulp(name):
    """SILU_ULP / SOFTPLUS_ULP as csrc/brax_actor.h states them."""
    m = re.search(rf"constexpr float {name} = ([0-9.]+)f;", open(_HDR).read())
    return float(m.group(1))


TANH_ULP = 2.0  # actor_arch.h: tanh_f32 is within 2 ulp


def shapes(h1, h2):
    return dict(w0=(OBS, h1), b0=(h1,), w1=(h1, h2), b1=(h2,), w2=(h2, LOGITS), b2=(LOGITS,))


def params(style, h1, h2, seed=None):
    """actor_arch_ref's three styles, stored [in, out]: a: N(0, 1 / fan_in); b: orthogonal hidden layers (gain
    sqrt 2), biases N(0, 0.1), the head orthogonal x 0.3; c: hidden-layer magnitudes log-uniform over 2^-12 .. 2^2."""
    shp = shapes(h1, h2)
    seed = {"a": 41, "b": 42, "c": 43}[style] + 1000 * h1 + h2 if seed is None else seed
    g = torch.Generator().manual_seed(seed)
    if style == "a":
        return {k: R._randn(g, *shp[k]) / math.sqrt(shp[k][0]) for k in NAMES}
    if style == "b":
        p = {}
        for k in NAMES:
            if len(shp[k]) == 2:
                p[k] = R._orthogonal(g, shp[k][1], shp[k][0], 0.3 if k == "w2" else math.sqrt(2.0)).t().contiguous()
            else:
                p[k] = R._randn(g, *shp[k]) * 0.1
        return p
    p = params("a", h1, h2, seed + 100)
    for k in ("w0", "w1"):
        e = torch.rand(*shp[k], generator=g, dtype=torch.float64) * 14.0 - 12.0
        s = torch.where(torch.rand(*shp[k], generator=g) < 0.5, -1.0, 1.0).double()
        p[k] = (s * torch.exp2(e)).float()
    return p


# nominal raw brax observation [qpos 11, qvel 10]: hovering at z = 1, unit quaternion, props at rest
_NOMINAL = torch.tensor([0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0] + [0] * 10, dtype=torch.float32)
# running-statistics scales of a trained run's observations: positions of order 1, prop angles of hundreds of
# radians, prop rates of hundreds of rad/s
_RAW_STD = torch.tensor([0.8, 0.8, 0.5, 0.2, 0.3, 0.3, 0.3, 250, 250, 250, 250, 1.5, 1.5, 1.0, 3, 3, 2, 300, 300, 300,
                         300], dtype=torch.float32)
_RAW_MEAN = torch.tensor([0.05, -0.03, 0.9, 0.95, 0.01, -0.02, 0.03, 310, -290, 305, -300, 0.02, 0.01, -0.1, 0.1, -0.1,
                          0.05, 410, -405, 400, -398], dtype=torch.float32)
CLIP_FEATURE = 3  # the quaternion's w: constant over a run that never tilts, so its std sits at the 1e-6 clip

_SETS = {}


def obs_set(name, n=N_ROWS):
    """(obs [n, 21], mean [21], std [21]), built once and never modified.
    unit: U(-1, 1) observations, identity normaliser.
    raw : raw brax observations (positions of order 1, prop angles up to hundreds of radians, prop rates of hundreds
          of rad/s) with a trained run's running statistics.
    clip: the raw set with feature 3's std at RunningStats' 1e-6 clip and its observations within 8 ulp of the mean
          (the normalised feature is of order 1, formed from a difference of the last bits)."""
    if (name, n) in _SETS:
        return _SETS[(name, n)]
    g = torch.Generator().manual_seed({"unit": 51, "raw": 52, "clip": 53}[name] + n)
    if name == "unit":
        out = (torch.rand(n, OBS, generator=g) * 2 - 1, torch.zeros(OBS), torch.ones(OBS))
    else:
        x = _RAW_MEAN + _RAW_STD * torch.randn(n, OBS, generator=g).clamp(-3, 3)
        x[:, 7:11] = (torch.rand(n, 4, generator=g) * 2 - 1) * 800.0   # prop angles, hundreds of radians
        mean, std = _RAW_MEAN.clone(), _RAW_STD.clone()
        if name == "clip":
            std[CLIP_FEATURE] = 1e-6
            mean[CLIP_FEATURE] = 1.0
            k = torch.randint(-8, 9, (n,), generator=g).float()
            x[:, CLIP_FEATURE] = 1.0 + k * 2.0 ** -23
        out = (x.contiguous(), mean, std)
    _SETS[(name, n)] = out
    return out


def normalize32(obs, mean, std):
    """RunningStats.normalize in f32: the network's input, bit for bit what the kernel forms."""
    return (torch.as_tensor(obs, dtype=torch.float32) - mean.float()) / std.float()


def cases(h1, h2):
    """[(name, params, xh)]: the 3 styles x 3 observation sets for one arch; xh = the normalised f32 input."""
    return [(f"{s}-{o}", params(s, h1, h2), normalize32(*obs_set(o))) for s in STYLES for o in OBS_SETS]


def _act(activation):
    return {"relu": torch.relu, "tanh": torch.tanh, "silu": torch.nn.functional.silu}[activation]


def forward64(p, xh, activation):
    """logits [n, 8] in float64 on the CPU from the f32 normalised input."""
    f, x = _act(activation), R._d(xh)
    h = f(x @ R._d(p["w0"]) + R._d(p["b0"]))
    h = f(h @ R._d(p["w1"]) + R._d(p["b1"]))
    return h @ R._d(p["w2"]) + R._d(p["b2"])


def forward32(p, xh, activation):
    """BraxMLP.forward's f32 arithmetic (addmm on [in, out] kernels) on whatever device the tensors are on."""
    f = _act(activation)
    x = torch.as_tensor(xh, dtype=torch.float32)
    h = f(torch.addmm(p["b0"], x, p["w0"]))
    h = f(torch.addmm(p["b1"], h, p["w1"]))
    return torch.addmm(p["b2"], h, p["w2"])


def _linear_fixed(x, w, b):
    """x @ w + b in f32 with a summation order that no BLAS chooses: exact 8-wide dot products (formed in float64)
    added to the f32 accumulator one after the other, one f32 rounding each."""
    n, k = x.shape
    pad = (-k) % 8
    xd = torch.nn.functional.pad(x.double(), (0, pad)).view(n, -1, 8)
    wd = torch.nn.functional.pad(w.double(), (0, 0, 0, pad)).view(-1, 8, w.shape[1])
    acc = b.float().expand(n, -1)
    for c in range(xd.shape[1]):
        acc = (acc.double() + xd[:, c] @ wd[c]).float()
    return acc


def forward32_fixed(p, xh, activation):
    """The CPU tests' f32 yardstick: forward32's arithmetic with _linear_fixed's summation order and the activation
    rounded from float64. torch's own f32 matmul on the CPU sums in an order that depends on the BLAS, the
    instruction set and the thread count, and the count of broken forms outside the bar moved with it from one
    machine to the next (9 of 9 on one, 5 to 8 of 9 on another); this one gives the same bits everywhere."""
    f = _act(activation)
    g = lambda h: f(h.double()).float()
    x = torch.as_tensor(xh, dtype=torch.float32).cpu()
    h = g(_linear_fixed(x, p["w0"], p["b0"]))
    h = g(_linear_fixed(h, p["w1"], p["b1"]))
    return _linear_fixed(h, p["w2"], p["b2"])


def emulate_x3(p, xh, activation, terms=R.SIX):
    """policy_x3_ref's scheme model for this net: the piece products in `terms` for both hidden layers, exact
    products, f32 accumulation, the activation and the head in f32. A model of the scheme, not of the hardware."""
    f, terms = _act(activation), set(terms)
    g = lambda h: f(h.double()).float()   # rounded from float64: torch's vectorised f32 tanh / silu differ by
    x = torch.as_tensor(xh, dtype=torch.float32).cpu()   # instruction set, and a case at the bar's edge with them
    h = g(R._layer_x3(p["w0"].t(), p["b0"], x, terms))
    h = g(R._layer_x3(p["w1"].t(), p["b1"], h, terms))
    return _linear_fixed(h, p["w2"], p["b2"])


def make_net(p, h1, h2, activation, device="cpu"):
    """A BraxActorCritic whose policy holds `p`; the value net keeps its own init."""
    from uav_reinforcement_learning_control_amd.ppo.brax_ppo import BraxActorCritic, BraxPPOConfig
    net = BraxActorCritic(OBS, 4, BraxPPOConfig(policy_hidden_sizes=(h1, h2), activation=activation))
    with torch.no_grad():
        for i in range(3):
            net.policy.kernels[i].copy_(p[f"w{i}"])
            net.policy.biases[i].copy_(p[f"b{i}"])
    return net.to(device)


# ---------------------------------------------------------------- scalar models of the header's functions
def silu_model(x):
    """silu_f32 in numpy float32 (numpy's exp in libm's place)."""
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore"):
        e = np.exp(-x).astype(np.float32)
        return (x / (np.float32(1) + e)).astype(np.float32)


def softplus_model(x):
    x = np.asarray(x, np.float32)
    t = np.abs(x)
    l = np.log1p(np.exp(-t).astype(np.float32)).astype(np.float32)
    return (np.maximum(x, np.float32(0)) + l).astype(np.float32)


def tanh_model(x):
    """actor::tanh_f32 (csrc/actor_core.h) in numpy float32."""
    x = np.asarray(x, np.float32)
    t = np.abs(x)
    z = t * t
    p = np.float32(0.002142803743481636)
    for c in (-0.008177093230187893, 0.021700501441955566, -0.05394670367240906, 0.1333320587873459,
              -0.3333333134651184):
        p = (p.astype(np.float64) * z + np.float64(np.float32(c))).astype(np.float32)   # one fma rounding
    small = ((t * z).astype(np.float64) * p + t).astype(np.float32)
    with np.errstate(over="ignore"):
        e = np.exp(np.float32(2) * t).astype(np.float32)
    big = np.float32(1) - np.float32(2) / (e + np.float32(1))
    return np.copysign(np.where(t < np.float32(0.625), small, big), x).astype(np.float32)


def ulp_err(got32, ref64):
    """|got - ref| in ulps of the float64 result rounded to f32."""
    r = np.abs(np.asarray(ref64, np.float64).astype(np.float32))
    sp = np.nextafter(r, np.float32(np.inf)).astype(np.float64) - r.astype(np.float64)
    return np.abs(np.asarray(got32, np.float64) - np.asarray(ref64, np.float64)) / sp


# ---------------------------------------------------------------- the action draw (policy_net.h gauss4 on stream 0x400)
NOISE_STREAM = 0x400
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox4x32_10(counter, key):
    """Philox4x32-10 on uint32 arrays: counter [..., 4], key [..., 2] (Salmon et al., SC'11)."""
    c = [np.asarray(counter[..., i], np.uint64) for i in range(4)]
    k0, k1 = np.asarray(key[..., 0], np.uint64), np.asarray(key[..., 1], np.uint64)
    m32 = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k0) & m32, p1 & m32, ((p0 >> np.uint64(32)) ^ c[3] ^ k1) & m32, p0 & m32]
        k0, k1 = (k0 + np.uint64(_W0)) & m32, (k1 + np.uint64(_W1)) & m32
    return np.stack(c, -1).astype(np.uint32)


def normals(seed, env_ids, step):
    """z [n, 4] in float64: Box-Muller on Philox(seed; env, step, 0x400), the kernel's draw with exact functions."""
    env = np.asarray(env_ids, np.uint64)
    ctr = np.stack([env & np.uint64(0xFFFFFFFF), env >> np.uint64(32), np.full(env.shape, step, np.uint64),
                    np.full(env.shape, NOISE_STREAM, np.uint64)], -1)
    key = np.broadcast_to(np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], np.uint64), env.shape + (2,))
    c = philox4x32_10(ctr, key).astype(np.float64)
    z = np.empty(env.shape + (4,))
    for k in range(2):
        u1 = (np.floor(c[..., 2 * k] / 256.0) + 1.0) * 2.0 ** -24
        u2 = np.floor(c[..., 2 * k + 1] / 256.0) * 2.0 ** -24
        r = np.sqrt(-2.0 * np.log(u1))
        z[..., 2 * k], z[..., 2 * k + 1] = r * np.cos(2 * np.pi * u2), r * np.sin(2 * np.pi * u2)
    return z


Z_BAR = 1e-5  # |z_kernel - z| <= Z_BAR (1 + |z|): tests/test_gpu_policy.py's bar for the hardware log / sin / cos


def action_bound(logits, z, deterministic):
    """(want, bound): the env action in float64 from the kernel's own logits and |got - want|'s bound from the
    stated ulps: tanh_f32's 2 ulp of the result, plus (|d tanh| <= 1) the argument's error -- softplus's
    SOFTPLUS_ULP ulps of the scale times |z|, the draw's Z_BAR, and three f32 roundings (scale + min_std, the
    product, the sum)."""
    lg = np.asarray(logits, np.float64)
    eps = 2.0 ** -24
    if deterministic:
        want = np.tanh(lg[:, :4])
        return want, TANH_ULP * 2 * eps * np.maximum(np.abs(want), 2.0 ** -126)
    sp = np.logaddexp(lg[:, 4:], 0.0)
    scale = sp + MIN_STD
    pre = lg[:, :4] + scale * z
    want = np.tanh(pre)
    d_pre = (header_ulp("SOFTPLUS_ULP") * 2 * eps * sp * np.abs(z) + scale * Z_BAR * (1 + np.abs(z))
             + eps * (scale * np.abs(z) * 2 + np.abs(pre)) * 2)
    return want, TANH_ULP * 2 * eps * np.maximum(np.abs(want), 2.0 ** -126) + d_pre


# ---------------------------------------------------------------- the closed loop's own sensitivity (float64 oracle)
# 256 brax_jax_mjx oracle episodes of up to 128 steps under a hover-biased (256, 256) SiLU policy, deterministic
# (action = tanh(loc)): the physical action is (a + 1) / 2 x [0, 52] N of total thrust and [-max, max] of each
# torque, so the thrust head's bias is the hover thrust and the torque heads' is zero; a style-a net of gain
# LOOP_GAIN (the torque heads LOOP_TORQUE_GAIN of that) on observations normalised by the first steps' scale tips
# most envs over before the limit and leaves the rest flying.
LOOP_SEED, LOOP_ENVS, LOOP_STEPS, LOOP_ARCH = 7, 256, 128, (256, 256, "silu")
LOOP_PARAM_SEED, LOOP_GAIN, LOOP_TORQUE_GAIN = 77, 0.1, 0.025
# share of those envs whose (status, steps) change when the action moves by +1 / -1 f32 ulp (oracle_ulp_share();
# tests/test_brax_actor_cpu.py re-measures it)
ORACLE_ULP_SHARE = 0.0
HOVER_THRUST_ACTION = 2.0 * 0.2227 * 9.81 / 52.0 - 1.0


def loop_params():
    h1, h2, _ = LOOP_ARCH
    p = params("a", h1, h2, LOOP_PARAM_SEED)
    p["w2"] = p["w2"] * LOOP_GAIN
    p["w2"][:, 1:4] *= LOOP_TORQUE_GAIN
    p["w2"][:, 4:] = 0.0
    p["b2"] = torch.tensor([math.atanh(HOVER_THRUST_ACTION), 0.0, 0.0, 0.0, -2.0, -2.0, -2.0, -2.0])
    return p


def loop_norm():
    """(mean, std): the nominal state and the scale of the first steps' observations."""
    std = torch.tensor([0.02] * 3 + [0.02] * 4 + [100.0] * 4 + [0.05] * 3 + [0.05] * 3 + [100.0] * 4)
    return _NOMINAL.clone(), std


def oracle_episodes(p, activation, ulps, seed=LOOP_SEED, n=LOOP_ENVS, steps=LOOP_STEPS, kind=None):
    """(status, steps, return) per env on the float64 oracle env with the float64 forward: the action
    tanh(loc) rounded to f32 and moved by `ulps` f32 ulps. status: 0 running at the limit, 1 terminated, 2
    truncated."""
    from oracle import oracle as O
    kind = O.ENV_BRAX_TRAJ if kind is None else kind
    envs = [O.BraxEnv(kind, 500) for _ in range(n)]
    obs = np.stack([e.reset_with(e.draw(seed, i, 0)) for i, e in enumerate(envs)]).astype(np.float32)
    mean, std = loop_norm()
    status, length, ret = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.float64)
    for _ in range(steps):
        if status.all():
            break
        lg = forward64(p, normalize32(torch.from_numpy(obs), mean, std), activation).numpy()
        act = np.tanh(lg[:, :4]).astype(np.float32)
        for _ in range(abs(ulps)):
            act = np.nextafter(act, np.float32(np.inf if ulps > 0 else -np.inf))
        for i, e in enumerate(envs):
            if status[i]:
                continue
            out = e.step(act[i], auto_reset=False)
            length[i] += 1
            ret[i] += out["reward"]
            obs[i] = out["obs"]
            if out["terminated"] or out["truncated"]:
                status[i] = 1 if out["terminated"] else 2
    return status, length, ret


_SHARE = {}


def oracle_ulp_share():
    """(share, status, steps, return, largest |return change|): the larger of the two shares of envs whose
    (status, steps) differ between the +1 ulp / -1 ulp runs and the unperturbed one, the unperturbed run, and the
    largest return change among the envs that agree. Computed once."""
    if not _SHARE:
        p, act = loop_params(), LOOP_ARCH[2]
        s0, l0, r0 = oracle_episodes(p, act, 0)
        shares, dret = [], 0.0
        for u in (1, -1):
            s, l, r = oracle_episodes(p, act, u)
            same = (s == s0) & (l == l0)
            shares.append(float((~same).mean()))
            dret = max(dret, float(np.abs(r - r0)[same].max()))
        _SHARE["v"] = (max(shares), s0, l0, r0, dret)
    return _SHARE["v"]
