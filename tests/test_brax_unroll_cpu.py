"""The Brax unroll's host side without a GPU: the defaults stay off, brax_unroll_supported's refusals, the
ctypes QuadBraxUnroll against the header's layout, the exports, and the float64 NumPy restatement of
NormalTanh.log_prob that tests/test_gpu_brax_unroll.py uses as its yardstick against torch's float64."""
import ctypes as C
import os
import subprocess

import numpy as np
import torch

import brax_actor_ref as B
import brax_unroll_ref as U
from uav_reinforcement_learning_control_amd import _native as N
from uav_reinforcement_learning_control_amd import train_brax
from uav_reinforcement_learning_control_amd.ppo.brax_ppo import BraxPPOConfig, NormalTanh
from uav_reinforcement_learning_control_amd.ppo.fused import BRAX_UNROLL_KEEP_LOOP, brax_unroll_supported

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_launch_is_off_by_default():
    assert BraxPPOConfig().fused_unroll is False
    assert train_brax.parse([]).fused_unroll is False
    assert train_brax.parse(["--fused-unroll"]).fused_unroll is True


class _Env:
    """What brax_unroll_supported reads of an env."""

    def __init__(self, kind, auto_reset=1, handle=object()):
        self.cfg = N.QuadCfg()
        self.cfg.env_kind, self.cfg.auto_reset = kind, auto_reset
        self._h = handle


def test_brax_unroll_supported_refuses_what_the_launch_cannot_fly():
    ok = _Env(N.ENV_BRAX_TRAJ)
    assert brax_unroll_supported((128, 128), "relu", ok) == (((128, 128), "relu") not in BRAX_UNROLL_KEEP_LOOP)
    assert brax_unroll_supported((64, 64), "silu", _Env(N.ENV_BRAX_HOVER)) == (
        ((64, 64), "silu") not in BRAX_UNROLL_KEEP_LOOP)
    assert not brax_unroll_supported((128, 128), "relu", _Env(N.ENV_HOVER))           # not a brax kind
    assert not brax_unroll_supported((128, 128), "relu", _Env(N.ENV_BRAX_TRAJ, handle=None))
    assert not brax_unroll_supported((128, 128), "relu", object())                    # no cfg at all
    assert not brax_unroll_supported((128, 128), "relu", _Env(N.ENV_BRAX_TRAJ, auto_reset=0))
    for sizes, act in (((64, 64, 64), "relu"), ((128, 32), "relu"), ((48, 64), "tanh"), ((1024, 64), "relu"),
                       ((128,), "relu"), ((128, 128), "gelu")):
        assert not brax_unroll_supported(sizes, act, ok), (sizes, act)


def test_ctypes_unroll_struct_has_the_headers_layout(tmp_path):
    header = os.path.join(ROOT, "include", "quadenv.h")
    fields = [n for n, _ in N.QuadBraxUnroll._fields_]
    prog = tmp_path / "layout.c"
    offs = ", ".join(f"offsetof(QuadBraxUnroll, {f})" for f in fields)
    fmt = " ".join(["%zu"] * (len(fields) + 1))
    prog.write_text(f'''#include <stdio.h>
#include <stddef.h>
#include "{os.path.abspath(header)}"
int main(void) {{
  printf("{fmt} %d %d\\n", sizeof(QuadBraxUnroll), {offs}, QUAD_POLICY_STAT_SLOTS, QUADENV_ABI_VERSION);
  return 0;
}}''')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(prog)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    want = [C.sizeof(N.QuadBraxUnroll)] + [getattr(N.QuadBraxUnroll, f).offset for f in fields] + \
           [N.POLICY_STAT_SLOTS, N.ABI_VERSION]
    assert got == want and got[0] == 96
    assert fields == ["obs", "raw", "log_prob", "reward", "discount", "truncation", "next_obs", "ep_ret", "stats",
                      "steps", "unroll_length", "noise_step0", "seed"]


def test_the_new_entry_points_are_exported():
    assert "quad_brax_actor_sample" in N.EXPORTS and "quad_brax_unroll" in N.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "quadenv.h")).read()
    assert "int quad_brax_actor_sample(" in hdr and "int quad_brax_unroll(" in hdr


def test_numpy_log_prob_is_torchs_float64():
    """brax_unroll_ref.log_prob64 against NormalTanh.log_prob on float64 tensors: ordinary logits, and the hand-built
    case's range (scale at min_std, |raw| up to 8 and beyond), to a few float64 roundings of the largest term. One
    difference is torch's own: F.softplus returns x itself above its threshold of 20, short of log(1 + e^x) by up to
    e^-20; that enters the log-det doubled, once per component with -2 raw > 20, and is allowed for exactly there."""
    g = torch.Generator().manual_seed(5)
    dist = NormalTanh(4, B.MIN_STD)
    n = 4096
    sets = []
    lg = torch.randn(n, 8, generator=g, dtype=torch.float64)
    sets.append((lg, lg[:, :4] + torch.randn(n, 4, generator=g, dtype=torch.float64)))
    lg = torch.cat([(torch.rand(n, 4, generator=g, dtype=torch.float64) * 2 - 1) * U.HAND_LOC_GAIN,
                    U.HAND_SCALE_BIAS + (torch.rand(n, 4, generator=g, dtype=torch.float64) * 2 - 1) * U.HAND_SCALE_GAIN], 1)
    lg[: n // 4, 4:] = -20.0
    scale = torch.nn.functional.softplus(lg[:, 4:]) + B.MIN_STD
    sets.append((lg, lg[:, :4] + scale * torch.randn(n, 4, generator=g, dtype=torch.float64)))
    sets.append((lg.float().double(), (lg[:, :4] * 1.5).float().double()))   # far from loc: |t| in the thousands
    for lg, raw in sets:
        want = dist.log_prob(lg, raw).numpy()
        got = U.log_prob64(lg.numpy(), raw.numpy())
        assert got.dtype == np.float64 and got.shape == (n,)
        cut = 2.0 * np.exp(-20.0) * (-2.0 * raw.numpy() > 20.0).sum(-1)
        assert np.all(np.abs(got - want) <= 64 * np.finfo(np.float64).eps * np.maximum(np.abs(want), 1.0) + cut)
    assert float(scale.min()) < B.MIN_STD * (1 + 1e-5) and float(sets[1][1].abs().max()) >= 7.9


def test_hand_built_net_makes_the_logits_linear_in_the_observation():
    """The hand-built case's premise, on the float64 forward: logit q = a_q x_q + b_q."""
    p, x = U.hand_params(), U.hand_obs()
    lg = B.forward64(p, x, U.HAND_ARCH[2]).numpy()
    xd = x.double().numpy()
    assert np.allclose(lg[:, :4], U.HAND_LOC_GAIN * xd[:, :4], rtol=0, atol=1e-12)
    assert np.allclose(lg[:, 4:], U.HAND_SCALE_BIAS + U.HAND_SCALE_GAIN * xd[:, 4:8], rtol=0, atol=1e-12)
    assert lg[:, 4:].min() == -20.0 and np.abs(lg[:, :4]).max() == 8.0
