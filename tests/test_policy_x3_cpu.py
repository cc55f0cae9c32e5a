"""The accuracy bar of tests/test_gpu_policy_precision.py can tell the bf16x3 scheme from its broken
forms on the very inputs the GPU test uses, before any GPU is involved (tests/policy_x3_ref.py).

Per case of cases() (3 policies x 3 observation sets, 4,096 rows), float64 as the reference and
torch CPU fp32 as the yardstick: the six-term model of policy_net.h's scheme is within
max|d| <= 4 max|d_torch32| + 1e-7 max|ref| on mean, value and log_prob; with any one of the small
terms a2b0 / a1b1 / a0b2 removed, or with two pieces per operand, it is outside that bar on BOTH the
mean (the actor) and the value (the critic). If a case stops separating, change the case, not the bar.
"""
import numpy as np
import pytest
import torch

import policy_x3_ref as R

_CASES = R.cases()


@pytest.fixture(scope="module")
def refs():
    out = {}
    for name, p, obs in _CASES:
        mean64, v64 = R.forward64(p, obs)
        pol = R.make_policy(p)
        with torch.no_grad():
            mean32, v32 = pol.forward_heads(obs)
        out[name] = (mean64, v64, mean32, v32, pol)
    return out


def test_bounds_are_the_hover_defaults():
    from oracle import oracle as O
    cfg = O.default_cfg(O.ENV_HOVER, O.WRAP_NONE)
    assert np.array_equal(np.array(cfg.term_low[:], np.float32), R.HOVER_TERM_LOW)
    assert np.array_equal(np.array(cfg.term_high[:], np.float32), R.HOVER_TERM_HIGH)


def test_cases_hold_what_they_claim():
    names = [c[0] for c in _CASES]
    assert len(set(names)) == 9
    for name, p, obs in _CASES:
        assert obs.shape == (R.N_ROWS, 12) and obs.dtype == torch.float32
        assert all(tuple(p[k].shape) == R.SHAPES[k] and p[k].dtype == torch.float32 for k in R.NAMES)
    ex = R.obs_exact()
    m, _ = torch.frexp(ex[ex != 0])
    assert (ex == 0).sum() > 1000 and (m.abs() == 0.5).sum() > 1000
    w = R.policy_c()["pi_w1"].abs()
    assert w.min() < 2.0 ** -11 and w.max() > 2.0 and w.max() <= 4.0
    # the pieces: x = p0 + p1 + p2 to 2^-24 |x| and each piece a bf16
    x = R.obs_bounds()
    p = R.split3(x)
    assert ((p[0] + p[1] + p[2] - x.double()).abs() <= 2.0 ** -24 * x.double().abs()).all()
    assert all(torch.equal(q.float().bfloat16().double(), q) for q in p)


@pytest.mark.parametrize("name,p,obs", _CASES, ids=[c[0] for c in _CASES])
def test_six_terms_inside_the_bar(name, p, obs, refs):
    mean64, v64, mean32, v32, pol = refs[name]
    mean, v = R.emulate_x3(p, obs)
    acts = R.noisy_actions(p, obs)
    with torch.no_grad():
        lp, lp32 = pol.log_prob(mean, acts), pol.log_prob(mean32, acts)
    for what, got, ref, g32 in (("mean", mean, mean64, mean32), ("value", v, v64, v32),
                                ("log_prob", lp, R.log_prob64(p, mean64, acts), lp32)):
        err, err32, scale, ratio = R.errors(got, ref, g32)
        print(f"{name} six {what}: err {err:.3g} torch32 {err32:.3g} ratio {ratio:.2f} scale {scale:.3g}")
        assert R.within_bar(got, ref, g32), (what, err, err32, scale)


@pytest.mark.parametrize("variant", list(R.VARIANTS))
@pytest.mark.parametrize("name,p,obs", _CASES, ids=[c[0] for c in _CASES])
def test_broken_forms_outside_the_bar(name, p, obs, variant, refs):
    mean64, v64, mean32, v32, _ = refs[name]
    mean, v = R.emulate_x3(p, obs, R.VARIANTS[variant])
    for what, got, ref, g32 in (("mean", mean, mean64, mean32), ("value", v, v64, v32)):
        err, err32, scale, ratio = R.errors(got, ref, g32)
        print(f"{name} {variant} {what}: err {err:.3g} torch32 {err32:.3g} ratio {ratio:.2f}")
        assert not R.within_bar(got, ref, g32), (what, err, err32, scale)
