"""The general learner (quad_ppo_arch_grad, ppo/learner.py FusedArchLearner) without a GPU: the chooser and its error
text, PPOConfig.fused_update_arch on a CPU device and outside the family, the host-side argument checks, and the
float64 restatement of the kernels' backward pass against autograd."""
import ctypes as C

import pytest
import torch

import learner_arch_ref as R
from uav_reinforcement_learning_control_amd import _native as N
from uav_reinforcement_learning_control_amd.ppo import PPO, PPOConfig
from uav_reinforcement_learning_control_amd.ppo.learner import (ARCH_UPDATE_KEEP_TORCH, FusedArchLearner, FusedLearner,
                                                                arch_of_learner, fused_learner_for)
from uav_reinforcement_learning_control_amd.ppo.policy import ActorCritic


class _StubEnv:
    """What PPO's constructor and torch update path read of an env."""
    num_envs, obs_dim, device = 8, 12, torch.device("cpu")


def test_chooser_picks_the_specialised_learner_for_128_relu_and_the_general_one_elsewhere():
    # on a CPU module each class refuses in its own name, after the chooser chose it
    with pytest.raises(N.QuadError, match=r"^FusedLearner needs"):
        fused_learner_for(ActorCritic(), 0.2, 0.0, 0.5)
    for hidden, act in (((64, 64), "tanh"), ((128, 128), "tanh"), ((256, 256), "relu"), ((512, 256), "tanh"),
                        ((96, 64), "relu")):
        with pytest.raises(N.QuadError, match=r"^FusedArchLearner needs"):
            fused_learner_for(ActorCritic(12, 4, hidden, activation=act), 0.2, 0.0, 0.5)
        arch = arch_of_learner(ActorCritic(12, 4, hidden, activation=act))
        assert (arch.h1, arch.h2, arch.activation) == (*hidden, N.ACTFNS[act])
    assert issubclass(FusedArchLearner, FusedLearner)
    assert isinstance(ARCH_UPDATE_KEEP_TORCH, frozenset)


@pytest.mark.parametrize("hidden,obs_dim", [((128, 32), 12), ((100, 64), 12), ((544, 64), 12), ((64, 64, 64), 12),
                                            ((64, 64), 7)])
def test_chooser_names_the_family_outside_it(hidden, obs_dim):
    with pytest.raises(ValueError, match=r"H1 a multiple of 32 up to 512, H2 in \(64, 128, 256\), relu / tanh"):
        fused_learner_for(ActorCritic(obs_dim, 4, hidden), 0.2, 0.0, 0.5)


def test_chooser_checks_the_value_net_too():
    pol = ActorCritic(12, 4, (64, 64), activation="tanh")
    pol.mlp_extractor.value_net[2] = torch.nn.Linear(64, 128)
    pol.value_net = torch.nn.Linear(128, 1)
    with pytest.raises(ValueError, match="same widths"):
        fused_learner_for(pol, 0.2, 0.0, 0.5)


def test_flag_raises_outside_the_family_and_is_off_by_default():
    assert PPOConfig().fused_update_arch is False
    for hidden in ((100, 64), (128, 32), (544, 64)):
        with pytest.raises(ValueError, match="H1 a multiple of 32"):
            PPO(_StubEnv(), PPOConfig(net_arch=hidden, n_steps=16, fused_update_arch=True), seed=1)
        PPO(_StubEnv(), PPOConfig(net_arch=hidden, n_steps=16), seed=1)  # without the flag: the torch path, as ever


def test_flag_leaves_a_cpu_device_ppo_on_the_torch_path():
    cfg = PPOConfig(activation="tanh", net_arch=(64, 64), n_steps=16, n_minibatches=4, n_epochs=1,
                    fused_update_arch=True)
    ppo = PPO(_StubEnv(), cfg, seed=1)
    assert ppo._fp is None and ppo._learner is None and ppo._adam is None and not ppo._one_launch
    g = torch.Generator().manual_seed(5)
    for buf, scale, shift in ((ppo.buf_obs, 1, 0), (ppo.buf_act, 1, 0), (ppo.buf_logp, 0.1, -5.7), (ppo.buf_adv, 1, 0),
                              (ppo.buf_ret, 1, 0)):
        buf.copy_(torch.randn(buf.shape, generator=g) * scale + shift)
    before = [p.detach().clone() for p in ppo.params]
    stats = ppo.train(n_epochs=1, max_minibatches=1)
    assert stats["n"] == 1
    assert any(not torch.equal(a, b.detach()) for a, b in zip(before, ppo.params))


def test_workspace_size_and_argument_checks_need_no_device():
    L = N.lib()
    size = lambda h1, h2, a, b: L.quad_ppo_arch_workspace_bytes(C.byref(N.QuadActorArch(h1=h1, h2=h2, activation=a)), b)
    for h1, h2 in R.ARCHS:
        for a in (0, 1):
            s128, s4096, s1m = size(h1, h2, a, 128), size(h1, h2, a, 4096), size(h1, h2, a, 1 << 20)
            assert 0 < s128 < s4096 < s1m
            # the hidden images of every row: x [16], and h1, dh2, dh1 of both nets
            assert s1m >= (1 << 20) * 4 * (16 + 2 * (2 * h1 + h2))
            assert size(h1, h2, a, 33) == size(h1, h2, a, 64)  # rows are padded to the 64-row chunk
    for h1, h2, a in ((128, 32, 0), (100, 64, 0), (544, 64, 0), (0, 64, 0), (64, 512, 0), (64, 64, 2)):
        assert size(h1, h2, a, 128) <= 0
    assert size(64, 64, 1, 0) <= 0
    assert L.quad_ppo_arch_workspace_bytes(None, 128) <= 0
    arch = N.QuadActorArch(h1=64, h2=64, activation=1)
    assert L.quad_ppo_arch_grad(C.byref(arch), None, None, None, None, 0, None) == N.QUAD_EINVAL
    assert L.quad_ppo_arch_grad(None, None, None, None, None, 0, None) == N.QUAD_EINVAL


@pytest.mark.parametrize("activation", ["tanh", "relu"])
@pytest.mark.parametrize("hidden", [(64, 64), (96, 64)])
def test_backward_restatement_matches_autograd(hidden, activation):
    """The backward pass as the kernels decompose it -- act' from the stored activation, db1 from the 1.0 column --
    is the gradient autograd forms, in float64 to 1e-10."""
    g = torch.Generator().manual_seed(3)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    h1, h2 = hidden
    x, d_out = rnd(37, 12), rnd(37, 4)
    ws = [rnd(h1, 12) * 0.4, rnd(h1) * 0.1, rnd(h2, h1) * 0.2, rnd(h2) * 0.1, rnd(4, h2), rnd(4)]
    leaves = [w.clone().requires_grad_(True) for w in ws]
    act = torch.tanh if activation == "tanh" else torch.relu
    out = act(act(x @ leaves[0].T + leaves[1]) @ leaves[2].T + leaves[3]) @ leaves[4].T + leaves[5]
    (out * d_out).sum().backward()
    got = R.mlp_backward(x, *ws, d_out, activation)
    for a, leaf in zip(got, leaves):
        scale = leaf.grad.abs().max().item()
        assert (a - leaf.grad).abs().max().item() <= 1e-10 * max(scale, 1.0)
