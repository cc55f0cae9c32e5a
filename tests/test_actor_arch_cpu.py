"""The general actor (csrc/actor_arch.h: 12 -> h1 -> h2 -> 4, ReLU / tanh) on the CPU: the bf16x3 scheme model at
every test arch against policy_x3_ref's bar, the bar's power to tell a broken scheme, and the Python layers that
carry a tanh / wider policy from an SB3 archive to the dispatch (ActorCritic, export, PPOConfig, FusedPolicy's
shape check). No GPU and no native call besides the library load."""
import io
import json
import zipfile

import pytest
import torch

import actor_arch_ref as A
import policy_x3_ref as R
from uav_reinforcement_learning_control_amd import export as X
from uav_reinforcement_learning_control_amd.ppo import ActorCritic, PPOConfig

_ARCH_ACT = [(h1, h2, act) for h1, h2 in A.ARCHS for act in A.ACTIVATIONS]
_IDS = [f"{h1}x{h2}-{act}" for h1, h2, act in _ARCH_ACT]


@pytest.fixture(scope="module")
def refs():
    """Per (arch, activation), built once: [(case name, params, obs, float64 mean, torch f32 mean)]."""
    cache = {}

    def get(h1, h2, act):
        if (h1, h2, act) not in cache:
            cache[(h1, h2, act)] = [(name, p, obs, A.forward64(p, obs, act), A.forward32(p, obs, act))
                                    for name, p, obs in A.cases(h1, h2)]
        return cache[(h1, h2, act)]
    return get


@pytest.mark.parametrize("h1,h2,act", _ARCH_ACT, ids=_IDS)
def test_six_terms_inside_the_bar(h1, h2, act, refs):
    """The full six-product scheme, in the kernel's role, against float64 with torch-CPU f32 as the yardstick:
    inside policy_x3_ref.within_bar on all nine (style, observation set) cases of every test arch."""
    bad = []
    for name, p, obs, m64, m32 in refs(h1, h2, act):
        got = A.emulate_x3(p, obs, act)
        err, err32, scale, ratio = R.errors(got, m64, m32)
        print(f"RATIO {h1}x{h2} {act} {name}: err {err:.3g} torch32 {err32:.3g} ratio {ratio:.2f}")
        if not R.within_bar(got, m64, m32):
            bad.append((name, ratio))
    assert not bad, bad


@pytest.mark.parametrize("variant", list(R.VARIANTS))
@pytest.mark.parametrize("h1,h2,act", _ARCH_ACT, ids=_IDS)
def test_broken_forms_outside_the_bar(h1, h2, act, variant, refs):
    """A dropped small term or a two-piece split is outside the bar in at least one case of every arch: the bar
    discriminates at these widths and with tanh as it does for the 128 ReLU net."""
    out = [name for name, p, obs, m64, m32 in refs(h1, h2, act)
           if not R.within_bar(A.emulate_x3(p, obs, act, R.VARIANTS[variant]), m64, m32)]
    print(f"{h1}x{h2} {act} {variant}: outside the bar in {len(out)} of 9 cases")
    assert out, f"{variant} is inside the bar in every case of {h1}x{h2} {act}"


def test_oracle_loop_sensitivity_is_the_recorded_share():
    """The bound of test_gpu_actor_arch's fused-against-torch-loop check: 256 hover + CTBR episodes of up to 128
    steps (seed 5, the (256, 256) tanh policy of actor_arch_ref.loop_params) on the float64 oracle env with the
    float64 forward, flown with the f32-rounded means as they are and moved by +1 and by -1 ulp. Measured: no
    env's (status, steps) changes (share 0.0, under the 5 % the check needs), while the episodes are not all
    alike: 135 terminate before step 128 (the earliest at 28) and 121 reach the limit."""
    share, status, length = A.oracle_ulp_share()
    print(f"ORACLE share {share:.4f}; terminated {(status == 1).sum()}, at the limit {(length == A.LOOP_STEPS).sum()}, "
          f"shortest {length.min()}")
    assert share == A.ORACLE_ULP_SHARE and share < 0.05
    assert (status == 1).sum() >= 64 and (length == A.LOOP_STEPS).sum() >= 64


def test_tanh_actor_critic_equals_a_hand_written_forward():
    torch.manual_seed(3)
    pol = ActorCritic(12, 4, (96, 64), activation="tanh")
    assert pol.activation == "tanh" and ActorCritic().activation == "relu"
    sd = pol.state_dict()
    assert [k for k in sd if k.startswith("mlp_extractor.policy_net")] == [
        "mlp_extractor.policy_net.0.weight", "mlp_extractor.policy_net.0.bias",
        "mlp_extractor.policy_net.2.weight", "mlp_extractor.policy_net.2.bias"]
    x = torch.randn(50, 12)
    lin = torch.nn.functional.linear
    want = []
    for net, head in (("policy_net", "action_net"), ("value_net", "value_net")):
        h = torch.tanh(lin(x, sd[f"mlp_extractor.{net}.0.weight"], sd[f"mlp_extractor.{net}.0.bias"]))
        h = torch.tanh(lin(h, sd[f"mlp_extractor.{net}.2.weight"], sd[f"mlp_extractor.{net}.2.bias"]))
        want.append(lin(h, sd[f"{head}.weight"], sd[f"{head}.bias"]))
    with torch.no_grad():
        mean, value = pol.forward_heads(x)
    assert torch.equal(mean, want[0]) and torch.equal(value, want[1][:, 0])
    with pytest.raises(ValueError):
        ActorCritic(activation="gelu")


def test_tanh_archive_round_trips(tmp_path):
    torch.manual_seed(4)
    pol = ActorCritic(12, 4, (256, 256), activation="tanh")
    path = X.save_sb3_zip(str(tmp_path / "tanh.zip"), pol)
    with zipfile.ZipFile(path) as z:
        data = json.loads(z.read("data"))
        sd = torch.load(io.BytesIO(z.read("policy.pth")), map_location="cpu", weights_only=True)
    assert "Tanh" in data["policy_kwargs"]["activation_fn"] and "ReLU" not in data["policy_kwargs"]["activation_fn"]
    assert data["policy_kwargs"]["net_arch"] == [256, 256]
    assert all(torch.equal(sd[k], v) for k, v in pol.state_dict().items())
    with pytest.raises(ValueError):
        X.load_sb3_policy(path)                      # the default admits ReLU only
    got = X.load_sb3_policy(path, activations=("relu", "tanh"))
    assert got.activation == "tanh" and isinstance(got.mlp_extractor.policy_net[1], torch.nn.Tanh)
    assert all(torch.equal(v, got.state_dict()[k]) for k, v in pol.state_dict().items())
    x = torch.randn(9, 12)
    with torch.no_grad():
        assert torch.equal(got.forward_heads(x)[0], pol.forward_heads(x)[0])
    # a ReLU module still writes ReLU, and evaluate's loader takes both
    from uav_reinforcement_learning_control_amd.evaluate import load_policy
    relu = X.save_sb3_zip(str(tmp_path / "relu.zip"), ActorCritic())
    assert "ReLU" in json.loads(zipfile.ZipFile(relu).read("data"))["policy_kwargs"]["activation_fn"]
    assert load_policy(path, "cpu")[0].activation == "tanh" and load_policy(relu, "cpu")[0].activation == "relu"


class _StubEnv:
    """What PPO's constructor and torch update path read of an env."""
    num_envs, obs_dim, device = 8, 12, torch.device("cpu")


def test_tanh_config_builds_a_torch_path_learner_and_updates():
    from uav_reinforcement_learning_control_amd.ppo import PPO
    cfg = PPOConfig(activation="tanh", net_arch=(64, 64), n_steps=16, n_minibatches=4, n_epochs=1)
    ppo = PPO(_StubEnv(), cfg, seed=1)
    assert ppo.policy.activation == "tanh" and isinstance(ppo.policy.mlp_extractor.value_net[3], torch.nn.Tanh)
    assert ppo._fp is None and ppo._learner is None and not ppo._one_launch
    # a 128-128 tanh config is not fusable either
    ppo128 = PPO(_StubEnv(), PPOConfig(activation="tanh", n_steps=16), seed=1)
    assert ppo128._fp is None and ppo128._learner is None
    g = torch.Generator().manual_seed(5)
    ppo.buf_obs.copy_(torch.randn(ppo.buf_obs.shape, generator=g))
    ppo.buf_act.copy_(torch.randn(ppo.buf_act.shape, generator=g))
    ppo.buf_logp.copy_(torch.randn(ppo.buf_logp.shape, generator=g) * 0.1 - 5.7)
    ppo.buf_adv.copy_(torch.randn(ppo.buf_adv.shape, generator=g))
    ppo.buf_ret.copy_(torch.randn(ppo.buf_ret.shape, generator=g))
    before = [p.detach().clone() for p in ppo.params]
    stats = ppo.train(n_epochs=1, max_minibatches=1)
    assert stats["n"] == 1 and all(map(lambda v: v == v, (stats["pg_loss"], stats["vf_loss"])))
    assert any(not torch.equal(a, b.detach()) for a, b in zip(before, ppo.params))


def test_fused_policy_refuses_a_128_tanh_module():
    from uav_reinforcement_learning_control_amd.ppo.fused import FusedActor, FusedPolicy
    FusedPolicy._check_shapes(ActorCritic())
    with pytest.raises(ValueError, match="ReLU"):
        FusedPolicy._check_shapes(ActorCritic(activation="tanh"))
    # the family's edge: what FusedActor admits and what falls back to torch
    arch = FusedActor.arch_of(ActorCritic(12, 4, (512, 256), activation="tanh"))
    assert (arch.h1, arch.h2, arch.activation) == (512, 256, 1)
    for hidden, obs_dim in (((128, 32), 12), ((100, 64), 12), ((544, 64), 12), ((64, 64, 64), 12), ((64, 64), 7)):
        with pytest.raises(ValueError):
            FusedActor.arch_of(ActorCritic(obs_dim, 4, hidden))


def test_packed_size_and_arch_checks_need_no_device():
    import ctypes as C
    from uav_reinforcement_learning_control_amd import _native as N
    L = N.lib()
    size = lambda h1, h2, a=0: L.quad_actor_packed_floats(C.byref(N.QuadActorArch(h1=h1, h2=h2, activation=a)))
    # B1 + B2 + W3 + B3 + W1 pieces, then 2 k-steps per (layer-1 block, layer-2 block) of 768 floats each
    for h1, h2 in A.ARCHS:
        nb1, mb = h1 // 32, h2 // 32
        assert size(h1, h2) == size(h1, h2, 1) == h1 + h2 + 4 * h2 + 4 + nb1 * 768 + nb1 * 2 * mb * 768
    for h1, h2, a in ((0, 64, 0), (48, 64, 0), (544, 64, 0), (64, 32, 0), (64, 512, 0), (64, 64, 2)):
        assert size(h1, h2, a) < 0 and b"actor arch" in L.quad_last_error()
    arch = N.QuadActorArch(h1=64, h2=64, activation=0)
    assert L.quad_actor_act(C.byref(arch), None, None, None, None, 4, None) == N.QUAD_EINVAL
    assert L.quad_actor_pack(C.byref(arch), None, None, None) == N.QUAD_EINVAL
    assert L.quad_actor_episode(None, C.byref(arch), None, None, None) == N.QUAD_EINVAL
