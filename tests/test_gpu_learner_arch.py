"""The general learner's minibatch gradient (csrc/learner_arch.hip, quad_ppo_arch_grad; ppo/learner.py
FusedArchLearner) against torch autograd of ppo_loss in float64, with tests/test_gpu_learner.py's inputs and bar
restated for any architecture of the family (tests/learner_arch_ref.py): per gradient tensor
|d| <= 1e-4 max|g64| + 4 err_torch32 + 1e-9 and |d| <= 4 err_torch32 + 1e-6 max|g64| + 1e-9, statistics to rtol 1e-4 /
atol 1e-7. ReLU nets draw their rows from those whose float64 hidden pre-activations are all at least 1e-5 from zero
(a ReLU decision within f32 rounding of zero is a discontinuity of the loss, not an accuracy statement); tanh nets
take every row. Then: the advantage modes, determinism and the gather, the argument checks, FusedAdam on a wide
net, PPO.train with the flag against the torch update, and a short learning run of the training driver."""
import copy
import ctypes as C
import functools
import json
import math
import os
import zlib

import numpy as np
import pytest
import torch

import learner_arch_ref as R

pytestmark = pytest.mark.gpu

# (hidden, activation, M, B, normalize): the smallest shapes at which each mechanism can break
CASES = {
    "64x64_tanh_b1": ((64, 64), "tanh", 500, 1, True),          # normalisation skipped; fewer neuron blocks than waves
    "64x64_tanh_b33": ((64, 64), "tanh", 3000, 33, True),       # one 32-row round plus one row
    "64x64_tanh_b65": ((64, 64), "tanh", 3000, 65, True),       # one 64-row chunk plus one row
    "96x64_relu_b37": ((96, 64), "relu", 3000, 37, False),      # no normalisation; an odd count of H1 blocks
    "128x128_relu_b200": ((128, 128), "relu", 3000, 200, True),  # FusedLearner's net, on the general kernels
    "256x256_tanh_b4113": ((256, 256), "tanh", 6400, 4096 + 17, True),  # several rounds per block, several splits
    "256x256_relu_b4113": ((256, 256), "relu", 6400, 4096 + 17, True),
    "512x256_tanh_b128": ((512, 256), "tanh", 3000, 128, True),  # the LDS edge, at the reference's batch size
    "512x256_relu_b128": ((512, 256), "relu", 3000, 128, True),
    # the large end: 256 rounds per forward block, the split-K cap, images of 2^26 floats per net
    "64x64_tanh_b1048576": ((64, 64), "tanh", (1 << 20) + 100, 1 << 20, True),
}


def _cfg(norm):
    from uav_reinforcement_learning_control_amd.ppo.ppo import PPOConfig
    return PPOConfig(normalize_advantage=norm)


def _run(pol, bufs, idx, norm, adv_sums=None, learner=None):
    """One FusedArchLearner.grads into garbage-filled .grad tensors: the 13 gradients and the stats."""
    from uav_reinforcement_learning_control_amd.ppo.learner import FusedArchLearner, _ordered
    cfg = _cfg(norm)
    fl = learner or FusedArchLearner(pol, cfg.clip_range, cfg.ent_coef, cfg.vf_coef, norm)
    for p in pol.parameters():  # the kernel must overwrite, not accumulate
        p.grad = torch.full_like(p, 7.0)
    stats = torch.full((4,), -3.0, device="cuda")
    fl.grads(*bufs, idx, stats, adv_sums=adv_sums)
    torch.cuda.synchronize()
    return [p.grad.clone() for p in _ordered(pol)], stats.clone()


@functools.lru_cache(maxsize=None)
def built(name):
    """A case's inputs, the kernel's result and the two autograd references, computed once and left unchanged."""
    hidden, act, M, B, norm = CASES[name]
    seed = zlib.crc32(name.encode()) % 1000  # a case's inputs do not depend on the other cases
    cfg = _cfg(norm)
    pol = R.make_policy(seed, hidden, act, "cuda")
    bufs = R.make_buffers(pol, M, seed, cfg.clip_range)
    idx, dropped = R.make_index(pol, bufs[0], M, B if B > 1 else M, seed + 9)
    if B == 1:  # a row whose ratio is inside the clip range: a clipped row has no policy gradient to check
        with torch.no_grad():
            lp = pol.log_prob(pol.forward_heads(bufs[0][idx])[0], bufs[1][idx]).double()
            inside = ((lp - bufs[2][idx].double()).exp() - 1).abs() < cfg.clip_range - 1e-3
        idx = idx[inside][:1].contiguous()
        assert idx.numel() == 1
    got, stats = _run(pol, bufs, idx, norm)
    ref64, st64 = R.torch_grads(pol, torch.float64, *bufs, idx, cfg)
    ref32, _ = R.torch_grads(pol, torch.float32, *bufs, idx, cfg)
    return dict(pol=pol, bufs=bufs, idx=idx, norm=norm, dropped=dropped, got=got, stats=stats, ref64=ref64,
                st64=st64, ref32=ref32)


def _check_bar(label, got, ref64, ref32):
    bad, ratios = [], []
    for n, g, r64, r32 in zip(R.NAMES, got, ref64, ref32):
        scale = r64.abs().max().item()
        err = (g.double() - r64).abs().max().item()
        err32 = (r32 - r64).abs().max().item()
        ratios.append(f"{n} {err / err32:.2f}" if err32 > 0 else f"{n} err {err:.1e}/0")
        tol = 1e-4 * scale + 4 * err32 + 1e-9
        if not (err <= tol and err <= 4 * err32 + 1e-6 * scale + 1e-9):
            bad.append(f"{n}: max err {err:.3e} (scale {scale:.3e}, torch fp32 err {err32:.3e})")
    print(f"\n[{label}] err / err_torch32: " + "; ".join(ratios))
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("name", sorted(CASES))
def test_arch_grad_matches_autograd(name):
    b = built(name)
    assert b["dropped"] <= 0.2, f"the ReLU filter dropped {b['dropped']:.1%} of the candidate rows"
    _check_bar(name, b["got"], b["ref64"], b["ref32"])
    np.testing.assert_allclose(b["stats"].double().cpu().numpy(), b["st64"].cpu().numpy(), rtol=1e-4, atol=1e-7)


def test_specialised_learner_meets_the_same_bar_on_the_same_inputs():
    """The 128-128 ReLU net is a member of the family: quad_ppo_grad's kernels (which fused_learner_for keeps for it)
    and the general kernels are both inside the bar on one set of inputs."""
    from uav_reinforcement_learning_control_amd.ppo.learner import FusedLearner, fused_learner_for
    b = built("128x128_relu_b200")
    cfg = _cfg(True)
    fl = fused_learner_for(b["pol"], cfg.clip_range, cfg.ent_coef, cfg.vf_coef, True)
    assert type(fl) is FusedLearner
    got, stats = _run(b["pol"], b["bufs"], b["idx"], True, learner=fl)
    _check_bar("128x128_relu_b200 FusedLearner", got, b["ref64"], b["ref32"])
    np.testing.assert_allclose(stats.double().cpu().numpy(), b["st64"].cpu().numpy(), rtol=1e-4, atol=1e-7)


@pytest.mark.parametrize("name", ["64x64_tanh_b65", "256x256_relu_b4113"])
def test_given_advantage_sums_give_the_pre_pass_bits(name):
    from uav_reinforcement_learning_control_amd.ppo.learner import FusedArchLearner
    b = built(name)
    cfg = _cfg(True)
    fl = FusedArchLearner(b["pol"], cfg.clip_range, cfg.ent_coef, cfg.vf_coef, True)
    B = b["idx"].numel()
    perm = torch.cat([b["idx"], b["idx"].flip(0)]).contiguous()  # two minibatches; the first is the case's
    rows = fl.adv_stats_epoch(b["bufs"][3], perm, B, 2)
    got, stats = _run(b["pol"], b["bufs"], b["idx"], True, adv_sums=rows[0], learner=fl)
    assert all(torch.equal(a, c) for a, c in zip(got, b["got"])) and torch.equal(stats, b["stats"])
    with pytest.raises(NotImplementedError):
        fl.adv_stats(b["bufs"][3], b["idx"])
    with pytest.raises(NotImplementedError):
        fl.grads(*b["bufs"], b["idx"], adv_ready=True)


@pytest.mark.parametrize("name", ["64x64_tanh_b33", "96x64_relu_b37", "256x256_tanh_b4113", "512x256_relu_b128"])
def test_bits_repeat_and_do_not_depend_on_where_the_rows_lie(name):
    b = built(name)
    again, stats = _run(b["pol"], b["bufs"], b["idx"], b["norm"])
    assert all(torch.equal(a, c) for a, c in zip(again, b["got"])) and torch.equal(stats, b["stats"])
    moved = tuple(t[b["idx"]].contiguous() for t in b["bufs"])  # the rows physically in index order
    ar = torch.arange(b["idx"].numel(), device="cuda")
    got, stats = _run(b["pol"], moved, ar, b["norm"])
    assert all(torch.equal(a, c) for a, c in zip(got, b["got"])) and torch.equal(stats, b["stats"])


def test_bad_arguments_are_refused_before_anything_is_written():
    from uav_reinforcement_learning_control_amd import _native as N
    from uav_reinforcement_learning_control_amd.ppo.learner import _ordered
    b = built("64x64_tanh_b33")
    pol, (obs, act, logp, adv, ret), idx = b["pol"], b["bufs"], b["idx"]
    cfg = _cfg(True)
    L = N.lib()
    B = idx.numel()
    arch = N.QuadActorArch(h1=64, h2=64, activation=N.ACTFN_TANH)
    nbytes = L.quad_ppo_arch_workspace_bytes(C.byref(arch), B)
    assert nbytes > 0
    ws = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device="cuda")
    for p in pol.parameters():
        p.grad = torch.full_like(p, 7.0)
    stats = torch.full((4,), -3.0, device="cuda")
    ps = _ordered(pol)
    prm = lambda: N.QuadPolicyParams(*[p.data_ptr() for p in ps])
    grd = lambda: N.QuadPolicyGrads(*[p.grad.data_ptr() for p in ps])
    batch = lambda **kw: N.QuadPPOBatch(**{**dict(obs=obs.data_ptr(), actions=act.data_ptr(), log_prob=logp.data_ptr(),
                                                advantages=adv.data_ptr(), returns=ret.data_ptr(),
                                                index=idx.data_ptr(), batch=B, normalize_advantage=1,
                                                clip_range=cfg.clip_range, ent_coef=cfg.ent_coef, vf_coef=cfg.vf_coef,
                                                stats=stats.data_ptr(), adv_sums=None), **kw})
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(arch_=arch, p=None, bt=None, g=None, wptr=None, wbytes=nbytes):
        p, bt, g = p or prm(), bt or batch(), g or grd()
        return L.quad_ppo_arch_grad(C.byref(arch_) if arch_ is not None else None, C.byref(p), C.byref(bt), C.byref(g),
                                    ws.data_ptr() if wptr is None else wptr, wbytes, stream)

    def with_field(make, name, value):
        s = make()
        setattr(s, name, value)
        return s

    bad = {f"arch {h}": dict(arch_=N.QuadActorArch(h1=h[0], h2=h[1], activation=0))
           for h in ((128, 32), (100, 64), (544, 64))}
    bad["activation 2"] = dict(arch_=N.QuadActorArch(h1=64, h2=64, activation=2))
    bad["arch NULL"] = dict(arch_=None)
    bad["param NULL"] = dict(p=with_field(prm, "vf_w1", None))
    bad["param misaligned"] = dict(p=with_field(prm, "pi_b0", ps[1].data_ptr() + 2))
    bad["grad NULL"] = dict(g=with_field(grd, "log_std", None))
    bad["grad misaligned"] = dict(g=with_field(grd, "act_w", ps[4].grad.data_ptr() + 1))
    bad["obs NULL"] = dict(bt=batch(obs=None))
    bad["obs misaligned"] = dict(bt=batch(obs=obs.data_ptr() + 4))
    bad["actions misaligned"] = dict(bt=batch(actions=act.data_ptr() + 8))
    bad["index misaligned"] = dict(bt=batch(index=idx.data_ptr() + 4))
    bad["index NULL"] = dict(bt=batch(index=None))
    bad["stats misaligned"] = dict(bt=batch(stats=stats.data_ptr() + 2))
    bad["workspace misaligned"] = dict(wptr=ws.data_ptr() + 8, wbytes=nbytes - 8)
    bad["workspace NULL"] = dict(wptr=0)
    bad["batch 0"] = dict(bt=batch(batch=0))
    bad["workspace one byte short"] = dict(wbytes=nbytes - 1)
    bad["clip_range 0"] = dict(bt=batch(clip_range=0.0))
    bad["QUAD_ADV_PRECOMPUTED"] = dict(bt=batch(normalize_advantage=N.QUAD_ADV_PRECOMPUTED))
    bad["QUAD_ADV_GIVEN without sums"] = dict(bt=batch(normalize_advantage=N.QUAD_ADV_GIVEN))
    for what, kw in bad.items():
        assert call(**kw) == N.QUAD_EINVAL, what
    torch.cuda.synchronize()
    assert bool((ws == 0x5A).all()) and bool((stats == -3.0).all())
    assert all(bool((p.grad == 7.0).all()) for p in ps)
    # the unchanged descriptors then launch, and give the bits FusedArchLearner gave
    assert call() == N.QUAD_OK
    torch.cuda.synchronize()
    assert all(torch.equal(p.grad, g) for p, g in zip(ps, b["got"])) and torch.equal(stats, b["stats"])


def test_fused_adam_steps_a_wide_tanh_net_as_torch_does():
    from uav_reinforcement_learning_control_amd.ppo.learner import FusedAdam, FusedArchLearner
    b = built("256x256_tanh_b4113")
    cfg = _cfg(True)
    pol = copy.deepcopy(b["pol"])
    twin = copy.deepcopy(pol)
    opt = torch.optim.Adam(pol.parameters(), lr=cfg.learning_rate, eps=cfg.adam_eps)
    topt = torch.optim.Adam(twin.parameters(), lr=cfg.learning_rate, eps=cfg.adam_eps)
    fl = FusedArchLearner(pol, cfg.clip_range, cfg.ent_coef, cfg.vf_coef, True)
    fa = FusedAdam(opt, cfg.max_grad_norm)
    assert len(fa.params) == 13
    for _ in range(2):
        fl.grads(*b["bufs"], b["idx"])
        for p, q in zip(pol.parameters(), twin.parameters()):
            q.grad = p.grad.clone()
        fa.step()
        torch.nn.utils.clip_grad_norm_(twin.parameters(), cfg.max_grad_norm)
        topt.step()
    torch.cuda.synchronize()
    sa, sb = opt.state_dict()["state"], topt.state_dict()["state"]
    # tests/test_gpu_brax_learner.py's tolerances: after two steps a moment is a sum of three f32-rounded terms
    for i, (p, q) in enumerate(zip(pol.parameters(), twin.parameters())):
        gm = float(q.grad.abs().max())
        torch.testing.assert_close(p, q, rtol=1e-5, atol=1e-9)
        torch.testing.assert_close(sa[i]["exp_avg"], sb[i]["exp_avg"], rtol=1e-5, atol=1e-7 * gm)
        torch.testing.assert_close(sa[i]["exp_avg_sq"], sb[i]["exp_avg_sq"], rtol=1e-5, atol=1e-9 * gm * gm)
        assert float(sa[i]["step"]) == 2.0
    sd = copy.deepcopy(opt.state_dict())
    fresh = torch.optim.Adam(pol.parameters(), lr=1.0, eps=1e-8)
    fresh.load_state_dict(sd)
    assert fresh.param_groups[0]["lr"] == cfg.learning_rate
    for i in range(13):
        assert torch.equal(fresh.state_dict()["state"][i]["exp_avg"], sa[i]["exp_avg"])


def test_ppo_train_fused_arch_matches_torch_update():
    """tests/test_gpu_learner.py test_ppo_train_fused_matches_torch_update's form and bounds for a (64, 64) tanh net
    with and without PPOConfig.fused_update_arch."""
    from uav_reinforcement_learning_control_amd.envs import QuadVecEnv
    from uav_reinforcement_learning_control_amd.ppo.learner import FusedArchLearner
    from uav_reinforcement_learning_control_amd.ppo.ppo import PPO, PPOConfig
    outs = []
    for fused in (True, False):
        env = QuadVecEnv(1024, env="hover", device="cuda:0", seed=3)
        cfg = PPOConfig(n_steps=16, n_minibatches=2, n_epochs=1, net_arch=(64, 64), activation="tanh",
                        fused_update_arch=fused)
        algo = PPO(env, cfg, seed=11)
        assert isinstance(algo._learner, FusedArchLearner) if fused else algo._learner is None
        assert algo._fp is None and not algo._one_launch and (algo._adam is not None) == fused
        algo.collect_rollouts()
        torch.manual_seed(5)  # same epoch permutation
        st = algo.train()
        outs.append(([p.detach().clone() for p in algo.policy.parameters()], st))
        env.close()
    (pa, sa), (pb, sb) = outs
    assert sa["n"] == sb["n"] == 2
    lr = PPOConfig().learning_rate
    d = torch.cat([(a - b).abs().reshape(-1) for a, b in zip(pa, pb)])
    assert d.max().item() <= 2 * lr * 2 + 1e-6
    assert (d > 1e-6).float().mean().item() < 0.01, f"{(d > 1e-6).sum().item()} of {d.numel()} differ"
    for k in ("pg_loss", "vf_loss", "entropy", "clip_fraction"):
        assert math.isclose(sa[k], sb[k], rel_tol=1e-3, abs_tol=1e-6), (k, sa[k], sb[k])


def test_captured_epoch_and_eager_update_give_the_same_bits():
    """3 epochs of n_steps = 256, batch_size = 128 on one rollout: graph_update on (the captured epoch) and off."""
    from uav_reinforcement_learning_control_amd.envs import QuadVecEnv
    from uav_reinforcement_learning_control_amd.ppo.ppo import PPO, PPOConfig
    outs, first = [], None
    for graph in (True, False):
        env = QuadVecEnv(16, env="hover", device="cuda:0", seed=3)
        cfg = PPOConfig(n_steps=256, batch_size=128, n_epochs=3, net_arch=(64, 64), activation="tanh",
                        fused_update_arch=True, graph_update=graph)
        algo = PPO(env, cfg, seed=11)
        algo.collect_rollouts()
        bufs = (algo.buf_obs, algo.buf_act, algo.buf_logp, algo.buf_adv, algo.buf_ret)
        if first is None:
            first = [t.clone() for t in bufs]
        else:  # the same rollout for both
            for t, s in zip(bufs, first):
                t.copy_(s)
        torch.manual_seed(5)
        st = algo.train()
        assert st["n"] == 3 * 32
        assert (algo._epoch_graph is not None) == graph
        outs.append([p.detach().clone() for p in algo.policy.parameters()])
        env.close()
    assert all(torch.equal(a, b) for a, b in zip(*outs))


def test_driver_learns_with_the_flag_and_its_policy_flies(tmp_path, capsys):
    from uav_reinforcement_learning_control_amd import train
    from uav_reinforcement_learning_control_amd.export import load_sb3_policy
    from uav_reinforcement_learning_control_amd.ppo.fused import FusedActor, fused_actor_for
    train.main(["--num-envs", "1024", "--total-timesteps", str(12 * 1024 * 64), "--n-steps", "64", "--n-epochs", "4",
                "--n-minibatches", "8", "--learning-rate", "3e-4", "--net-arch", "64", "64", "--activation", "tanh",
                "--fused-arch-update", "--eval-freq", "0", "--checkpoint-freq", "0",
                "--log-dir", str(tmp_path / "logs"), "--model-dir", str(tmp_path / "models")])
    out = capsys.readouterr().out
    assert "update: fused minibatch gradient for net (64, 64) tanh (FusedArchLearner: quad_ppo_arch_grad" in out
    (run,) = os.listdir(tmp_path / "models")
    cfg = json.load(open(tmp_path / "models" / run / "config.json"))
    assert cfg["fused_arch_update"] is True and cfg["ppo"]["net_arch"] == [64, 64]
    (log,) = os.listdir(tmp_path / "logs")
    rows = np.genfromtxt(tmp_path / "logs" / log / "progress.csv", delimiter=",", names=True)
    ret = rows["mean_return"]
    print("mean returns", [round(float(x), 2) for x in ret])
    assert len(ret) == 12 and np.all(np.isfinite(ret))
    assert np.mean(ret[-3:]) > np.mean(ret[:3])
    pol = load_sb3_policy(str(tmp_path / "models" / run / "hover_policy_final.zip"), activations=("relu", "tanh")).cuda()
    fa = fused_actor_for(pol)
    assert type(fa) is FusedActor
    fa.pack()
    obs = torch.rand(100, 12, device="cuda") * 2 - 1
    a_env = torch.empty(100, 4, device="cuda")
    fa.act(obs, a_env)
    with torch.no_grad():
        want = pol.forward_heads(obs)[0].clamp(-1, 1)
    torch.testing.assert_close(a_env, want, rtol=2e-5, atol=2e-5)
