"""ppo.ArchPopulationPPO against stand-alone PPO runs with both arch flags: member m must be BIT-IDENTICAL to
PPO(env, cfg, seed) -- parameters, Adam moments and step counters, every rollout buffer, num_timesteps and the rollout
statistics (raw-byte comparisons, no tolerance) --, and population_for / optimize --search-arch route every arch of the
reference's search space to its class."""
import dataclasses
import os

import numpy as np
import pytest
import torch

from test_gpu_population_ppo import N_ENVS, WRAPPER, _same, _state, _stats_key

pytestmark = pytest.mark.gpu

SEEDS = (3, 11, 42)


def _configs(net_arch=(64, 64), activation="tanh", n_steps=32, batch=64):
    from uav_reinforcement_learning_control_amd.ppo import PPOConfig
    base = PPOConfig(n_steps=n_steps, batch_size=batch, net_arch=net_arch, activation=activation,
                     fused_rollout_arch=True, fused_update_arch=True)
    return [dataclasses.replace(base, n_epochs=2, learning_rate=3e-4, gamma=0.99, gae_lambda=0.95, clip_range=0.2,
                                ent_coef=1e-4, vf_coef=0.5, max_grad_norm=0.5),
            dataclasses.replace(base, n_epochs=3, learning_rate=1e-3, gamma=0.97, gae_lambda=0.9, clip_range=0.1,
                                ent_coef=1e-3, vf_coef=0.7, max_grad_norm=0.3),
            dataclasses.replace(base, n_epochs=2, learning_rate=1e-4, gamma=0.95, gae_lambda=0.8, clip_range=0.3,
                                ent_coef=0.0, vf_coef=0.3, max_grad_norm=5.0)]


def _standalone(cfg, seed, iters):
    """The stand-alone run: per iteration (state bytes, rollout statistics, num_timesteps)."""
    from uav_reinforcement_learning_control_amd.envs import QuadVecEnv
    from uav_reinforcement_learning_control_amd.ppo import PPO
    from uav_reinforcement_learning_control_amd.ppo.fused import FusedActorCritic
    from uav_reinforcement_learning_control_amd.ppo.learner import FusedArchLearner
    env = QuadVecEnv(N_ENVS, env="hover", wrapper=WRAPPER, device="cuda:0", seed=seed)
    model = PPO(env, cfg, seed=seed)
    assert type(model._fp) is FusedActorCritic and type(model._learner) is FusedArchLearner and model._one_launch
    out = []
    for _ in range(iters):
        rs = model.collect_rollouts()
        model.train()
        out.append((_state(model), _stats_key(rs), model.num_timesteps))
    return out


@pytest.fixture(scope="module")
def reference():
    """Three stand-alone (64, 64) tanh runs of two iterations, one after another, computed once and left unchanged."""
    return [_standalone(c, s, 2) for c, s in zip(_configs(), SEEDS)]


def _population(**kw):
    from uav_reinforcement_learning_control_amd.ppo import ArchPopulationPPO
    return ArchPopulationPPO(list(zip(_configs(**kw), SEEDS)), n_envs=N_ENVS, env="hover", wrapper=WRAPPER,
                             device="cuda:0")


def test_members_equal_standalone_ppo(reference):
    pop = _population()
    assert pop.nmb == 4 and pop.batch == 64
    for it in range(2):
        rs = pop.collect_rollouts()
        ts = pop.train()
        for m in range(3):
            want, stats, steps = reference[m][it]
            _same(_state(pop.member(m)), want, f"iteration {it} member {m}")
            assert _stats_key(rs[m]) == stats and pop.member(m).num_timesteps == steps == (it + 1) * 32 * N_ENVS
            assert ts[m]["n"] == pop.member(m).cfg.n_epochs * 4  # the two-epoch members left the subset early
    a, b = _state(pop.member(0)), _state(pop.member(1))
    assert not np.array_equal(a["p0"], b["p0"]) and not np.array_equal(a["buf_rew"], b["buf_rew"])
    pop.close()


def test_widest_members_equal_standalone_ppo():
    """(512, 256) relu, one iteration: the widest LDS of every kernel."""
    kw = dict(net_arch=(512, 256), activation="relu")
    pop = _population(**kw)
    rs = pop.collect_rollouts()
    pop.train()
    got = [(_state(pop.member(m)), _stats_key(rs[m])) for m in range(3)]
    pop.close()
    for m, (cfg, seed) in enumerate(zip(_configs(**kw), SEEDS)):
        (want, stats, steps), = _standalone(cfg, seed, 1)
        _same(got[m][0], want, f"member {m}")
        assert got[m][1] == stats and steps == 32 * N_ENVS


def test_deactivate_freezes_a_member(reference):
    pop = _population()
    pop.collect_rollouts()
    pop.train()
    frozen = _state(pop.member(1))
    steps = pop.member(1).num_timesteps
    pop.deactivate(1)
    rs = pop.collect_rollouts()
    ts = pop.train()
    assert rs[1] is None and ts[1] is None
    _same(_state(pop.member(1)), frozen, "deactivated member 1")
    assert pop.member(1).num_timesteps == steps
    for m in (0, 2):
        _same(_state(pop.member(m)), reference[m][1][0], f"iteration 1 member {m}")
    pop.close()


def test_evaluate_equals_evaluate_episodes():
    from uav_reinforcement_learning_control_amd.evaluate import evaluate_episodes
    pop = _population()
    pop.collect_rollouts()
    pop.train()
    seeds = [1_000_003 * (s + 1) + 4 for s in SEEDS]
    got = pop.evaluate(num_episodes=4, seeds=seeds)
    for m in range(3):
        ref = evaluate_episodes(pop.member(m).policy, num_episodes=4, wrapper=WRAPPER, device="cuda:0", seed=seeds[m])
        for k in ("rewards", "lengths", "terminated"):
            assert np.array_equal(np.asarray(got[m][k]), np.asarray(ref[k])), (m, k)
        assert got[m]["mean_reward"] == ref["mean_reward"] and got[m]["mean_length"] == ref["mean_length"]
    assert got[0]["mean_reward"] != got[1]["mean_reward"]
    pop.close()


def test_population_for_routes_by_arch():
    from uav_reinforcement_learning_control_amd.ppo import ArchPopulationPPO, PopulationPPO, PPOConfig, population_for
    kw = dict(n_envs=N_ENVS, env="hover", wrapper=WRAPPER, device="cuda:0")
    base = PPOConfig(n_steps=32, batch_size=64)
    pop = population_for([(base, 1), (dataclasses.replace(base, n_epochs=3), 2)], **kw)
    assert type(pop) is PopulationPPO
    pop.close()
    tanh = dataclasses.replace(base, activation="tanh")
    pop = population_for([(tanh, 1), (tanh, 2)], **kw)
    assert type(pop) is ArchPopulationPPO and all(m.cfg.fused_rollout_arch and m.cfg.fused_update_arch for m in pop.members)
    pop.close()
    with pytest.raises(ValueError):
        population_for([(dataclasses.replace(base, net_arch=(100, 64)), 1)], **kw)   # H1 no multiple of 32
    with pytest.raises(ValueError):
        population_for([(dataclasses.replace(base, net_arch=(64, 64, 64)), 1)], **kw)
    with pytest.raises(ValueError, match="share net_arch and activation"):
        population_for([(tanh, 1), (dataclasses.replace(tanh, net_arch=(256, 256)), 2)], **kw)
    on = dataclasses.replace(tanh, fused_rollout_arch=True, fused_update_arch=True)
    with pytest.raises(ValueError, match="share net_arch and activation"):
        ArchPopulationPPO([(on, 1), (dataclasses.replace(on, net_arch=(256, 256)), 2)], **kw)
    with pytest.raises(ValueError, match="PopulationPPO"):
        ArchPopulationPPO([(dataclasses.replace(base, fused_rollout_arch=True, fused_update_arch=True), 1)], **kw)
    with pytest.raises(ValueError, match="fused_rollout_arch"):
        ArchPopulationPPO([(tanh, 1)], **kw)


def test_optimize_search_arch_end_to_end(tmp_path, capsys):
    """optimize --search-arch at a toy budget: seed 2 samples all six arch combinations in six trials (one of them
    (small, relu), which trains on PopulationPPO); the CSV has the golden header and six rows whose arch columns are
    the trials'; the --save-best archive loads with the best trial's arch."""
    import json
    from uav_reinforcement_learning_control_amd import export, optimize as O
    best = tmp_path / "best"
    rc = O.main(["--search-arch", "--n-trials", "6", "--n-timesteps", "2048", "--n-envs", "8", "--seed", "2",
                 "--study-name", "toy", "--out-dir", str(tmp_path), "--save-best", str(best)], n_steps_choices=(256,))
    assert rc == 0
    out = capsys.readouterr().out
    assert "Populations: 6 (largest 1, median 1 trials)" in out and "Best trial" in out
    path = tmp_path / "study_results_toy.csv"
    header = open(os.path.join(os.path.dirname(__file__), "golden", "study_results_header.txt")).read().split()
    assert open(path).readline().strip().split(",") == header
    rows = O.read_csv(str(path))
    trials = O.make_trials(6, 2, 8, (256,), search_arch=True)
    assert len({(t.params["net_arch"], t.params["activation_fn"]) for t in trials}) >= 3
    assert [r["number"] for r in rows] == list(range(6))
    for r, t in zip(rows, trials):
        assert (r["params_net_arch"], r["params_activation_fn"], r["user_attrs_net_arch_name"]) == \
            (t.params["net_arch"], t.params["activation_fn"], t.params["net_arch"])
        assert r["state"] in ("COMPLETE", "PRUNED")
    done = [r for r in rows if r["state"] == "COMPLETE"]
    assert done and all(np.isfinite(r["value"]) for r in done)
    top = max(done, key=lambda r: r["value"])
    arch = O.NET_ARCH[top["params_net_arch"]]
    assert f'"net_arch": {arch},' in out and f'nn.{O.ACTIVATION_CLASS[top["params_activation_fn"]]},' in out
    cfg = json.load(open(best / "config.json"))
    assert cfg["trial"] == top["number"] and cfg["ppo"]["net_arch"] == arch
    assert cfg["ppo"]["activation_fn"] == O.ACTIVATION_CLASS[top["params_activation_fn"]]
    pol = export.load_sb3_policy(str(best / "hover_policy_final.zip"), activations=("relu", "tanh"))
    assert tuple(pol.mlp_extractor.policy_net[0].weight.shape) == (arch[0], 12)
    assert tuple(pol.mlp_extractor.policy_net[2].weight.shape) == (arch[1], arch[0])
    assert pol.activation == top["params_activation_fn"]
    assert all(torch.isfinite(p).all() for p in pol.parameters())
