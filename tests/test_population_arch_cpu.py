"""CPU checks of optimize --search-arch and of the general family's population ABI: without the flag the
driver samples, groups and prints exactly what it did; with it the reference's net_arch x activation_fn space is drawn
after ent_coef, groups never mix arches, and every text output carries the arch. The gradient table entry of the
family's populations (csrc/learner_arch.h lrna::Args) is pinned through a host program, in the style of
tests/native_population/."""
import ctypes as C
import json
import os
import random
import subprocess

import pytest

from uav_reinforcement_learning_control_amd import _native as N
from uav_reinforcement_learning_control_amd import optimize as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUT = os.path.join(REPO, "tests", "native_population_arch", "_build", "args_layout")
EARLIER = ("learning_rate", "n_steps", "batch_size", "n_epochs", "gamma_inv", "gae_lambda", "clip_range", "ent_coef")
COMBOS = {(a, f) for a in ("small", "medium", "large") for f in ("tanh", "relu")}


def test_flag_off_draws_todays_trials():
    for seed in (0, 7):
        a = O.make_trials(40, seed, 8)
        b = O.make_trials(40, seed, 8, search_arch=False)
        assert [(t.number, t.params, t.seed, t.batch) for t in a] == [(t.number, t.params, t.seed, t.batch) for t in b]
        assert all(t.params["net_arch"] == "small" and t.params["activation_fn"] == "relu" for t in a)
        # the sampler consumes exactly the eight draws it did: the rng ends where eight manual draws leave it
        rng, ref = random.Random(seed), random.Random(seed)
        p = O.sample_ppo_params(rng)
        q = {"learning_rate": O._log_uniform(ref, 1e-5, 1e-3), "n_steps": ref.choice(list(O.N_STEPS_CHOICES)),
             "batch_size": ref.choice(O.BATCH_CHOICES), "n_epochs": ref.choice(O.N_EPOCHS_CHOICES),
             "gamma_inv": O._log_uniform(ref, 0.001, 0.05), "gae_lambda": ref.uniform(0.9, 0.99),
             "clip_range": ref.uniform(0.1, 0.3), "ent_coef": O._log_uniform(ref, 1e-5, 0.1)}
        assert {k: p[k] for k in EARLIER} == q and rng.getstate() == ref.getstate()
    assert list(p) == list(EARLIER) + ["net_arch", "activation_fn"]
    a = O.build_parser().parse_args([])
    assert a.search_arch is False
    assert O.NET_ARCH == {"small": [128, 128], "medium": [256, 256], "large": [512, 256]}


def test_flag_on_draws_the_arch_after_ent_coef():
    rng, seen = random.Random(3), set()
    for _ in range(600):
        state = rng.getstate()
        p = O.sample_ppo_params(rng, search_arch=True)
        off = random.Random()
        off.setstate(state)
        q = O.sample_ppo_params(off)
        assert {k: p[k] for k in EARLIER} == {k: q[k] for k in EARLIER}
        # then net_arch, then activation_fn (the reference's order of suggestions)
        assert p["net_arch"] == off.choice(("small", "medium", "large"))
        assert p["activation_fn"] == off.choice(("tanh", "relu"))
        assert off.getstate() == rng.getstate()
        seen.add((p["net_arch"], p["activation_fn"]))
    assert seen == COMBOS
    trials = O.make_trials(600, 3, 8, search_arch=True)
    assert {(t.params["net_arch"], t.params["activation_fn"]) for t in trials} == COMBOS


def test_groups_never_mix_arches():
    trials = O.make_trials(300, 1, 8, search_arch=True)
    groups = O.group_trials(trials, 16)
    assert sorted(t.number for g in groups for t in g) == list(range(300))
    for g in groups:
        assert len(g) <= 16
        assert len({(t.params["n_steps"], t.batch, t.params["net_arch"], t.params["activation_fn"]) for t in g}) == 1
    assert len({(g[0].params["net_arch"], g[0].params["activation_fn"]) for g in groups}) == 6
    # without the flag the key's arch part is constant: the groups are the (n_steps, batch) groups they were
    plain = O.make_trials(60, 1, 8)
    by = {}
    for t in plain:
        by.setdefault((t.params["n_steps"], t.batch), []).append(t.number)
    assert sorted(map(tuple, by.values())) == sorted(tuple(t.number for t in g) for g in O.group_trials(plain, 1000))
    text = O.population_sizes(groups)
    assert f"Populations: {len(groups)}" in text and f"largest {max(map(len, groups))}" in text and "median" in text


class _Member:
    obs_dim = 12
    num_timesteps = 4096
    policy = opt = cfg = None


class _Pop:
    def member(self, m):
        return _Member()


def test_text_outputs_carry_the_arch(tmp_path, monkeypatch):
    t = next(t for t in O.make_trials(200, 5, 8, search_arch=True)
             if (t.params["net_arch"], t.params["activation_fn"]) == ("large", "tanh"))
    t.state, t.value = O.COMPLETE, -12.5
    row = O.trial_row(t)
    assert (row["params_net_arch"], row["params_activation_fn"], row["user_attrs_net_arch_name"]) == \
        ("large", "tanh", "large")
    assert set(row) == set(O.CSV_COLUMNS)
    best = O.format_best(t)
    assert '"net_arch": [512, 256],' in best and '"activation_fn": nn.Tanh,' in best and "net_arch_name: large" in best
    u = O.make_trials(1, 5, 8)[0]
    u.value = 1.0
    assert '"net_arch": [128, 128],' in O.format_best(u) and '"activation_fn": nn.ReLU,' in O.format_best(u)
    cfg = O.ppo_config(t)
    assert tuple(cfg.net_arch) == (512, 256) and cfg.activation == "tanh"
    assert tuple(O.ppo_config(u).net_arch) == (128, 128) and O.ppo_config(u).activation == "relu"
    # save_best's config.json (the archive itself is written from a trained member: tests/test_gpu_population_arch_ppo.py)
    import uav_reinforcement_learning_control_amd.export as E
    monkeypatch.setattr(E, "save_sb3_zip", lambda path, *a, **k: path + ".zip")
    O.save_best(_Pop(), 0, t, str(tmp_path), 8, 4096)
    with open(tmp_path / "config.json") as f:
        saved = json.load(f)
    assert saved["ppo"]["net_arch"] == [512, 256] and saved["ppo"]["activation_fn"] == "Tanh"
    assert "search-arch" in O.build_parser().format_help() and "only architecture" not in O.build_parser().format_help()


def test_population_class_is_picked_by_the_arch_before_any_gpu_work():
    from uav_reinforcement_learning_control_amd.ppo import PPOConfig
    from uav_reinforcement_learning_control_amd.ppo.population import population_for
    mixed = [(PPOConfig(net_arch=(256, 256), activation="tanh"), 0), (PPOConfig(net_arch=(256, 256), activation="relu"), 1)]
    with pytest.raises(ValueError, match="share net_arch and activation"):
        population_for(mixed)
    with pytest.raises(ValueError):
        population_for([])


def test_abi_exports_and_rejections_without_a_device():
    L = N.lib()
    for name in N.POP_ARCH_EXPORTS:
        assert name in N.EXPORTS and hasattr(L, name), name
    assert N.ABI_VERSION == 8
    arch = N.QuadActorArch(h1=64, h2=64, activation=N.ACTFN_TANH)
    h = C.c_void_p(1)
    assert L.quad_pop_create_arch(C.byref(arch), None, 1, 32, 1, C.byref(h)) == N.QUAD_EINVAL and not h.value
    assert b"quad_pop_create_arch" in L.quad_last_error()
    bad = N.QuadActorArch(h1=100, h2=64, activation=N.ACTFN_TANH)
    h = C.c_void_p(1)
    assert L.quad_pop_create_arch(C.byref(bad), None, 1, 32, 1, C.byref(h)) == N.QUAD_EINVAL and not h.value
    assert b"family" in L.quad_last_error()
    ad = N.QuadAdam()
    assert L.quad_pop_arch_workspace_bytes(C.byref(bad), C.byref(ad), 32) == 0
    assert L.quad_pop_arch_workspace_bytes(C.byref(arch), C.byref(ad), 32) == 0  # count = 0: an invalid QuadAdam


def test_gradient_table_entry_layout():
    """lrna::Args as the host compiles it: the population launch reads it from a device table, so its size and the
    offsets of the fields the launch advances (g.idx, g.adv_part, stats) are pinned like an ABI struct's."""
    subprocess.run(["make", "-s", "-C", os.path.dirname(os.path.dirname(LAYOUT))], check=True)
    out = subprocess.run([LAYOUT], capture_output=True, text=True, check=True).stdout
    got = {k: int(v) for k, v in (line.split() for line in out.splitlines())}
    assert got == {"sizeof": 416, "g": 0, "g.idx": 144, "g.adv_part": 152, "g.batch": 168, "gr": 216, "stats": 320,
                   "x": 328, "h1": 336, "dh2": 344, "dh1": 352, "sp": 360, "pb": 368, "h1w": 376, "rps": 404,
                   "ent_coef": 408}
    assert got["stats"] - got["gr"] == C.sizeof(N.QuadPolicyGrads)
