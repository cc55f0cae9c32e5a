"""Populations on the deployed observation without a GPU: quad_pop_create_deployed /
quad_pop_deployed_workspace_bytes at the C boundary and in the binding, QuadPopDeploy's layout, the refusals of
DeployedPopulationPPO / deployed_population_for before anything is built, and optimize's --deployed / --search-alpha
(the driver without them draws, groups and writes what it did)."""
import csv
import ctypes as C
import json
import os
import random
import re
import subprocess

import pytest

from uav_reinforcement_learning_control_amd import _native as N
from uav_reinforcement_learning_control_amd import optimize as O
from uav_reinforcement_learning_control_amd.ppo import PPOConfig
from uav_reinforcement_learning_control_amd.ppo import population as POP

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "quadenv.h")
LAYOUT = os.path.join(REPO, "tests", "native_population_deployed", "_build", "deploy_layout")
GOLDEN_HEADER = os.path.join(REPO, "tests", "golden", "study_results_header.txt")
EARLIER = ("learning_rate", "n_steps", "batch_size", "n_epochs", "gamma_inv", "gae_lambda", "clip_range", "ent_coef",
           "net_arch", "activation_fn")


def _header_params(ret, name):
    src = open(HEADER).read()
    m = re.search(r"\b" + ret + r"\s+" + name + r"\s*\(([^;]*?)\)\s*;", src, re.S)
    assert m, name
    return [re.sub(r"/\*.*?\*/", "", p, flags=re.S).strip() for p in m.group(1).split(",")]


# ---------------------------------------------------------------- the C boundary
def test_symbols_prototypes_and_abi_version():
    L = N.lib()
    assert L.quad_abi_version() == 8 and N.ABI_VERSION == 8
    assert N.POP_DEPLOYED_EXPORTS == ("quad_pop_deployed_workspace_bytes", "quad_pop_create_deployed")
    for name in N.POP_DEPLOYED_EXPORTS:
        assert name in N.EXPORTS and hasattr(L, name), name
    assert "QuadPopDeploy" in open(HEADER).read()
    ws, mk = L.quad_pop_deployed_workspace_bytes, L.quad_pop_create_deployed
    assert ws.restype is C.c_int64 and mk.restype is C.c_int
    assert _header_params("int64_t", "quad_pop_deployed_workspace_bytes") == \
        ["const QuadActorArch* arch", "const QuadAdam* adam", "int32_t batch"]
    assert ws.argtypes == [C.POINTER(N.QuadActorArch), C.POINTER(N.QuadAdam), C.c_int32]
    params = _header_params("int", "quad_pop_create_deployed")
    assert [p.split()[-1] for p in params] == ["arch", "members", "deploy", "P", "batch", "normalize_advantage", "out"]
    assert mk.argtypes == [C.POINTER(N.QuadActorArch), C.POINTER(N.QuadPopMember), C.POINTER(N.QuadPopDeploy),
                           C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
    assert N.need_deployed_population() is L
    nm = subprocess.run(["nm", "-D", "--defined-only", N.LIB_PATH], capture_output=True, text=True).stdout
    for name in N.POP_DEPLOYED_EXPORTS:
        assert re.search(rf"\bT {name}\b", nm), name


def test_quad_pop_deploy_layout_equals_the_headers():
    """QuadPopDeploy as the host compiles it against its ctypes twin, and the device table's entry (pop::EstEntry),
    which the rollout kernel reads field by field; pop::RollEntry has the size it had (the estimator arguments went
    into a table of their own)."""
    subprocess.run(["make", "-s", "-C", os.path.dirname(os.path.dirname(LAYOUT))], check=True)
    out = subprocess.run([LAYOUT], capture_output=True, text=True, check=True).stdout
    got = {k: int(v) for k, v in (line.split() for line in out.splitlines())}
    D, E = N.QuadPopDeploy, N.QuadVelEst
    assert got["QuadPopDeploy"] == C.sizeof(D) == 40
    assert got["QuadPopDeploy.est"] == D.est.offset == 0 and got["QuadPopDeploy.est_dt"] == D.est_dt.offset == 32
    for f in ("alpha", "alpha_all", "max_dt", "state"):
        assert got["QuadPopDeploy.est." + f] == D.est.offset + getattr(E, f).offset, f
        assert got["EstEntry.est." + f] == getattr(E, f).offset, f
    assert got["EstEntry"] == 40 and got["EstEntry.est_dt"] == 32
    assert got["RollEntry"] == 184


def test_null_and_bad_arguments_are_refused_without_a_device():
    L = N.lib()
    ok = N.QuadActorArch(h1=64, h2=64, activation=N.ACTFN_TANH)
    small = N.QuadActorArch(h1=128, h2=128, activation=N.ACTFN_RELU)
    bad = N.QuadActorArch(h1=100, h2=64, activation=N.ACTFN_TANH)
    mem, dep = (N.QuadPopMember * 1)(), (N.QuadPopDeploy * 1)()

    def refused(word, *args):
        h = C.c_void_p(1)
        assert L.quad_pop_create_deployed(*args, C.byref(h)) == N.QUAD_EINVAL and not h.value, word
        assert word.encode() in L.quad_last_error(), (word, L.quad_last_error())

    refused("family", C.byref(bad), mem, dep, 1, 32, 1)
    refused("family", None, mem, dep, 1, 32, 1)
    refused("deploy is NULL", C.byref(ok), mem, None, 1, 32, 1)
    refused("members", C.byref(ok), None, dep, 1, 32, 1)
    refused("P must be", C.byref(ok), mem, dep, 0, 32, 1)
    refused("batch", C.byref(ok), mem, dep, 1, 8193, 1)
    refused("member 0", C.byref(small), mem, dep, 1, 32, 1)  # an empty member: env / packed is NULL
    assert L.quad_pop_create_deployed(C.byref(ok), mem, dep, 1, 32, 1, None) == N.QUAD_EINVAL
    ad = N.QuadAdam()
    assert L.quad_pop_deployed_workspace_bytes(C.byref(bad), C.byref(ad), 32) == 0
    assert L.quad_pop_deployed_workspace_bytes(None, C.byref(ad), 32) == 0
    assert L.quad_pop_deployed_workspace_bytes(C.byref(ok), C.byref(ad), 32) == 0     # count = 0: an invalid QuadAdam
    assert L.quad_pop_deployed_workspace_bytes(C.byref(small), C.byref(ad), 32) == 0


# ---------------------------------------------------------------- the Python classes
def _dep(net=(64, 64), act="tanh", **kw):
    return PPOConfig(net_arch=net, activation=act, n_steps=16, n_minibatches=4, fused_rollout_arch=True,
                     fused_update_arch=True, obs_mode="deployed", **kw)


class _Built(Exception):
    """Raised by the stub env: every check that precedes the first device object has passed."""


@pytest.fixture
def stub_env(monkeypatch):
    def make(*a, **k):
        raise _Built()
    monkeypatch.setattr(POP, "QuadVecEnv", make)


@pytest.mark.parametrize("make", [POP.DeployedPopulationPPO, POP.deployed_population_for],
                         ids=["DeployedPopulationPPO", "deployed_population_for"])
def test_refusals_come_before_anything_is_built(make, stub_env):
    env_m = PPOConfig(net_arch=(64, 64), activation="tanh", n_steps=16, n_minibatches=4, fused_rollout_arch=True,
                      fused_update_arch=True)
    with pytest.raises(ValueError, match=r"member 1 has obs_mode='env'"):
        make([(_dep(), 0), (env_m, 1)], n_envs=8)
    with pytest.raises(ValueError, match="share net_arch and activation"):
        make([(_dep(), 0), (_dep(act="relu"), 1)], n_envs=8)
    with pytest.raises(ValueError, match="share net_arch and activation"):
        make([(_dep((128, 128), "relu"), 0), (_dep((256, 256), "relu"), 1)], n_envs=8)
    for net in ((48, 64), (64, 32), (64, 64, 64), (544, 64)):
        with pytest.raises(ValueError, match="12-H1-H2"):
            make([(_dep(net), 0), (_dep(net), 1)], n_envs=8)
    with pytest.raises(ValueError):
        make([], n_envs=8)


@pytest.mark.parametrize("make", [POP.DeployedPopulationPPO, POP.deployed_population_for],
                         ids=["DeployedPopulationPPO", "deployed_population_for"])
@pytest.mark.parametrize("net,act", [((64, 64), "tanh"), ((128, 128), "relu"), ((512, 256), "relu")])
def test_members_may_differ_in_velocity_alpha_and_est_max_dt(make, net, act, stub_env):
    members = [(_dep(net, act, velocity_alpha=0.8), 0), (_dep(net, act, velocity_alpha=0.95), 1),
               (_dep(net, act, velocity_alpha=0.0, est_max_dt=0.05), 2)]
    with pytest.raises(_Built):  # accepted: the class went on to build member 0's env
        make(members, n_envs=8)


def test_the_env_mode_classes_still_refuse_deployed_members(stub_env):
    for make in (POP.PopulationPPO, POP.population_for):
        with pytest.raises(ValueError, match=r"member 0 has obs_mode='deployed'"):
            make([(_dep((128, 128), "relu"), 0)], n_envs=8)
    with pytest.raises(ValueError, match=r"member 0 has obs_mode='deployed'"):
        POP.ArchPopulationPPO([(_dep(), 0)], n_envs=8)
    assert issubclass(POP.DeployedPopulationPPO, POP.ArchPopulationPPO)
    assert POP.DEPLOYED_POPULATION_KEEP_SERIAL == frozenset() or all(
        len(k) == 2 for k in POP.DEPLOYED_POPULATION_KEEP_SERIAL)


def test_keep_serial_rows_stay_off_the_population(monkeypatch, stub_env):
    monkeypatch.setattr(POP, "DEPLOYED_POPULATION_KEEP_SERIAL", frozenset({((64, 64), "tanh")}))
    with pytest.raises(ValueError, match="stays off the deployed population path"):
        POP.deployed_population_for([(_dep(), 0)], n_envs=8)
    with pytest.raises(_Built):
        POP.deployed_population_for([(_dep((128, 128), "relu"), 0)], n_envs=8)


# ---------------------------------------------------------------- optimize
def _key(t):
    return t.number, dict(t.params), t.seed, t.batch


@pytest.mark.parametrize("seed", [0, 1])
def test_no_new_flag_is_todays_driver(seed):
    a = O.parse_args(["--seed", str(seed)])
    assert (a.deployed, a.search_alpha, a.velocity_alpha) == (False, False, 0.8)
    plain = O.make_trials(60, seed, 8)
    # today's sampler, restated: eight draws per trial from one Random(seed), the fixed arch, seed * 100003 + k
    rng = random.Random(seed)
    for t in plain:
        q = {"learning_rate": O._log_uniform(rng, 1e-5, 1e-3), "n_steps": rng.choice(list(O.N_STEPS_CHOICES)),
             "batch_size": rng.choice(O.BATCH_CHOICES), "n_epochs": rng.choice(O.N_EPOCHS_CHOICES),
             "gamma_inv": O._log_uniform(rng, 0.001, 0.05), "gae_lambda": rng.uniform(0.9, 0.99),
             "clip_range": rng.uniform(0.1, 0.3), "ent_coef": O._log_uniform(rng, 1e-5, 0.1),
             "net_arch": "small", "activation_fn": "relu"}
        assert t.params == q and list(t.params) == list(EARLIER)
        assert t.seed == seed * 100_003 + t.number and t.batch == O.clamp_batch_size(q["n_steps"], 8, q["batch_size"])
        assert (t.obs_mode, t.velocity_alpha) == ("env", 0.8)
        cfg = O.ppo_config(t)
        assert cfg.obs_mode == "env" and cfg == PPOConfig(
            learning_rate=q["learning_rate"], n_steps=q["n_steps"], batch_size=t.batch, n_epochs=q["n_epochs"],
            gamma=t.gamma, gae_lambda=q["gae_lambda"], clip_range=q["clip_range"], ent_coef=q["ent_coef"])
    by = {}
    for t in plain:
        by.setdefault((t.params["n_steps"], t.batch), []).append(t.number)
    groups = O.group_trials(plain, 1000)
    assert sorted(map(tuple, by.values())) == sorted(tuple(t.number for t in g) for g in groups)
    assert [g[0].number for g in groups] == sorted(g[0].number for g in groups)
    assert O.csv_columns(plain) == O.CSV_COLUMNS and set(O.trial_row(plain[0])) == set(O.CSV_COLUMNS)
    assert list(O.CSV_COLUMNS) == open(GOLDEN_HEADER).read().split()


def test_no_new_flag_writes_the_golden_header(tmp_path):
    trials = O.make_trials(3, 0, 8)
    O.write_csv(str(tmp_path / "s.csv"), trials)
    with open(tmp_path / "s.csv") as f:
        assert f.readline().strip().split(",") == open(GOLDEN_HEADER).read().split()
    assert "velocity_alpha" not in O.format_best(trials[0])


@pytest.mark.parametrize("seed", [0, 1])
def test_search_alpha_adds_only_velocity_alpha(seed, tmp_path):
    plain = O.make_trials(120, seed, 8)
    dep = O.make_trials(120, seed, 8, deployed=True, velocity_alpha=0.95)
    srch = O.make_trials(120, seed, 8, deployed=True, search_alpha=True)
    assert [_key(t) for t in dep] == [_key(t) for t in plain]  # --deployed alone draws nothing more
    assert all((t.obs_mode, t.velocity_alpha) == ("deployed", 0.95) for t in dep)
    for p, s in zip(plain, srch):
        assert (s.number, s.seed, s.batch) == (p.number, p.seed, p.batch)
        assert {k: s.params[k] for k in EARLIER} == p.params
        assert list(s.params) == list(EARLIER) + ["velocity_alpha"]
        assert s.params["velocity_alpha"] in O.VELOCITY_ALPHA_CHOICES and s.velocity_alpha == s.params["velocity_alpha"]
        cfg = O.ppo_config(s)
        assert (cfg.obs_mode, cfg.velocity_alpha) == ("deployed", s.velocity_alpha)
    assert {s.params["velocity_alpha"] for s in srch} == {0.0, 0.5, 0.8, 0.95}
    # the alphas are the draws that follow every earlier one: the rng of the no-flag study, continued
    rng = random.Random(seed)
    for _ in range(120):
        O.sample_ppo_params(rng)
    assert [s.velocity_alpha for s in srch] == [rng.choice(O.VELOCITY_ALPHA_CHOICES) for _ in range(120)]
    # the groups are the no-flag groups (alpha is no shape), and the CSV gets one more column, last
    assert [[t.number for t in g] for g in O.group_trials(srch, 16)] == \
        [[t.number for t in g] for g in O.group_trials(plain, 16)]
    assert O.csv_columns(srch) == O.CSV_COLUMNS + ("params_velocity_alpha",)
    O.write_csv(str(tmp_path / "s.csv"), srch[:5])
    rows = O.read_csv(str(tmp_path / "s.csv"))
    with open(tmp_path / "s.csv") as f:
        assert next(csv.reader(f)) == list(O.CSV_COLUMNS) + ["params_velocity_alpha"]
    assert [r["params_velocity_alpha"] for r in rows] == [t.velocity_alpha for t in srch[:5]]
    assert "velocity_alpha" in O.format_best(srch[0])


def test_search_alpha_without_deployed_is_an_argparse_error(capsys):
    with pytest.raises(SystemExit) as e:
        O.parse_args(["--search-alpha"])
    assert e.value.code == 2 and "--search-alpha needs --deployed" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        O.main(["--search-alpha", "--n-trials", "1"])
    with pytest.raises(ValueError):
        O.make_trials(2, 0, 8, search_alpha=True)
    a = O.parse_args(["--deployed", "--search-alpha", "--velocity-alpha", "0.5"])
    assert a.deployed and a.search_alpha and a.velocity_alpha == 0.5


class _Member:
    obs_dim = 12
    num_timesteps = 4096
    policy = opt = cfg = None


class _Pop:
    def member(self, m):
        return _Member()


def test_save_best_records_the_observation_mode(tmp_path, monkeypatch):
    import uav_reinforcement_learning_control_amd.export as E
    monkeypatch.setattr(E, "save_sb3_zip", lambda path, *a, **k: path + ".zip")
    t = O.make_trials(1, 0, 8, deployed=True, velocity_alpha=0.95)[0]
    t.value = 1.0
    O.save_best(_Pop(), 0, t, str(tmp_path / "dep"), 8, 4096)
    with open(tmp_path / "dep" / "config.json") as f:
        saved = json.load(f)
    assert saved["obs_mode"] == "deployed" and saved["velocity_alpha"] == 0.95
    u = O.make_trials(1, 0, 8)[0]
    u.value = 1.0
    O.save_best(_Pop(), 0, u, str(tmp_path / "env"), 8, 4096)
    with open(tmp_path / "env" / "config.json") as f:
        plain = json.load(f)
    assert "obs_mode" not in plain and "velocity_alpha" not in plain
    assert {k: v for k, v in saved.items() if k not in ("obs_mode", "velocity_alpha")} == plain
