"""The bf16x3 policy forward (csrc/policy_net.h) held to float64 accuracy and to exact layouts, through
FusedPolicy.pack / act / post / rollout only (k_policy_pack, k_policy_act, k_rollout_post, k_rollout).

1. Accuracy: mean, value and log_prob against the float64 nets (policy_x3_ref.forward64) with the
   torch fp32 ActorCritic on the GPU as the yardstick, per output tensor
       max|got - ref64| <= 4 max|torch32 - ref64| + 1e-7 max|ref64|
   on policy_x3_ref.cases() (tests/test_policy_x3_cpu.py shows that a lost small-term MFMA or a
   two-piece split is outside this bar on the same inputs), through act, quad_rollout (both tile
   forms) and quad_rollout_post.
2. A row's bits do not depend on the batch around it.  3. A non-finite row stays in its row.
4. The critic is the same bits in every form that runs it.  5. Every entry of W1 and W2, with all
three pieces, is read where the layout says (exact selector constructions).
"""
import math

import numpy as np
import pytest
import torch

import policy_x3_ref as R

pytestmark = pytest.mark.gpu

_CASES = R.cases()
_IDS = [c[0] for c in _CASES]
SEED = 0x1234_5678_9ABC


def _fused(pol):
    from uav_reinforcement_learning_control_amd.ppo.fused import FusedPolicy
    fp = FusedPolicy(pol)
    fp.pack()
    return fp


def _bits(a, b):
    """Same bits (NaN payloads included)."""
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _act(fp, obs, deterministic=True, seed=SEED, base=0):
    n = obs.shape[0]
    o = dict(act_env=torch.empty(n, 4, device="cuda"), actions=torch.empty(1, n, 4, device="cuda"),
             log_prob=torch.empty(1, n, device="cuda"), value=torch.empty(1, n, device="cuda"))
    fp.act(obs, o["act_env"], actions=o["actions"], log_prob=o["log_prob"], value=o["value"],
           deterministic=deterministic, seed=seed, env_id_base=base)
    return {k: (v if k == "act_env" else v[0]) for k, v in o.items()}


def _env(n, seed=5):
    from uav_reinforcement_learning_control_amd.envs import QuadVecEnv
    env = QuadVecEnv(n, env="hover", wrapper=None, device="cuda:0", seed=seed, max_episode_steps=512)
    env.reset()
    return env


def _rollout1(fp, obs, deterministic=True, seed=SEED):
    """quad_rollout, one step from last_obs = obs: row 0 of the buffers is the policy on exactly these
    rows (the env steps afterwards)."""
    from uav_reinforcement_learning_control_amd import _native as N
    n = obs.shape[0]
    env = _env(n)
    f = dict(dtype=torch.float32, device="cuda")
    b = dict(obs_copy=torch.zeros(1, n, 12, **f), actions=torch.zeros(1, n, 4, **f), log_prob=torch.zeros(1, n, **f),
             value=torch.zeros(1, n, **f), episode_starts=torch.zeros(1, n, **f), rewards=torch.zeros(1, n, **f),
             last_obs=obs.clone(), last_start=torch.ones(n, **f), ep_ret=torch.zeros(n, **f),
             ep_len=torch.zeros(n, **f), stats=torch.zeros(N.POLICY_STAT_SLOTS, 3, dtype=torch.float64, device="cuda"))
    fp.rollout(env, t0=0, steps=1, seed=seed, gamma=0.99, deterministic=deterministic, **b)
    torch.cuda.synchronize()
    env.close()
    return b


def _post_values(fp, tobs, fused=False, reward=None, term=None, trunc=None):
    """buf_rew of the pending step with gamma = 1, rows = 1 (default: reward 0 and every env timed out,
    so buf_rew is V(terminal_obs) itself), through quad_rollout_post or the epilogue fused into act."""
    from uav_reinforcement_learning_control_amd import _native as N
    n = tobs.shape[0]
    z = lambda *s: torch.zeros(*s, device="cuda")
    reward = z(n) if reward is None else reward
    term = torch.zeros(n, dtype=torch.bool, device="cuda") if term is None else term
    trunc = torch.ones(n, dtype=torch.bool, device="cuda") if trunc is None else trunc
    buf_rew = torch.full((1, n), -5.0, device="cuda")
    slots = torch.zeros(N.POLICY_STAT_SLOTS, 3, dtype=torch.float64, device="cuda")
    keep = (reward, term, trunc, tobs, buf_rew, z(n), z(n), z(n), slots)
    epi = fp.make_epilogue(*keep, 1, 1.0)
    cur = torch.tensor([1, 1, 0, 0], dtype=torch.int32, device="cuda")
    if fused:
        fp.act(torch.rand(n, 12, device="cuda"), torch.empty(n, 4, device="cuda"), cursor=cur, rows=1, epilogue=epi)
    else:
        fp.post(epi, cur)
    torch.cuda.synchronize()
    return buf_rew[0]


# ---------------------------------------------------------------- 1. accuracy
@pytest.fixture(scope="module")
def case_refs():
    """Per case, built once: the packed policy, the rows on the GPU, float64 and torch fp32 results."""
    cache = {}

    def get(i):
        if i not in cache:
            name, p, obs = _CASES[i]
            pol = R.make_policy(p, "cuda")
            x = obs.cuda()
            mean64, v64 = R.forward64(p, obs)
            with torch.no_grad():
                mean32, v32 = pol.forward_heads(x)
            cache[i] = dict(name=name, p=p, pol=pol, fp=_fused(pol), x=x, mean64=mean64, v64=v64,
                            mean32=mean32, v32=v32)
        return cache[i]
    return get


def _bar(case, what, got, ref64, got32):
    err, err32, scale, ratio = R.errors(got, ref64, got32)
    print(f"RATIO {case} {what}: err {err:.3g} torch32 {err32:.3g} ratio {ratio:.2f} scale {scale:.3g}")
    return R.within_bar(got, ref64, got32), f"{case} {what}: err {err:.3g} torch32 {err32:.3g} ratio {ratio:.2f}"


def test_bounds_are_the_hover_defaults():
    from uav_reinforcement_learning_control_amd.envs import QuadVecEnv
    env = QuadVecEnv(32, env="hover", wrapper=None, device="cuda:0", seed=1)
    assert np.array_equal(np.array(env.cfg.term_low[:], np.float32), R.HOVER_TERM_LOW)
    assert np.array_equal(np.array(env.cfg.term_high[:], np.float32), R.HOVER_TERM_HIGH)
    env.close()


@pytest.mark.parametrize("i", range(len(_CASES)), ids=_IDS)
def test_act_meets_the_float64_bar(i, case_refs):
    """mean and value of act(deterministic), log_prob of a sampled act's stored actions.

    Measured kernel error / torch fp32 error (one MI355X, 2026-10-19), range over the nine cases:
    mean 0.74 .. 1.41 (worst: b-uniform), value 0.56 .. 1.04 (a-uniform), log_prob 0.70 .. 1.58
    (c-bounds); k_rollout and k_rollout_post return the same bits, so the same ratios. The bar's factor
    therefore stays the learner suite's 4. A scratch build without mfma6's a2 * b0 term measured up
    to 26 and failed every case here while tests/test_gpu_policy.py passed. Every case's figures are
    printed (RATIO lines, pytest -s)."""
    c = case_refs(i)
    det = _act(c["fp"], c["x"])
    smp = _act(c["fp"], c["x"], deterministic=False)
    with torch.no_grad():
        lp32 = c["pol"].log_prob(c["mean32"], smp["actions"])
    lp64 = R.log_prob64(c["p"], c["mean64"], smp["actions"])
    res = [_bar(c["name"], "mean", det["actions"], c["mean64"], c["mean32"]),
           _bar(c["name"], "value", det["value"], c["v64"], c["v32"]),
           _bar(c["name"], "log_prob", smp["log_prob"], lp64, lp32)]
    assert all(ok for ok, _ in res), [m for ok, m in res if not ok]
    assert _bits(smp["value"], det["value"])
    assert torch.equal(det["act_env"], det["actions"].clamp(-1, 1))


@pytest.mark.parametrize("nt", ["2", "1"])
@pytest.mark.parametrize("i", range(len(_CASES)), ids=_IDS)
def test_rollout_meets_the_float64_bar(i, nt, case_refs, monkeypatch):
    """k_rollout's first step on the same rows: the actor's W2 pieces from LDS, both tile forms. The
    same bar, and the same bits as act."""
    monkeypatch.setenv("QUADENV_ROLLOUT_NT", nt)
    c = case_refs(i)
    b = _rollout1(c["fp"], c["x"])
    res = [_bar(c["name"], f"rollout nt={nt} mean", b["actions"][0], c["mean64"], c["mean32"]),
           _bar(c["name"], f"rollout nt={nt} value", b["value"][0], c["v64"], c["v32"])]
    assert all(ok for ok, _ in res), [m for ok, m in res if not ok]
    det = _act(c["fp"], c["x"])
    assert _bits(b["actions"][0], det["actions"]) and _bits(b["value"][0], det["value"])
    assert _bits(b["obs_copy"][0], c["x"])


@pytest.mark.parametrize("i", range(len(_CASES)), ids=_IDS)
def test_post_meets_the_float64_bar(i, case_refs):
    """The TimeLimit critic (net_forward<1, 1> in k_rollout_post): every env timed out, reward 0,
    gamma 1, so buf_rew is V(terminal_obs)."""
    c = case_refs(i)
    v = _post_values(c["fp"], c["x"])
    ok, msg = _bar(c["name"], "post value", v, c["v64"], c["v32"])
    assert ok, msg


# ---------------------------------------------------------------- 2. batch independence
def test_rows_do_not_depend_on_the_batch():
    """300 fixed rows alone, scattered over n = 4,096, at the end of n = 65,536 + 97 (one full grid
    stride of 256 CUs x 4 waves x 2 tiles x 32 envs, so the last 97 of them are the whole second,
    prefetched, ragged iteration), and their first 1 and 33 rows alone (a tile with one live lane; a pair whose second
    tile has one live lane): mean, value and clipped actions are the same bits; with the same
    (seed, global env id) per row so are the sampled actions, log_prob and what the env receives."""
    p = R.policy_b(41)
    fp = _fused(R.make_policy(p, "cuda"))
    g = torch.Generator().manual_seed(42)
    rows = (R.obs_bounds(300, 43) * 0.5).cuda()
    base = 1 << 20
    want = _act(fp, rows)
    want_s = _act(fp, rows, deterministic=False, base=base)
    assert not _bits(want_s["actions"], want["actions"])   # the noise is on
    # scattered among other rows
    n = 4096
    pos = torch.randperm(n, generator=g)[:300].cuda()
    big = (torch.rand(n, 12, generator=g) * 2 - 1).cuda()
    big[pos] = rows
    got = _act(fp, big)
    for k in ("actions", "value", "act_env"):
        assert _bits(got[k][pos], want[k]), k
    # at the end of one grid stride + 97
    n = 65536 + 97
    big = (torch.rand(n, 12, generator=g) * 2 - 1).cuda()
    big[n - 300:] = rows
    got = _act(fp, big)
    got_s = _act(fp, big, deterministic=False, base=base - (n - 300))
    for k in ("actions", "value", "act_env"):
        assert _bits(got[k][n - 300:], want[k]), k
    for k in ("actions", "log_prob", "value", "act_env"):
        assert _bits(got_s[k][n - 300:], want_s[k]), k
    for m in (1, 33):
        got = _act(fp, rows[:m].contiguous())
        got_s = _act(fp, rows[:m].contiguous(), deterministic=False, base=base)
        for k in ("actions", "value", "act_env"):
            assert _bits(got[k], want[k][:m]), (m, k)
        for k in ("actions", "log_prob", "value", "act_env"):
            assert _bits(got_s[k], want_s[k][:m]), (m, k)


# ---------------------------------------------------------------- 3. a bad row stays in its row
_POISON = {5: {0: math.nan, 9: math.inf, 4: -3e38},               # lane half 0 of the first tile
           37: {3: -math.inf, 10: 3e38, 8: -math.nan, 1: 3e38},   # the second tile of a pair
           64 + 31: {7: 3e38, 11: math.nan, 2: math.inf}}         # the last lane of a tile


def _poisoned(clean):
    bad = clean.clone()
    for r, feats in _POISON.items():
        for f, v in feats.items():
            bad[r, f] = v
    return bad


def test_a_non_finite_row_stays_in_its_row(monkeypatch):
    """NaN, +-Inf and 3e38 in rows 5, 37 and 95 of n = 128 (features of both lane halves): every other
    row's outputs are the bits of a run where those rows hold ordinary values, through act
    (deterministic and sampled) and k_rollout (both tile forms), and what the env receives is finite
    and within [-1, 1] on every row (the clamp maps NaN to -1).

    Recorded, not asserted -- what a poisoned row's own mean / value read (one MI355X, 2026-10-19;
    printed as POISON lines): finite, and the same for all three rows in every form, namely the nets'
    output for relu(h1) = 0, W3 relu(b2) + b3. Each of these rows holds a NaN (an Inf becomes one in the
    split: Inf - Inf), every hidden pre-activation of the row is then NaN, and the integer-max ReLU
    read all of them as 0, so the NaNs the MFMA returned had the sign bit set."""
    p = R.policy_a(51)
    fp = _fused(R.make_policy(p, "cuda"))
    n = 128
    clean = R.obs_uniform(n, 52).cuda()
    bad = _poisoned(clean)
    others = torch.ones(n, dtype=torch.bool, device="cuda")
    others[list(_POISON)] = False
    assert others.sum().item() == n - 3 and not torch.isfinite(bad[~others]).all(1).any()
    for det in (True, False):
        a, b = _act(fp, clean, deterministic=det), _act(fp, bad, deterministic=det)
        for k in ("actions", "log_prob", "value", "act_env"):
            assert _bits(a[k][others], b[k][others]), (det, k)
        assert torch.isfinite(b["act_env"]).all() and b["act_env"].abs().max().item() <= 1.0
        if det:
            for r in _POISON:
                print(f"POISON act row {r}: mean {b['actions'][r].tolist()} value {b['value'][r].item()} "
                      f"act_env {b['act_env'][r].tolist()}")
    for nt in ("2", "1"):
        monkeypatch.setenv("QUADENV_ROLLOUT_NT", nt)
        for det in (True, False):
            a, b = _rollout1(fp, clean, deterministic=det), _rollout1(fp, bad, deterministic=det)
            sel = lambda t: t[others] if t.shape[0] == n else t[:, others]   # the env axis ([n, ..] or [1, n, ..])
            for k in ("actions", "log_prob", "value", "rewards", "last_obs", "obs_copy", "ep_ret"):
                assert _bits(sel(a[k]), sel(b[k])), (nt, det, k)
            # the env was never handed a NaN: every env's next observation and reward are finite
            assert torch.isfinite(b["last_obs"]).all() and torch.isfinite(b["rewards"]).all(), (nt, det)
            ref = _act(fp, bad, deterministic=det)
            assert _bits(b["actions"][0][others], ref["actions"][others]), (nt, det)
            if det:
                for r in _POISON:
                    print(f"POISON rollout nt={nt} row {r}: mean {b['actions'][0][r].tolist()} "
                          f"value {b['value'][0][r].item()}")


# ---------------------------------------------------------------- 4. one critic
def test_one_critic_whichever_form_runs_it():
    """V of 1,000 rows through net_forward2<2> (act), net_forward<1, 1> in k_rollout_post and the
    same in act's fused epilogue: the same bits, within the accuracy bar; then sparse timeouts (one in
    some tiles, none in others, one beside a terminated-and-truncated env): bootstrapped rows are
    V's bits, all other rows the reward's."""
    p = R.policy_b(61)
    pol = R.make_policy(p, "cuda")
    fp = _fused(pol)
    n = 1000
    tobs = (R.obs_bounds(n, 62) * 0.3).cuda()
    v_act = _act(fp, tobs)["value"]
    v_post = _post_values(fp, tobs)
    v_fused = _post_values(fp, tobs, fused=True)
    assert _bits(v_post, v_act) and _bits(v_fused, v_act)
    _, v64 = R.forward64(p, tobs)
    with torch.no_grad():
        v32 = pol.value(tobs)
    ok, msg = _bar("one-critic", "value", v_act, v64, v32)
    assert ok, msg
    # sparse: tiles 0, 2, 5 and the ragged last tile (31: envs 992..999) hold exactly one timeout, tile 7 a
    # timeout beside a terminated-and-truncated env, every other tile none
    timeouts = [3, 2 * 32 + 31, 5 * 32, 7 * 32 + 10, 31 * 32 + 7]
    g = torch.Generator().manual_seed(63)
    reward = (torch.rand(n, generator=g) + 0.5).cuda()
    reward[timeouts] = 0.0
    term = (torch.rand(n, generator=g) < 0.05).cuda()
    trunc = torch.zeros(n, dtype=torch.bool, device="cuda")
    term[timeouts] = False
    trunc[timeouts] = True
    term[7 * 32 + 11] = trunc[7 * 32 + 11] = True
    boot = torch.zeros(n, dtype=torch.bool, device="cuda")
    boot[timeouts] = True
    for fused in (False, True):
        r = _post_values(fp, tobs, fused=fused, reward=reward, term=term, trunc=trunc)
        assert _bits(r[boot], v_act[boot]), fused
        assert _bits(r[~boot], reward[~boot]), fused


# ---------------------------------------------------------------- 5. exact selectors for the weight pieces
def _selector_policy(seed):
    """Zero biases, log_std 0, W2 = I, full-mantissa random W1 and W2 candidates; heads set per pass."""
    g = torch.Generator().manual_seed(seed)
    p = {k: torch.zeros(R.SHAPES[k]) for k in R.NAMES}
    full = lambda *s: (torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1).float()
    for net in ("pi", "vf"):
        p[f"{net}_w0"] = full(128, 12)
        p[f"{net}_w1"] = torch.eye(128)
    return p, full(128, 128), full(128, 128)


def _heads(pol, k):
    """Pass k: the critic reads neuron k, actor output q reads neuron (4k + q) % 128, weight 1.0."""
    with torch.no_grad():
        pol.action_net.weight.zero_()
        pol.value_net.weight.zero_()
        idx = (4 * k + torch.arange(4)) % 128
        pol.action_net.weight[torch.arange(4), idx] = 1.0
        pol.value_net.weight[0, k] = 1.0
    return idx


def test_every_w1_entry_with_all_pieces_exact():
    """W1 full-mantissa random, W2 = I, one-hot heads, rows +-e_f: x = +-1 is a single piece, so every
    product and partial sum is exact and the outputs must be relu(+-W1[m, f]) bit for bit -- which
    needs all three pieces of every W1 entry of both nets in the right place (k_policy_pack's W1
    pieces). 128 tiny passes move the heads over all neurons."""
    p, _, _ = _selector_policy(71)
    pol = R.make_policy(p, "cuda")
    from uav_reinforcement_learning_control_amd.ppo.fused import FusedPolicy
    fp = FusedPolicy(pol)
    rows = torch.cat([torch.eye(12), -torch.eye(12)]).cuda()               # row f: +e_f, row 12 + f: -e_f
    w1a = torch.cat([p["pi_w0"].t(), -p["pi_w0"].t()]).cuda()              # [24, 128]: +-W1[m, f]
    w1c = torch.cat([p["vf_w0"].t(), -p["vf_w0"].t()]).cuda()
    seen_a = torch.zeros(24, 128, dtype=torch.bool)
    seen_c = torch.zeros(24, 128, dtype=torch.bool)
    got_a, got_c, want_a, want_c = [], [], [], []
    for k in range(128):
        idx = _heads(pol, k)
        fp.pack()
        o = _act(fp, rows)
        got_a.append(o["actions"]); got_c.append(o["value"])
        want_a.append(torch.relu(w1a[:, idx.cuda()])); want_c.append(torch.relu(w1c[:, k]))
        seen_a[:, idx] = True; seen_c[:, k] = True
    got_a, got_c, want_a, want_c = (torch.stack(t) for t in (got_a, got_c, want_a, want_c))
    assert seen_a.all() and seen_c.all()                     # every entry read with each sign
    assert (want_a > 0).sum() > 1000 and (want_c > 0).sum() > 1000
    assert _bits(got_a, want_a), f"{(got_a != want_a).sum().item()} actor outputs differ"
    assert _bits(got_c, want_c), f"{(got_c != want_c).sum().item()} critic outputs differ"


def test_every_w2_entry_with_all_pieces_exact(monkeypatch):
    """Layer 1 emits an exact one-hot: features 2 and 9 (one per lane half) hold j and j^2, W1[k] =
    (2k, -1) on them and b1[k] = 1 - k^2, so h1[k](row j) = 1 - (k - j)^2 -- integers below 2^15, 1 at
    k = j and <= 0 elsewhere. Then h2[m](row j) = W2[m, j] exactly for full-mantissa random W2 (b2 = 0;
    the three pieces times 1.0 sum small-first to the f32 value) and a one-hot head reads
    relu(W2[m, j]); a second pass with -W2 reads the other sign. The actor through act and k_rollout
    (both tile forms: the L2 pieces and the LDS pieces on both sides of LP_SPLIT), the critic through
    act and k_rollout_post."""
    p, w2a, w2c = _selector_policy(72)
    j = torch.arange(128, dtype=torch.float32)
    for net in ("pi", "vf"):
        w = torch.zeros(128, 12)
        w[:, 2], w[:, 9] = 2 * j, -1.0
        p[f"{net}_w0"] = w
        p[f"{net}_b0"] = 1 - j * j
    rows = torch.zeros(128, 12)
    rows[:, 2], rows[:, 9] = j, j * j
    rows = rows.cuda()
    pol = R.make_policy(p, "cuda")
    from uav_reinforcement_learning_control_amd.ppo.fused import FusedPolicy
    fp = FusedPolicy(pol)
    ex = pol.mlp_extractor
    n_checked = 0
    for sign in (1.0, -1.0):
        with torch.no_grad():
            ex.policy_net[2].weight.copy_(sign * w2a)
            ex.value_net[2].weight.copy_(sign * w2c)
        wa, wc = torch.relu(sign * w2a).cuda(), torch.relu(sign * w2c).cuda()   # [m, j]
        seen_a = torch.zeros(128, dtype=torch.bool)
        got = {k: [] for k in ("act_a", "act_c", "post_c", "roll1_a", "roll2_a")}
        want_a, want_c = [], []
        for k in range(128):
            idx = _heads(pol, k)
            fp.pack()
            o = _act(fp, rows)
            got["act_a"].append(o["actions"]); got["act_c"].append(o["value"])
            got["post_c"].append(_post_values(fp, rows))
            want_a.append(wa[idx.cuda()].t()); want_c.append(wc[k])            # row j reads W2[m, j]
            seen_a[idx] = True
            if k < 32:  # 4 neurons per pass: 32 passes read every actor neuron
                for nt in ("1", "2"):
                    monkeypatch.setenv("QUADENV_ROLLOUT_NT", nt)
                    got[f"roll{nt}_a"].append(_rollout1(fp, rows)["actions"][0])
        assert seen_a.all() and len(want_c) == 128             # every W2 row of both nets, all 128 columns (rows j)
        want_a, want_c = torch.stack(want_a), torch.stack(want_c)
        assert (want_a > 0).sum() > 1000 and (want_c > 0).sum() > 1000
        for name, g in got.items():
            g = torch.stack(g)
            want = want_c if name.endswith("_c") else want_a[:g.shape[0]]
            assert _bits(g, want), f"sign {sign} {name}: {(g != want).sum().item()} outputs differ"
            n_checked += g.numel()
    # per sign: the critic through act and post, the actor through act (128 passes) and two rollout forms (32)
    assert n_checked == 2 * (2 * 128 * 128 + 128 * 128 * 4 + 2 * 32 * 128 * 4)
