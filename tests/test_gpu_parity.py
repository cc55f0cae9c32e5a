"""GPU parity: the HIP step/reset (through the C ABI) against the float64 CPU oracle from the
identical (state, action), and against the reference golden vectors.

Parity bar (DESIGN.md "Parity"): obs / reward / voltage |d| <= 1e-5 |ref| + 1e-6; qpos / qvel (and
their float32 copies in info["state"]) |d| <= 1e-5 max(|ref|, |pre-step|) + 1e-6 (float32 error is
relative to the step's operands);
terminated / truncated / step counters bit-exact; reset draws bit-exact.
"""
import os

import numpy as np
import pytest
import torch

from oracle import oracle as O

pytestmark = pytest.mark.gpu

VARIANTS = [("hover", None, O.ENV_HOVER, O.WRAP_NONE),
            ("hover", "RateControlWrapper", O.ENV_HOVER, O.WRAP_CTBR),
            ("trajectory", None, O.ENV_TRAJ, O.WRAP_NONE),
            ("trajectory", "RateControlWrapper", O.ENV_TRAJ, O.WRAP_CTBR)]


def _env(n, env="hover", wrapper=None, **kw):
    from uav_reinforcement_learning_control_amd.envs import QuadVecEnv
    return QuadVecEnv(n, env=env, wrapper=wrapper, device="cuda:0", **kw)


def parity_ok(got, ref, pre=None, rtol=1e-5, atol=1e-6):
    got = np.asarray(got, np.float64); ref = np.asarray(ref, np.float64)
    scale = np.abs(ref) if pre is None else np.maximum(np.abs(ref), np.abs(np.asarray(pre, np.float64)))
    both_nan = np.isnan(got) & np.isnan(ref)
    return np.all(both_nan | (np.abs(got - ref) <= rtol * scale + atol), axis=-1)


# The Euler columns (state12[3:6], obs[3:6]). scipy's as_euler('xyz') of a
# quaternion has roll and yaw individually ill-conditioned as |pitch| -> pi/2: d(roll), d(yaw) ~
# |dq| / cos(pitch), while roll - sign(pitch) yaw stays well-conditioned. The state is float32 (a
# design decision), so the quaternion a step produces carries ~1 ulp of rounding whatever the
# implementation: rounding the float64 oracle's own post-step quaternion to float32 moves roll / yaw
# by up to 1.2e-4 at cos(pitch) = 3e-4. So the Euler columns are pinned in parts, each at the plain
# bar |d| <= 1e-5 |ref| + 1e-6 with no extra tolerance: (i) the post-step quaternion qpos[3:7]
# against the oracle's; (ii) state12[3:6] and obs[3:6] against the oracle's float64 quat -> Euler
# (+ normalize) OF THE KERNEL'S OWN float32 QUATERNION (the conversion's arithmetic, at any pitch);
# (iii) roll - sign(pitch) yaw against the oracle's (euler_combination_ok).
NON_EULER = [0, 1, 2, 6, 7, 8, 9, 10, 11]


def euler_of_quat(qpos):
    """float32 scipy Euler angles of the quaternions qpos[:, 3:7] (the oracle's float64 conversion)."""
    return O.quat_to_euler_batch(np.atleast_2d(np.asarray(qpos, np.float64))[:, 3:7]).astype(np.float32)


def obs_euler_of_quat(qpos, obs_bounds=None):
    """obs[3:6] of those angles: normalize (utils/normalization.py:7-17) in float32, NumPy's order.
    obs_bounds = (obs_low, obs_high) of a handle whose bounds are not the defaults."""
    e = euler_of_quat(qpos)
    low, high = (OBS_LOW, OBS_HIGH) if obs_bounds is None else (np.asarray(b, np.float32) for b in obs_bounds)
    lo, hi = low[3:6], high[3:6]
    return (np.float32(2) * (e - lo)) / (hi - lo) - np.float32(1)


def euler_ok(got_s12, got_obs, got_qpos, ref_qpos, obs_bounds=None):
    """Per row: (i) the quaternion vs the oracle's and (ii) the Euler columns of state12 (and of obs,
    unless got_obs is None) vs the conversion of the kernel's own quaternion, at the plain bar."""
    gq = np.atleast_2d(got_qpos)
    ok = parity_ok(gq[:, 3:7], np.atleast_2d(ref_qpos)[:, 3:7])
    ok &= parity_ok(np.atleast_2d(got_s12)[:, 3:6], euler_of_quat(gq))
    if got_obs is not None:
        ok &= parity_ok(np.atleast_2d(got_obs)[:, 3:6], obs_euler_of_quat(gq, obs_bounds))
    return ok


def euler_combination_ok(got_s12, ref_s12, rtol=1e-5, atol=1e-6):
    """roll - sign(pitch) yaw (wrapped to (-pi, pi]) of the step's state12 within the plain bar:
    the part of the attitude the quaternion determines well at any pitch."""
    g = np.atleast_2d(np.asarray(got_s12, np.float64)); r = np.atleast_2d(np.asarray(ref_s12, np.float64))
    sg = np.where(r[:, 4] >= 0, 1.0, -1.0)
    wrap = lambda a: (a + np.pi) % (2 * np.pi) - np.pi
    cg, cr = wrap(g[:, 3] - sg * g[:, 5]), wrap(r[:, 3] - sg * r[:, 5])
    d = np.abs(wrap(cg - cr))
    return d <= rtol * np.abs(cr) + atol


_OC = O.default_cfg(O.ENV_HOVER, O.WRAP_NONE)
OBS_SPAN = np.array(_OC.obs_high[:], np.float64) - np.array(_OC.obs_low[:], np.float64)  # same for both kinds
OBS_LOW, OBS_HIGH = np.array(_OC.obs_low[:], np.float32), np.array(_OC.obs_high[:], np.float32)
CANCEL = 0.1  # the documented class: |ref| <= CANCEL |pre|, a step that removed >= 90 % of the operand


def operand_only(got, ref, pre, rtol=1e-5, atol=1e-6):
    """Components that meet the operand-relative bar (|d| <= rtol max(|ref|, |pre|) + atol) but
    not SURVEY 8(d)'s strict |d| <= rtol |ref| + atol. Returns (count, outside): `outside` lists
    the components that are NOT near-cancelling updates (|ref| > CANCEL |pre|) -- always a failure."""
    got = np.asarray(got, np.float64); ref = np.asarray(ref, np.float64); pre = np.asarray(pre, np.float64)
    err = np.abs(got - ref)
    strict = err <= rtol * np.abs(ref) + atol
    loose = err <= rtol * np.maximum(np.abs(ref), np.abs(pre)) + atol
    only = loose & ~strict & ~(np.isnan(got) & np.isnan(ref))
    outside = np.argwhere(only & (np.abs(ref) > CANCEL * np.abs(pre)))
    return int(only.sum()), outside


def _random_states(n, rng, wide=True, kind=O.ENV_HOVER):
    """kind: the voltage is drawn in the kind's [min_voltage, nominal_voltage] (7.6 .. 8.4 V hover, 13.2 ..
    16.8 V trajectory). A trajectory env given a hover voltage clips to min_voltage on its first step, which
    hides the sag constants vdrop_base / vdrop_load from every comparison."""
    qpos = np.zeros((n, 11), np.float32)
    qpos[:, :3] = rng.uniform([-1.9, -1.9, 0.05], [1.9, 1.9, 1.95], (n, 3))
    q = rng.normal(size=(n, 4))
    qpos[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    qpos[:, 7:] = rng.uniform(-60, 60, (n, 4))
    qvel = np.zeros((n, 10), np.float32)
    s = 3.0 if wide else 0.5
    qvel[:, :3] = rng.normal(0, s, (n, 3))
    qvel[:, 3:6] = rng.normal(0, 2 * s, (n, 3))
    qvel[:, 6:] = rng.normal(0, 10 * s, (n, 4))
    volt = rng.uniform(*((13.2, 16.8) if kind == O.ENV_TRAJ else (7.6, 8.4)), n).astype(np.float32)
    tgt = rng.uniform([-1.5, -1.5, 0.3], [1.5, 1.5, 1.8], (n, 3)).astype(np.float32)
    step = rng.integers(0, 512, n).astype(np.int32)
    rint = rng.uniform(-0.01, 0.01, (n, 3)).astype(np.float32)
    return dict(qpos=qpos, qvel=qvel, voltage=volt, target=tgt, step_count=step, rate_int=rint)


def _oracle_step(kind, wrap, st, acts, max_steps=None):
    cfg = O.default_cfg(kind, wrap)
    if max_steps:
        cfg.max_episode_steps = max_steps
    outs = []
    for i in range(len(acts)):
        e = O.Env(cfg=cfg)
        e.set_full_state(st["qpos"][i], st["qvel"][i], st["voltage"][i], st["target"][i],
                         st["step_count"][i], st["rate_int"][i])
        o = O.out_to_dict(e.step(acts[i]))
        o["qpos"] = e.qpos; o["qvel"] = e.qvel; o["rate_int"] = np.array(e.s.rate_int[:])
        outs.append(o)
    return outs


def _gpu_step(env, st, acts):
    env.set_state(**st)
    a = torch.from_numpy(np.ascontiguousarray(acts, np.float32)).cuda()
    obs, rew, te, tr, inf = env.step(a, info="full")
    torch.cuda.synchronize()
    g = env.get_state()
    return dict(obs=obs.cpu().numpy(), reward=rew.cpu().numpy(), terminated=te.cpu().numpy(),
                truncated=tr.cpu().numpy(), term_obs=inf["terminal_observation"].cpu().numpy(),
                state12=inf["state"].cpu().numpy(), motor=inf["motor_commands"].cpu().numpy(),
                vscale=inf["voltage_scale"].cpu().numpy(), **g)


def _pre12(st, i):
    """Pre-step operand scale for state12 = [pos, euler, v, w]: the same bar as qpos / qvel
    (position and rates are those values; the Euler angles get none)."""
    return np.concatenate([st["qpos"][i][:3], np.zeros(3, np.float32), st["qvel"][i][:6]])


@pytest.fixture(params=["0", "0t", "0d", "0w", "0wt"])
def kernel_variant(request, monkeypatch):
    """Every step kernel form must be exact: the one-thread-per-env step waves with helper waves
    drawing the resets (k_step_h, the form at every size) -- in 64-env blocks ("0", the form up to
    32,768 envs; "0t" with the nt state cache policy, forced by QUADENV_NT: the form from 2M envs; "0d"
    the same as k_step_hd, the 7-waves-per-SIMD DRAM form of >= 4M-env batches, forced by QUADENV_HD)
    and in the 256-env blocks of the batches between ("0w", forced by QUADENV_HBLOCK; "0wt" with the nt
    policy of the 65,536-env-scale batches). (The one-wave k_step and the lane-group k_step_g forms
    were A/B builds, removed from the library in round 6.)"""
    if "w" in request.param:
        monkeypatch.setenv("QUADENV_HBLOCK", "256")
    else:
        monkeypatch.delenv("QUADENV_HBLOCK", raising=False)
    if request.param.endswith(("t", "d")):
        monkeypatch.setenv("QUADENV_NT", "1")
    else:
        monkeypatch.delenv("QUADENV_NT", raising=False)
    if request.param.endswith("d"):
        monkeypatch.setenv("QUADENV_HD", "1")
    else:
        monkeypatch.delenv("QUADENV_HD", raising=False)
    return request.param


@pytest.fixture(params=["1", "0"])
def spec_mode(request, monkeypatch):
    """Default-config handles run the kernels with the reference constants compiled in
    (kconsts_default.h); QUADENV_SPEC=0 forces the generic kernels that read the handle's block."""
    monkeypatch.setenv("QUADENV_SPEC", request.param)
    return request.param


def test_kernel_form_pins(monkeypatch):
    """QUADENV_HD / QUADENV_NT / QUADENV_HBLOCK pin the size policy (quad_create reads them); k_step_hd
    (bit 9) is only ever the 64-env nt launch: pinned on, it needs the nt policy and 64-env blocks."""
    from uav_reinforcement_learning_control_amd import _native as N
    for v in ("QUADENV_HD", "QUADENV_NT", "QUADENV_HBLOCK"):
        monkeypatch.delenv(v, raising=False)
    cases = ((1 << 22, dict(QUADENV_HD="0"), 32 | 256), (1 << 22, dict(QUADENV_NT="0"), 32),
             (1 << 22, dict(QUADENV_HBLOCK="256"), 32 | 128 | 256), (4096, dict(QUADENV_HD="1"), 32),
             (4096, dict(QUADENV_HD="1", QUADENV_NT="1"), 32 | 256 | 512),
             (65536, dict(QUADENV_HD="1"), 32 | 128 | 256), (65536, dict(QUADENV_HD="1", QUADENV_HBLOCK="64"), 32 | 256 | 512))
    for n, pins, form in cases:
        for k, v in pins.items():
            monkeypatch.setenv(k, v)
        e = _env(n)
        assert N.lib().quad_kernel_form(e._h) & ~16 == form, (n, pins)
        e.close()
        for k in pins:
            monkeypatch.delenv(k)


def test_kernel_form_selection(spec_mode):
    from uav_reinforcement_learning_control_amd import _native as N
    # 32: helper waves (k_step_h, the form at every size), + 128: in 256-env blocks (32,769 ..
    # 2,097,151 envs), + 256: with the nt state cache policy (65,536-env-scale batches and from 2M
    # envs), + 512: as k_step_hd (from 4M envs)
    for n, form in ((4096, 32), (32768, 32), (32769, 32 | 128 | 256), (65536, 32 | 128 | 256),
                    (300000, 32 | 128), ((1 << 20) + 64, 32 | 128), ((1 << 21) - 64, 32 | 128),
                    (1 << 21, 32 | 256), ((1 << 22) - 64, 32 | 256), (1 << 22, 32 | 256 | 512)):
        e = _env(n)
        assert N.lib().quad_kernel_form(e._h) == form | (16 if spec_mode == "1" else 0), n
        e.close()
    for kw in (dict(max_episode_steps=100), dict(cfg_overrides=dict(density=1.0))):
        e = _env(1024, **kw)  # not the reference default: generic kernels
        assert N.lib().quad_kernel_form(e._h) == 32
        e.close()
    for env_name, wrapper in (("hover", "RateControlWrapper"), ("trajectory", None), ("trajectory", "RateControlWrapper")):
        e = _env(1024, env_name, wrapper)
        assert N.lib().quad_kernel_form(e._h) == 32 | (16 if spec_mode == "1" else 0), (env_name, wrapper)
        e.close()
    # RELPOS and brax handles launch k_step_relpos / k_step_brax whatever their size: no form bits
    from uav_reinforcement_learning_control_amd.envs import QuadVecEnv
    for kw in (dict(env="hover", wrapper="RelPosActWrapper"), dict(env="trajectory", wrapper="RelPosActWrapper"),
               dict(env="brax_hover"), dict(env="brax_jax_mjx")):
        e = QuadVecEnv(1024, device="cuda:0", seed=0, **kw)
        assert N.lib().quad_kernel_form(e._h) == 64, kw
        e.close()


@pytest.mark.parametrize("env_name,wrapper,kind,wrap", VARIANTS)
def test_step_matches_oracle_random_states(env_name, wrapper, kind, wrap, kernel_variant, spec_mode):
    n = 3000
    rng = np.random.default_rng(17 + kind * 2 + wrap)
    st = _random_states(n, rng, kind=kind)
    acts = rng.uniform(-1.3, 1.3, (n, 4)).astype(np.float32)
    env = _env(n, env_name, wrapper, auto_reset=False)
    g = _gpu_step(env, st, acts)
    ref = _oracle_step(kind, wrap, st, acts)
    bad = []
    eul = euler_ok(g["state12"], g["obs"], g["qpos"], np.stack([o["qpos"] for o in ref]))
    for i, o in enumerate(ref):
        ok = (g["terminated"][i] == o["terminated"] and g["truncated"][i] == o["truncated"]
              and g["step_count"][i] == st["step_count"][i] + 1
              and parity_ok(g["obs"][i][NON_EULER], o["obs"][NON_EULER])
              and parity_ok(g["reward"][i], o["reward"])
              and parity_ok(g["voltage"][i], o["voltage"])
              and parity_ok(g["qpos"][i], o["qpos"], st["qpos"][i])
              and parity_ok(g["qvel"][i], o["qvel"], st["qvel"][i])
              and parity_ok(g["motor"][i], o["motor_commands"])
              and parity_ok(g["state12"][i][NON_EULER], o["state12"][NON_EULER], _pre12(st, i)[NON_EULER])
              and eul[i]
              and euler_combination_ok(g["state12"][i], o["state12"]).all()
              and parity_ok(g["rate_int"][i], o["rate_int"], st["rate_int"][i], atol=1e-9))
        if not ok:
            bad.append(i)
    assert not bad, (len(bad), bad[:5])
    # how many envs pass only because of the operand-relative slack, and that every such
    # component is a near-cancelling update; reported, bounded, never widened
    nq, oq = operand_only(g["qpos"], np.stack([o["qpos"] for o in ref]), st["qpos"])
    nv, ov = operand_only(g["qvel"], np.stack([o["qvel"] for o in ref]), st["qvel"])
    ns, os_ = operand_only(g["state12"], np.stack([o["state12"] for o in ref]),
                           np.stack([_pre12(st, i) for i in range(n)]))
    print(f"\noperand-relative-only components ({env_name}, {wrapper}, form {kernel_variant}, spec {spec_mode}): "
          f"qpos {nq}, qvel {nv}, state12 {ns} of {n} envs")
    assert len(oq) == len(ov) == len(os_) == 0, (oq[:5], ov[:5], os_[:5])
    assert nq + nv + ns <= 0.01 * n
    env.close()


@pytest.mark.parametrize("name,kind,wrap,ms", [("hover_steps", 0, 0, None), ("hover_trunc", 0, 0, 15),
                                               ("hover_nan", 0, 0, None), ("ctbr_steps", 0, 1, None),
                                               ("traj_ctbr_steps", 1, 1, None), ("traj_steps", 1, 0, None)])
def test_step_matches_reference_goldens(golden_dir, name, kind, wrap, ms, kernel_variant, spec_mode):
    d = np.load(os.path.join(golden_dir, f"golden_{name}.npz"))
    n = len(d["action"])
    env = _env(n, "trajectory" if kind else "hover", "RateControlWrapper" if wrap else None,
               auto_reset=False, max_episode_steps=ms)
    st = dict(qpos=d["pre_qpos"].astype(np.float32), qvel=d["pre_qvel"].astype(np.float32),
              voltage=d["pre_voltage"].astype(np.float32), target=d["pre_target"],
              step_count=d["pre_step"].astype(np.int32), rate_int=d["pre_rate_int"].astype(np.float32))
    g = _gpu_step(env, st, d["action"])
    # identical-state oracle (the GPU starts from the float32-rounded golden state)
    ref = _oracle_step(kind, wrap, st, d["action"], ms)
    for i, o in enumerate(ref):
        assert g["terminated"][i] == o["terminated"] == d["terminated"][i], i
        assert g["truncated"][i] == o["truncated"] == d["truncated"][i], i
        assert parity_ok(g["obs"][i], o["obs"]) and parity_ok(g["obs"][i], d["obs"][i]), i
        assert parity_ok(g["reward"][i], o["reward"]) and parity_ok(g["reward"][i], d["reward"][i]), i
        assert parity_ok(g["qvel"][i], o["qvel"], st["qvel"][i]), i
        assert parity_ok(g["qpos"][i], o["qpos"], st["qpos"][i]), i
    nq, oq = operand_only(g["qpos"], np.stack([o["qpos"] for o in ref]), st["qpos"])
    nv, ov = operand_only(g["qvel"], np.stack([o["qvel"] for o in ref]), st["qvel"])
    print(f"\noperand-relative-only components ({name}, form {kernel_variant}): qpos {nq}, qvel {nv} of {n}")
    assert len(oq) == len(ov) == 0, (oq[:5], ov[:5])
    assert nq + nv <= max(1, 0.01 * n)
    env.close()


@pytest.mark.parametrize("env_name,kind", [("hover", 0), ("trajectory", 1)])
def test_reset_bit_exact_with_oracle_draws(env_name, kind):
    n = 5000
    env = _env(n, env_name, seed=2024, env_id_base=1000)
    obs = env.reset().cpu().numpy()
    obs2 = env.reset().cpu().numpy()  # second episode: counter 1
    st = env.get_state()
    cfg = O.default_cfg(kind, O.WRAP_NONE)
    for i in range(0, n, 7):
        for ep, ob in ((0, obs), (1, obs2)):
            i12, t3 = O.reset_draw(cfg, 2024, 1000 + i, ep)
            e = O.Env(cfg=cfg)
            ref = e.reset_with(i12, t3)
            assert np.array_equal(ob[i], ref), (i, ep)
        assert np.array_equal(st["qpos"][i][:3], i12[:3]) and np.array_equal(st["qvel"][i][:6], i12[6:])
        np.testing.assert_allclose(st["qpos"][i][3:7], e.qpos[3:7], atol=2e-7)
        assert np.all(st["qpos"][i][7:] == 0) and np.all(st["qvel"][i][6:] == 0)
        assert st["step_count"][i] == 0 and st["episode"][i] == 2
        assert np.array_equal(st["target"][i], i12[:3] if kind else t3)
    env.close()


def test_masked_reset_and_seed():
    n = 1024
    env = _env(n, seed=5)
    a = env.reset().clone()
    mask = torch.zeros(n, dtype=torch.bool, device="cuda:0"); mask[::3] = True
    b = env.reset(mask=mask).clone()
    assert torch.equal(a[~mask], b[~mask]) and not torch.equal(a[mask], b[mask])
    c = env.reset(seed=5).clone()  # re-seeding restarts the episode counters
    assert torch.equal(a, c)
    env.close()


def test_auto_reset_semantics(kernel_variant):
    n = 4096
    env = _env(n, seed=9, max_episode_steps=6)
    env.reset()
    cfg = O.default_cfg(O.ENV_HOVER, O.WRAP_NONE)
    saw_term = saw_trunc = False
    for k in range(20):
        pre = env.get_state()
        acts = env.random_actions(k)
        obs, rew, te, tr, inf = env.step(acts)
        torch.cuda.synchronize()
        te = te.cpu().numpy(); tr = tr.cpu().numpy(); obs = obs.cpu().numpy()
        tobs = inf["terminal_observation"].cpu().numpy()
        tl = inf["TimeLimit.truncated"].cpu().numpy()
        post = env.get_state()
        a = acts.cpu().numpy()
        done = np.nonzero(te | tr)[0]
        saw_term |= te.any(); saw_trunc |= tr.any()
        assert np.array_equal(tl, tr & ~te)
        for i in done[:50]:
            e = O.Env(cfg=cfg)
            e.set_full_state(pre["qpos"][i], pre["qvel"][i], pre["voltage"][i], pre["target"][i],
                             pre["step_count"][i])
            o = O.out_to_dict(e.step(a[i]))
            assert parity_ok(tobs[i], o["obs"])
            ep = pre["episode"][i]
            i12, t3 = O.reset_draw(cfg, 9, i, ep)
            assert np.array_equal(obs[i], O.Env(cfg=cfg).reset_with(i12, t3))
            assert post["step_count"][i] == 0 and post["episode"][i] == ep + 1
        notdone = np.nonzero(~(te | tr))[0]
        assert np.all(post["step_count"][notdone] == pre["step_count"][notdone] + 1)
    assert saw_term and saw_trunc
    env.close()


def test_random_actions_match_oracle():
    n = 2048
    env = _env(n, seed=77, env_id_base=123)
    a = env.random_actions(42).cpu().numpy()
    for i in range(0, n, 13):
        assert np.array_equal(a[i], O.random_action(77, 123 + i, 42))
    assert a.min() >= -1 and a.max() < 1
    env.close()


def test_nan_and_extreme_actions(kernel_variant):
    n = 256
    rng = np.random.default_rng(3)
    st = _random_states(n, rng, wide=False)
    st["step_count"][:] = 0
    acts = rng.uniform(-1, 1, (n, 4)).astype(np.float32)
    acts[0::4, 0] = np.nan
    acts[1::4, 2] = np.inf
    acts[2::4, 1] = -np.inf
    acts[3::8, :] = 1e30
    env = _env(n, auto_reset=False)
    g = _gpu_step(env, st, acts)
    ref = _oracle_step(O.ENV_HOVER, O.WRAP_NONE, st, acts)
    for i, o in enumerate(ref):
        assert g["terminated"][i] == o["terminated"], i
        assert parity_ok(g["qvel"][i], o["qvel"], st["qvel"][i]), i
        assert parity_ok(g["obs"][i], o["obs"]), i
        assert (np.isnan(g["voltage"][i]) and np.isnan(o["voltage"])) or parity_ok(g["voltage"][i], o["voltage"])
    env.close()


def test_bad_state_and_acceleration_resets(kernel_variant):
    """MuJoCo's mj_checkPos/Vel (NaN/Inf or |x| > 1e10 in qpos/qvel -> mj_resetData) and
    mj_checkAcc, and large-but-good states whose |x| sum exceeds 1e10 (the kernel's screen then
    falls back to per-element tests, which must find nothing bad)."""
    n = 512
    rng = np.random.default_rng(11)
    st = _random_states(n, rng, wide=False)
    st["step_count"][:] = 0
    k = np.arange(n) % 8
    st["qpos"][k == 0, 0] = np.nan
    st["qvel"][k == 1, 1] = 2e10
    st["qpos"][k == 2, 4] = np.inf
    st["qvel"][k == 3, 3:5] = 6e9      # good state, sum > 1e10; angular rate -> bad acceleration
    st["qvel"][k == 4, 6:8] = 6e9      # prop spins: good state, bad acceleration
    st["qvel"][k == 5, 0:2] = 6e9      # linear velocity: good state, bad acceleration (drag)
    st["qpos"][k == 6, 3:5] = 6e9      # unnormalized quaternion: good state, normalized by the step
    acts = rng.uniform(-1, 1, (n, 4)).astype(np.float32)
    env = _env(n, auto_reset=False)
    g = _gpu_step(env, st, acts)
    ref = _oracle_step(O.ENV_HOVER, O.WRAP_NONE, st, acts)
    for i, o in enumerate(ref):
        assert g["terminated"][i] == o["terminated"], i
        # pre-step scale without the NaN / huge entries (they would void or loosen the check)
        pp, pv = (np.where(np.abs(st[f][i]) < 1e9, st[f][i], 0) for f in ("qpos", "qvel"))
        assert parity_ok(g["qpos"][i], o["qpos"], pp), (i, g["qpos"][i], o["qpos"])
        assert parity_ok(g["qvel"][i], o["qvel"], pv), (i, g["qvel"][i], o["qvel"])
        assert parity_ok(g["obs"][i], o["obs"]), i
    # bad states (rows 0-2) and bad accelerations (rows 3-5) really were reset to qpos0: unit
    # quaternion, zero hinge angles, zero angular and prop rates (only gravity acts afterwards)
    for i in np.nonzero(k <= 5)[0]:
        assert np.array_equal(g["qvel"][i][3:], np.zeros(7, np.float32)), i
        assert np.array_equal(g["qpos"][i][3:], np.array([1, 0, 0, 0, 0, 0, 0, 0], np.float32)), i
    env.close()


def test_large_batch_properties():
    """Full-size batch (1,048,576 envs): size-independent properties + a strided oracle sample."""
    n = 1 << 20
    env = _env(n, seed=1)
    env.reset()
    for k in range(3):
        acts = env.random_actions(k)
        pre = env.get_state() if k == 2 else None
        obs, rew, te, tr, inf = env.step(acts, info="full")
    torch.cuda.synchronize()
    assert torch.isfinite(obs).all() and torch.isfinite(rew).all()
    assert ((rew > 0) & (rew <= 1)).all()
    s12 = inf["state"]
    lo = torch.tensor(env.cfg.term_low[:], device="cuda:0")
    hi = torch.tensor(env.cfg.term_high[:], device="cuda:0")
    term_ref = ~(((s12 >= lo) & (s12 <= hi)).all(dim=1))
    assert torch.equal(term_ref, te)
    a = acts.cpu().numpy(); g_obs = inf["terminal_observation"].cpu().numpy()
    o_obs = obs.cpu().numpy(); ten = te.cpu().numpy()
    cfg = O.default_cfg(O.ENV_HOVER, O.WRAP_NONE)
    for i in range(0, n, n // 512):
        e = O.Env(cfg=cfg)
        e.set_full_state(pre["qpos"][i], pre["qvel"][i], pre["voltage"][i], pre["target"][i],
                         pre["step_count"][i])
        o = O.out_to_dict(e.step(a[i]))
        assert o["terminated"] == bool(ten[i])
        assert parity_ok(g_obs[i] if ten[i] else o_obs[i], o["obs"])
    env.close()


def test_gae_matches_sb3_restatement():
    from uav_reinforcement_learning_control_amd.ppo.gae import gae
    T, n = 64, 777
    rng = np.random.default_rng(0)
    rew = rng.normal(size=(T, n)).astype(np.float32)
    val = rng.normal(size=(T, n)).astype(np.float32)
    starts = (rng.uniform(size=(T, n)) < 0.1).astype(np.float32)
    last = rng.normal(size=n).astype(np.float32)
    dones = (rng.uniform(size=n) < 0.1).astype(np.float32)
    gamma, lam = 0.9906345854291289, 0.9079441765099094
    adv_ref = np.zeros((T, n), np.float64)
    last_gae = 0
    for t in reversed(range(T)):  # SB3 RolloutBuffer.compute_returns_and_advantage
        if t == T - 1:
            nnt = 1.0 - dones; nv = last
        else:
            nnt = 1.0 - starts[t + 1]; nv = val[t + 1]
        delta = rew[t] + gamma * nv * nnt - val[t]
        last_gae = delta + gamma * lam * nnt * last_gae
        adv_ref[t] = last_gae
    c = lambda x: torch.from_numpy(x).cuda()
    adv, ret = gae(c(rew), c(val), c(starts), c(last), c(dones), gamma, lam)
    np.testing.assert_allclose(adv.cpu().numpy(), adv_ref, rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(ret.cpu().numpy(), adv_ref + val, rtol=1e-4, atol=1e-4)


def test_step_range_touches_only_its_rows(kernel_variant):
    """quad_step_range(first, count): rows outside the range are neither read nor written, and the
    two halves stepped separately equal one full step."""
    import ctypes as C
    from uav_reinforcement_learning_control_amd import _native as N
    n = 3000
    a = _env(n, seed=4)
    b = _env(n, seed=4)
    a.reset(); b.reset()
    acts = a.random_actions(0)
    oa, ra, ta, ua, _ = a.step(acts)
    oa, ra, ta, ua = oa.clone(), ra.clone(), ta.clone(), ua.clone()
    sentinel = torch.full((n, 12), 7.0, device="cuda:0")
    b.obs.copy_(sentinel)
    out = N.QuadStepOut(obs=b.obs.data_ptr(), reward=b.reward.data_ptr(),
                        terminated=b.terminated.data_ptr(), truncated=b.truncated.data_ptr(),
                        terminal_obs=b.terminal_obs.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    N.check(N.lib().quad_step_range(b._h, 0, 1234, C.c_void_p(acts.data_ptr()), C.byref(out), s), "r")
    torch.cuda.synchronize()
    assert torch.equal(b.obs[1234:], sentinel[1234:])
    N.check(N.lib().quad_step_range(b._h, 1234, n - 1234, C.c_void_p(acts.data_ptr()), C.byref(out), s), "r")
    torch.cuda.synchronize()
    assert torch.equal(b.obs, oa) and torch.equal(b.reward, ra)
    assert torch.equal(b.terminated, ta) and torch.equal(b.truncated, ua)
    sa, sb = a.get_state(), b.get_state()
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    assert N.lib().quad_step_range(b._h, n - 1, 2, C.c_void_p(acts.data_ptr()), C.byref(out), s) == N.QUAD_EINVAL
    a.close(); b.close()


@pytest.mark.parametrize("env_name", ["hover", "trajectory"])
def test_relpos_wrapper_is_base_obs_plus_prev_action(env_name):
    """RelPosActWrapper (envs/wrappers.py:13-25): obs7 = [obs12[0:3], _prev_action]. Each step
    starts both envs from the same state (re-synced), so the rel-pos part matches the unwrapped
    env's to the parity bar (separately compiled kernels may differ by an ulp) and the flags
    exactly; the previous action is the action just taken and zeros after a reset; observe and
    get_state agree."""
    n, T = 2048, 30
    base = _env(n, env_name, None, seed=11, max_episode_steps=12)
    rel = _env(n, env_name, "RelPosActWrapper", seed=11, max_episode_steps=12)
    o12, o7 = base.reset(), rel.reset()
    assert o7.shape == (n, 7) and torch.equal(o7[:, :3], o12[:, :3]) and torch.all(o7[:, 3:] == 0)
    for t in range(T):
        st = base.get_state()
        st.pop("prev_action")
        rel.set_state(**st)
        a = base.random_actions(t)
        o12, r12, te12, tr12, i12 = base.step(a)
        o7, r7, te7, tr7, i7 = rel.step(a)
        done = te12 | tr12
        assert torch.equal(te7, te12) and torch.equal(tr7, tr12)
        assert parity_ok(r7.cpu().numpy()[:, None], r12.cpu().numpy()[:, None]).all()
        assert parity_ok(o7[:, :3].cpu().numpy(), o12[:, :3].cpu().numpy()).all()
        assert torch.equal(o7[~done, 3:], a[~done]) and torch.all(o7[done, 3:] == 0)
        tob7, tob12 = i7["terminal_observation"], i12["terminal_observation"]
        assert parity_ok(tob7[done, :3].cpu().numpy(), tob12[done, :3].cpu().numpy()).all()
        assert torch.equal(tob7[done, 3:], a[done])
    assert torch.equal(rel.observe(torch.empty(n, 7, device="cuda")), o7)
    g = rel.get_state()
    assert np.array_equal(g["prev_action"], o7[:, 3:].cpu().numpy())


def _spline_ref(seed, gid, episode, start, step, L=2048, dur=30.0):
    """TrajectoryFollowEnv._sample_sinusoid_trajectory restated with scipy at the reference's spline
    constants (cfg_cases.spline_ref)."""
    from cfg_cases import spline_ref
    return spline_ref(seed, gid, episode, start, step, L=L, dur=dur)


def test_trajectory_info_spline_matches_scipy():
    """info["target" / "target_vel" / "target_acc"] of TrajectoryFollowEnv
    (trajectory_follow_env.py:163-168, :175-243) vs scipy's natural CubicSpline on the same draws."""
    n, seed = 512, 21
    env = _env(n, "trajectory", None, seed=seed, max_episode_steps=40)
    env.reset()
    starts = env.get_state()["target"].copy()      # traj_pos[0] = start position
    eps = env.get_state()["episode"].copy()
    for t in range(1, 46):
        a = env.random_actions(t)
        steps = env.get_state()["step_count"] + 1   # the step being taken, per env
        _, _, te, tr, inf = env.step(a, info="full")
        ti = torch.cat([inf["target"], inf["target_vel"], inf["target_acc"]], 1).cpu().numpy()
        for i in range(0, n, 37):
            ref = _spline_ref(seed, i, int(eps[i]) - 1, starts[i], int(steps[i]), L=40)
            np.testing.assert_allclose(ti[i], ref, rtol=1e-6, atol=2e-6)
        done = (te | tr).cpu().numpy()
        if done.any():  # new episodes: new start position and draw counter
            g = env.get_state()
            starts[done] = g["target"][done]
            eps[done] = g["episode"][done]
        if t == 1:
            np.testing.assert_allclose(ti[:, :3], starts, atol=1e-6)  # the spline starts at the start


@pytest.mark.parametrize("n", [1, 255, 257, 4097])
def test_ragged_sizes_match_oracle(n, kernel_variant):
    """Batch sizes that are not a multiple of the 256-thread block (and a single env) step every
    env exactly once, in every kernel form; rows past N are never touched."""
    rng = np.random.default_rng(n)
    st = _random_states(n, rng)
    acts = rng.uniform(-1, 1, (n, 4)).astype(np.float32)
    env = _env(n, "hover", "RateControlWrapper", auto_reset=False)
    env.set_state(**st)
    a = torch.from_numpy(acts).cuda()
    obs = torch.full((n + 7, 12), 7.0, device="cuda")  # sentinel rows after the batch
    env.step(a, obs=obs[:n])
    torch.cuda.synchronize()
    assert torch.all(obs[n:] == 7.0)
    ref = _oracle_step(O.ENV_HOVER, O.WRAP_CTBR, st, acts)
    got = obs[:n].cpu().numpy()
    assert all(parity_ok(got[i], ref[i]["obs"]) for i in range(n))
    env.close()


@pytest.mark.parametrize("n", [1000, 4096 + 37])
def test_ragged_mass_auto_reset_draws(n, kernel_variant):
    """Every env truncates at once (max_episode_steps = 1) in a batch whose last wave is partly
    empty: k_step_h's helper waves draw every env's next-reset row, and the lanes past N shadow the
    last env (in-range loads, no stores). Each reset obs equals the oracle's draw."""
    env = _env(n, seed=31, env_id_base=77, max_episode_steps=1)
    env.reset()
    cfg = O.default_cfg(O.ENV_HOVER, O.WRAP_NONE)
    for k in range(2):
        pre = env.get_state()
        obs, rew, te, tr, inf = env.step(torch.zeros(n, 4, device="cuda"))
        torch.cuda.synchronize()
        assert bool(tr.all())
        obs = obs.cpu().numpy()
        for i in list(range(0, n, 97)) + list(range(n - 70, n)):
            i12, t3 = O.reset_draw(cfg, 31, 77 + i, int(pre["episode"][i]))
            assert np.array_equal(obs[i], O.Env(cfg=cfg).reset_with(i12, t3)), (k, i)
    env.close()


def test_four_million_envs_properties():
    """A 4,194,304-env batch (index arithmetic far past 2^16 blocks): every row finite, rewards in
    (0, 1], flags consistent with the state bounds, a strided oracle sample exact."""
    n = 1 << 22
    env = _env(n, seed=5)
    env.reset()
    acts = env.random_actions(0)
    pre = env.get_state()
    obs, rew, te, tr, inf = env.step(acts, info="full")
    torch.cuda.synchronize()
    assert torch.isfinite(obs).all() and ((rew > 0) & (rew <= 1)).all()
    s12 = inf["state"]
    lo = torch.tensor(env.cfg.term_low[:], device="cuda:0")
    hi = torch.tensor(env.cfg.term_high[:], device="cuda:0")
    assert torch.equal(~(((s12 >= lo) & (s12 <= hi)).all(dim=1)), te)
    a = acts.cpu().numpy(); o_obs = obs.cpu().numpy(); tob = inf["terminal_observation"].cpu().numpy()
    ten = te.cpu().numpy()
    cfg = O.default_cfg(O.ENV_HOVER, O.WRAP_NONE)
    for i in list(range(0, n, n // 256)) + [n - 1]:
        e = O.Env(cfg=cfg)
        e.set_full_state(pre["qpos"][i], pre["qvel"][i], pre["voltage"][i], pre["target"][i],
                         pre["step_count"][i])
        o = O.out_to_dict(e.step(a[i]))
        assert o["terminated"] == bool(ten[i])
        assert parity_ok(tob[i] if ten[i] else o_obs[i], o["obs"])
    env.close()


def test_invalid_arguments_fail_cleanly():
    import ctypes as C
    from uav_reinforcement_learning_control_amd import _native as N
    L = N.lib()
    cfg = N.default_cfg()
    h = C.c_void_p()
    for n in (0, -5, 1 << 30):
        assert L.quad_create(C.byref(cfg), 0, 0, 0, n, C.byref(h)) == N.QUAD_EINVAL and not h.value
    bad = N.default_cfg()
    bad.max_episode_steps = 0
    assert L.quad_create(C.byref(bad), 0, 0, 0, 16, C.byref(h)) == N.QUAD_EINVAL
    assert L.quad_create(C.byref(cfg), 99, 0, 0, 16, C.byref(h)) == N.QUAD_EINVAL
    env = _env(64)
    a = torch.zeros(64, 4, device="cuda")
    out = N.QuadStepOut(obs=None, reward=env.reward.data_ptr(), terminated=env.terminated.data_ptr(),
                        truncated=env.truncated.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.quad_step(env._h, C.c_void_p(a.data_ptr()), C.byref(out), s) == N.QUAD_EINVAL
    out.obs = env.obs.data_ptr()
    assert L.quad_step_range(env._h, 60, 8, C.c_void_p(a.data_ptr()), C.byref(out), s) == N.QUAD_EINVAL
    assert L.quad_step(env._h, C.c_void_p(a.data_ptr() + 4), C.byref(out), s) == N.QUAD_EINVAL
    assert b"aligned" in L.quad_last_error()
    assert L.quad_step(env._h, C.c_void_p(a.data_ptr()), C.byref(out), s) == N.QUAD_OK
    env.close()


@pytest.mark.parametrize("env_name,wrapper", [("hover", None), ("trajectory", "RateControlWrapper")])
@pytest.mark.parametrize("helper", ["1", "1w"])
def test_step_random_is_the_step_by_step_rollout(env_name, wrapper, spec_mode, helper, monkeypatch):
    # k_step_random_h ("1w": its 256-env blocks of > 32,768-env batches)
    if helper.endswith("w"):
        monkeypatch.setenv("QUADENV_HBLOCK", "256")
    else:
        monkeypatch.delenv("QUADENV_HBLOCK", raising=False)
    """quad_step_random (config 2 in one launch, state on chip) == random_actions + quad_step
    step by step, bit for bit: every step's obs, reward, flags, terminal obs, the actions, and the
    final state (incl. episode counters after the auto-resets it crossed)."""
    n, T = 5000, 40
    ms = 13 if spec_mode == "0" else None  # the default episode length keeps the SPEC kernels
    a = _env(n, env_name, wrapper, seed=21, env_id_base=77, max_episode_steps=ms)
    b = _env(n, env_name, wrapper, seed=21, env_id_base=77, max_episode_steps=ms)
    a.reset(); b.reset()
    res = a.step_random(T, step0=5, actions=True)
    resets = 0
    for t in range(T):
        acts = b.random_actions(5 + t)
        obs, rew, te, tr, inf = b.step(acts)
        done = te | tr
        resets += int(done.sum())
        assert torch.equal(res["actions"][t], acts), t
        assert torch.equal(res["obs"][t], obs) and torch.equal(res["reward"][t], rew), t
        assert torch.equal(res["terminated"][t], te) and torch.equal(res["truncated"][t], tr), t
        assert torch.equal(res["terminal_observation"][t][done], inf["terminal_observation"][done]), t
    assert resets > (n if ms else n // 10)  # (13-step episodes: every env resets at least twice)
    ga, gb = a.get_state(), b.get_state()
    for k in ga:
        assert np.array_equal(ga[k], gb[k]), k
    a.close(); b.close()


def test_step_random_against_oracle_short_horizon():
    """The K-step launch against the float64 oracle from the same start states: every step's obs
    within the parity bar for 3 steps (one-step errors compound after that), and the reset obs of
    any env that finishes bit-exact with the oracle's draw of that episode."""
    n, T = 512, 3
    env = _env(n, "hover", seed=8, max_episode_steps=2)
    env.reset()
    st = env.get_state()
    res = env.step_random(T, step0=0)
    cfg = O.default_cfg(O.ENV_HOVER, O.WRAP_NONE)
    cfg.max_episode_steps = 2
    obs = res["obs"].cpu().numpy(); te = res["terminated"].cpu().numpy(); tr = res["truncated"].cpu().numpy()
    for i in range(0, n, 5):
        e = O.Env(cfg=cfg)
        e.set_full_state(st["qpos"][i], st["qvel"][i], st["voltage"][i], st["target"][i], st["step_count"][i])
        ep = st["episode"][i]
        for t in range(T):
            o = O.out_to_dict(e.step(O.random_action(8, i, t)))
            assert o["terminated"] == te[t, i] and o["truncated"] == tr[t, i], (i, t)
            if o["terminated"] or o["truncated"]:
                i12, t3 = O.reset_draw(cfg, 8, i, ep)
                ep += 1
                assert np.array_equal(obs[t, i], e.reset_with(i12, t3)), (i, t)
            else:
                assert parity_ok(obs[t, i], o["obs"]).all(), (i, t, obs[t, i], o["obs"])
    env.close()
