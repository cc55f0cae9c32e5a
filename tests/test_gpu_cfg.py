"""GPU: every QuadCfg field, in every kernel family, against the float64 oracle at the same configuration.

A handle whose configuration differs from the reference defaults runs the generic kernels, which read
the handle's KConsts block (quad_create takes the SPEC kernels only for a byte-identical block). The
rest of the suite runs those kernels at the default values, where a kernel that read a compiled-in
constant instead of its KConsts word would go unnoticed. Here (tests/cfg_cases.py holds the cases, and
tests/test_cfg_cases_cpu.py shows on the oracle that each moves its outputs on >= 25 % of the rows):

a. one field at a time: quad_step / quad_reset / info's spline against the oracle (scipy for the spline);
b. alt_cfg (every field moved at once) through the five step forms, the mass auto-reset, quad_reset,
   quad_observe, quad_terminated at +-1 ulp of the bounds, the info spline and quad_deploy_obs;
c. edges: max_motor_thrust above the model's ctrlrange and at zero, no voltage sag, min == nominal
   voltage, a rate loop without its integrator, a small time step, and a refused horizontal gravity;
d. the brax kinds, field by field and at their alt_cfg;
e. every fused family against its per-step loop on alt_cfg handles: the families' own bit-for-bit tests,
   at their smallest shapes, run with every QuadVecEnv they build carrying alt_cfg (alt_handles);
f. the control laws' plant (make_pid_plant): pid_act / ctrl_act against pid_ref / ctrl_ref with
   plant_of(cfg), at alt_cfg and one plant constant at a time.

The bar is DESIGN.md's "Parity" bar, unchanged (tests/test_gpu_parity.py): obs / reward / voltage /
motor commands |d| <= 1e-5 |ref| + 1e-6; qpos / qvel / state12 relative to max(|ref|, |pre-step|); the
Euler columns in parts (euler_ok); flags, counters and reset draws exact.
"""
import contextlib
import ctypes as C
import dataclasses
import inspect
import os

import numpy as np
import pytest
import torch

import cfg_cases as CC
import ctrl_ref
import deploy_ref
import pid_ref
from oracle import oracle as O
from test_gpu_brax import _close, _resynced_rollout
from test_gpu_parity import (_gpu_step, euler_of_quat, kernel_variant, obs_euler_of_quat, operand_only,  # noqa: F401
                             parity_ok)  # (kernel_variant: the fixture that pins the five step forms)
from test_gpu_parity_full import _check_rows
import test_gpu_actor_arch as TA
import test_gpu_brax_actor as TBA
import test_gpu_brax_unroll as TBU
import test_gpu_ctrl as TC
import test_gpu_parity as TP
import test_gpu_pid as TPID
import test_gpu_policy_episode as PE
import test_gpu_population_ppo as TPP
import test_gpu_rollout as TR
import test_gpu_waypoints as TW
from uav_reinforcement_learning_control_amd import _native as N
from uav_reinforcement_learning_control_amd import controllers as ctl
from uav_reinforcement_learning_control_amd.envs import QuadVecEnv

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEED, BASE = 0xC0FFEE, 1 << 20
N_FIELD, N_ALT = 260, 520  # four / eight 64-env blocks and a ragged one (two 256-env blocks and a ragged one)
ACT_TOL, STATE_TOL, DIAG_TOL = 2.0 ** -23, 1e-12, 1e-9  # tests/test_gpu_pid.py, tests/test_gpu_ctrl.py

_id = lambda k, w: f"{CC.ENV_NAME[k]}-{CC.WRAPPER_NAME[w]}"
_relpos = lambda w: w in (CC.RELPOS, CC.CTBR_RELPOS)


def _env(kind, wrap, n, overrides=None, **kw):
    return QuadVecEnv(n, env=CC.ENV_NAME[kind], wrapper=CC.WRAPPER_NAME[wrap], device=DEV, cfg_overrides=overrides, **kw)


def _generic(env):
    """A handle that differs from the defaults in a field its kernels read must not take a SPEC kernel."""
    assert N.lib().quad_kernel_form(env._h) & 16 == 0


def _bounds(q):
    return np.array(q.obs_low[:], np.float32), np.array(q.obs_high[:], np.float32)


def _compare_step(g, ref, st, acts, q, rows=None, what=None):
    """Every output test_step_matches_oracle_random_states compares, on `rows` (all by default), with the
    Euler helpers at the handle's own observation bounds; under a RELPOS wrapper the 7-D row instead
    of the 12-D one (its first three columns at the bar, the action copied exactly)."""
    n = len(acts)
    rows = np.arange(n) if rows is None else rows
    g = dict(g, motor_commands=g["motor"])
    what = what or ("obs", "reward", "voltage", "motor_commands", "qpos", "qvel", "state12", "rate_int")
    if _relpos(q.wrapper):
        what = tuple(k for k in what if k != "obs")
    bad = _check_rows(g, ref, st, rows, what, obs_bounds=_bounds(q))
    assert len(bad) == 0, (len(bad), bad[:8])
    assert parity_ok(g["vscale"][rows, None], ref["voltage_scale"][rows, None]).all()
    for k in ("qpos", "qvel"):  # operand-relative slack only on near-cancelling updates
        cnt, outside = operand_only(g[k][rows], ref[k][rows], st[k][rows])
        assert len(outside) == 0, (k, outside[:5])


def _relpos_rows(obs7, ref, acts, rows):
    assert parity_ok(obs7[rows, :3], ref["obs7"][rows, :3]).all()
    assert np.array_equal(obs7[rows, 3:], acts[rows])  # the action just taken, copied exactly


def _one_step(kind, wrap, overrides, n=N_FIELD, states_cfg=None, seed=None):
    """One quad_step (auto_reset off) of random states against the oracle; returns (g, ref, st, acts)."""
    env = _env(kind, wrap, n, overrides, seed=SEED, env_id_base=BASE, auto_reset=False)
    _generic(env)
    q = env.cfg
    st, acts = CC.step_inputs(kind, wrap, n, cfg=states_cfg, seed=seed)
    g = _gpu_step(env, st, acts)
    ref = O.step_batch(CC.oracle_cfg_of(q), st, acts)
    _compare_step(g, ref, st, acts, q)
    assert np.array_equal(g["step_count"], st["step_count"] + 1)
    if _relpos(wrap):
        assert g["obs"].shape == (n, 7)
        _relpos_rows(g["obs"], ref, acts, np.arange(n))
        assert np.array_equal(g["prev_action"], acts)
    env.close()
    return g, ref, st, acts


# ---------------------------------------------------------------------------------------------
# a. one field at a time
STEP_FIELDS = [(name, k, w) for name, c in CC.FIELD_CASES.items() for k, w in c.applies
               if not CC.is_brax(k) and not ({"reset", "target_info"} & set(c.outputs))]
RESET_FIELDS = [(name, k, w) for name, c in CC.FIELD_CASES.items() for k, w in c.applies
                if not CC.is_brax(k) and "reset" in c.outputs]
SPLINE_FIELDS = [(name, k, w) for name, c in CC.FIELD_CASES.items() for k, w in c.applies if "target_info" in c.outputs]
BRAX_FIELDS = [(name, k) for name, c in CC.FIELD_CASES.items() for k, w in c.applies if CC.is_brax(k)]


@pytest.mark.parametrize("name,kind,wrap", STEP_FIELDS, ids=[f"{n}-{_id(k, w)}" for n, k, w in STEP_FIELDS])
def test_field_step_matches_oracle(name, kind, wrap):
    """quad_step on a handle that differs from the default in `name` alone, from the inputs on which
    test_cfg_cases_cpu shows the field's teeth, against the oracle at that configuration."""
    case = CC.FIELD_CASES[name]
    g, ref, st, acts = _one_step(kind, wrap, case.overrides(name, kind, wrap))
    if "terminated" in case.outputs or "truncated" in case.outputs:  # both values of the flag occur
        for k in set(case.outputs) & {"terminated", "truncated"}:
            assert 0.1 < ref[k].mean() < 0.98, (k, ref[k].mean())


def _check_reset(env, kind, n, episodes=(0, 1)):
    """quad_reset: observation and state bit-exact with the oracle's draw of each episode counter."""
    oc = CC.oracle_cfg_of(env.cfg)
    gids = BASE + np.arange(n, dtype=np.uint64)
    for ep in episodes:
        obs = env.reset().cpu().numpy()
        eps = np.full(n, ep, np.uint32)
        ref = O.reset_obs_batch(oc, SEED, gids, eps)
        if obs.shape[1] == 7:
            assert np.array_equal(obs[:, :3].view(np.uint32), ref[:, :3].view(np.uint32)) and not obs[:, 3:].any()
        else:
            assert np.array_equal(obs.view(np.uint32), ref.view(np.uint32)), int(np.any(obs != ref, axis=1).sum())
        i12, t3 = O.reset_draw_batch(oc, SEED, gids, eps)
        s = env.get_state()
        assert np.array_equal(s["qpos"][:, :3], i12[:, :3]) and np.array_equal(s["qvel"][:, :6], i12[:, 6:])
        assert np.array_equal(s["target"], i12[:, :3] if kind == CC.TRAJ else t3)
        assert np.all(s["voltage"] == np.float32(env.cfg.nominal_voltage))
        assert np.all(s["step_count"] == 0) and np.all(s["episode"] == ep + 1)


@pytest.mark.parametrize("name,kind,wrap", RESET_FIELDS, ids=[f"{n}-{_id(k, w)}" for n, k, w in RESET_FIELDS])
def test_field_reset_matches_oracle(name, kind, wrap):
    env = _env(kind, wrap, N_FIELD, CC.FIELD_CASES[name].overrides(name, kind, wrap), seed=SEED, env_id_base=BASE)
    _generic(env)
    _check_reset(env, kind, N_FIELD)
    env.close()


def _check_spline(env, seed, steps, stride):
    """step(info="full")'s target / target_vel / target_acc against scipy's natural cubic spline at the
    handle's spline_* constants and episode length (test_trajectory_info_spline_matches_scipy's check)."""
    n, q = env.num_envs, env.cfg
    starts = env.get_state()["target"].copy()      # traj_pos[0] = start position
    eps = env.get_state()["episode"].copy()
    crossed = 0
    for t in range(1, steps + 1):
        a = env.random_actions(t)
        cnt = env.get_state()["step_count"] + 1     # the step being taken, per env
        _, _, te, tr, inf = env.step(a, info="full")
        ti = torch.cat([inf["target"], inf["target_vel"], inf["target_acc"]], 1).cpu().numpy()
        for i in range(0, n, stride):
            ref = CC.spline_ref_cfg(q, seed, i, int(eps[i]) - 1, starts[i], int(cnt[i]))
            np.testing.assert_allclose(ti[i], ref, rtol=1e-6, atol=2e-6)
        done = (te | tr).cpu().numpy()
        crossed += int(done[::stride].sum())
        if done.any():  # new episodes: new start position and draw counter
            g = env.get_state()
            starts[done] = g["target"][done]
            eps[done] = g["episode"][done]
    assert crossed > 0  # second episodes were sampled too


@pytest.mark.parametrize("name,kind,wrap", SPLINE_FIELDS, ids=[f"{n}-{_id(k, w)}" for n, k, w in SPLINE_FIELDS])
def test_field_spline_matches_scipy(name, kind, wrap):
    ov = dict(CC.FIELD_CASES[name].overrides(name, kind, wrap), max_episode_steps=20)
    env = _env(kind, wrap, 130, ov, seed=21)
    env.reset()
    _check_spline(env, 21, 24, 13)
    env.close()


# ---------------------------------------------------------------------------------------------
# b. alt_cfg through every step form
@pytest.mark.parametrize("kind,wrap", CC.STEP4, ids=[_id(k, w) for k, w in CC.STEP4])
def test_alt_step_and_mass_auto_reset_match_oracle(kind, wrap, kernel_variant):
    alt = CC.alt_cfg(kind, wrap)
    n = N_ALT
    # one step, auto_reset off: every output
    env = _env(kind, wrap, n, alt, seed=SEED, env_id_base=BASE, auto_reset=False)
    form = N.lib().quad_kernel_form(env._h)
    assert form & 16 == 0 and bool(form & 128) == ("w" in kernel_variant) and bool(form & 512) == kernel_variant.endswith("d")
    q = env.cfg
    oc = CC.oracle_cfg_of(q)
    st, acts = CC.step_inputs(kind, wrap, n, cfg=q, seed=900 + 7 * kind + wrap)
    st["episode"] = np.random.default_rng(5).integers(0, 1 << 20, n).astype(np.uint32)
    g = _gpu_step(env, st, acts)
    ref = O.step_batch(oc, st, acts)
    _compare_step(g, ref, st, acts, q)
    assert np.array_equal(g["step_count"], st["step_count"] + 1) and np.array_equal(g["episode"], st["episode"])
    env.close()
    # the same step with auto_reset on: the shrunken bounds and the 137-step limit finish many envs
    env = _env(kind, wrap, n, alt, seed=SEED, env_id_base=BASE, auto_reset=True)
    g = _gpu_step(env, st, acts)
    done = g["terminated"] | g["truncated"]
    dr, nr = np.nonzero(done)[0], np.nonzero(~done)[0]
    assert len(dr) > n // 4 and len(nr) > n // 8 and ref["terminated"].sum() > n // 8 and ref["truncated"].sum() > n // 8
    assert np.array_equal(g["terminated"], ref["terminated"]) and np.array_equal(g["truncated"], ref["truncated"])
    _compare_step(g, ref, st, acts, q, rows=nr, what=("obs", "reward", "voltage", "qpos", "qvel", "rate_int"))
    assert np.array_equal(g["step_count"][nr], st["step_count"][nr] + 1)
    assert np.array_equal(g["episode"][nr], st["episode"][nr])
    # finished envs: the step's reward and terminal observation, then the redrawn state and its observation
    assert parity_ok(g["term_obs"][dr], ref["obs"][dr]).all()
    assert parity_ok(g["reward"][dr, None], ref["reward"][dr, None]).all()
    gids = BASE + dr.astype(np.uint64)
    reset_obs = O.reset_obs_batch(oc, SEED, gids, st["episode"][dr])
    assert np.array_equal(g["obs"][dr].view(np.uint32), reset_obs.view(np.uint32)), \
        int(np.sum(np.any(g["obs"][dr] != reset_obs, axis=1)))
    i12, t3 = O.reset_draw_batch(oc, SEED, gids, st["episode"][dr])
    assert np.array_equal(g["qpos"][dr, :3], i12[:, :3]) and np.array_equal(g["qvel"][dr, :6], i12[:, 6:])
    assert np.all(g["qpos"][dr, 7:] == 0) and np.all(g["qvel"][dr, 6:] == 0)
    assert np.array_equal(g["target"][dr], i12[:, :3] if kind == CC.TRAJ else t3)
    assert np.all(g["voltage"][dr] == np.float32(q.nominal_voltage))
    assert np.all(g["step_count"][dr] == 0) and np.array_equal(g["episode"][dr], st["episode"][dr] + 1)
    if wrap == CC.CTBR:
        assert np.all(g["rate_int"][dr] == 0)
    env.close()


@pytest.mark.parametrize("kind,wrap", CC.STEP6, ids=[_id(k, w) for k, w in CC.STEP6])
def test_alt_reset_observe_and_terminated(kind, wrap):
    """quad_reset (bit-exact draws at the alt init_* / target_* / nominal voltage), quad_observe of given
    states against the oracle's _get_obs at the alt observation bounds, and quad_terminated at the alt
    bounds and one ulp to either side of each."""
    n = N_FIELD
    env = _env(kind, wrap, n, CC.alt_cfg(kind, wrap), seed=SEED, env_id_base=BASE)
    _generic(env)
    q = env.cfg
    _check_reset(env, kind, n)
    st, _ = CC.step_inputs(kind, wrap, n, cfg=q, seed=77)
    env.set_state(**st)
    obs, s12 = env.observe(state=True)
    obs, s12 = obs.cpu().numpy(), s12.cpu().numpy()
    oc = CC.oracle_cfg_of(q)
    ref_obs, ref_s12 = np.zeros((n, 12), np.float32), np.zeros((n, 12), np.float32)
    for i in range(n):
        e = O.Env(cfg=oc)
        e.set_full_state(st["qpos"][i], st["qvel"][i], st["voltage"][i], st["target"][i], st["step_count"][i])
        O.lib().oracle_get_obs(C.byref(oc), C.byref(e.s), ref_obs[i].ctypes.data_as(C.POINTER(C.c_float)))
        ref_s12[i] = e.s.state12[:]
    ne = [0, 1, 2, 6, 7, 8, 9, 10, 11]
    assert np.array_equal(s12[:, ne], ref_s12[:, ne])  # positions and rates are copies of the state
    assert parity_ok(s12[:, 3:6], euler_of_quat(st["qpos"])).all()  # (the Euler columns: see euler_ok)
    if _relpos(wrap):
        assert parity_ok(obs[:, :3], ref_obs[:, :3]).all() and np.array_equal(obs[:, 3:], st["prev_action"])
    else:
        assert parity_ok(obs[:, ne], ref_obs[:, ne]).all()
        assert parity_ok(obs[:, 3:6], obs_euler_of_quat(st["qpos"], _bounds(q))).all()
    # the termination predicate on each bound, just inside and just outside it
    lo, hi = np.array(q.term_low[:], np.float32), np.array(q.term_high[:], np.float32)
    mid = ((lo.astype(np.float64) + hi) / 2).astype(np.float32)
    rows, want = [mid.copy()], [False]
    for j in range(12):
        for b, out in ((lo[j], np.float32(-np.inf)), (hi[j], np.float32(np.inf))):
            for v, t in ((b, False), (np.nextafter(b, -out), False), (np.nextafter(b, out), True)):
                s = mid.copy()
                s[j] = v
                rows.append(s); want.append(t)
    got = env.is_terminated(torch.from_numpy(np.stack(rows)).to(DEV)).cpu().numpy()
    assert np.array_equal(got, np.array(want)), np.nonzero(got != np.array(want))[0]
    env.close()


@pytest.mark.parametrize("wrap", [CC.NONE, CC.CTBR], ids=["None", "ctbr"])
def test_alt_spline_matches_scipy(wrap):
    """The info spline at the alt spline_* constants and the alt episode length (137 samples on the alt
    duration); half of the envs start 25 steps before the time limit, so second episodes are sampled."""
    n, seed = 130, 21
    env = _env(CC.TRAJ, wrap, n, CC.alt_cfg(CC.TRAJ, wrap), seed=seed)
    env.reset()
    step = np.zeros(n, np.int32)
    step[::2] = CC.ALT_MAX_EPISODE_STEPS - 25
    env.set_state(step_count=step)
    _check_spline(env, seed, 40, 7)
    env.close()


DEPLOY_CASES = {"alt": lambda: CC.alt_cfg(CC.HOVER, CC.NONE),
                "obs_low": lambda: CC.FIELD_CASES["obs_low"].overrides("obs_low", CC.HOVER, CC.NONE),
                "obs_high": lambda: CC.FIELD_CASES["obs_high"].overrides("obs_high", CC.HOVER, CC.NONE)}


@pytest.mark.parametrize("case", list(DEPLOY_CASES))
def test_deploy_obs_at_other_spans_equals_the_ref_bitwise(case):
    """quad_deploy_obs normalises through div_const (a reciprocal with Markstein's correction), verified
    exhaustively for the five default spans only: at other spans the rows must still carry the bits of
    deploy_ref.build_obs's true float32 division. The velocity reaches the builder through the estimator's
    state block (alpha = 1 keeps it), as in test_deploy_obs_matches_the_fixture_and_the_ref."""
    n = N_ALT
    env = _env(CC.HOVER, CC.NONE, 8, DEPLOY_CASES[case](), auto_reset=False)  # the handle supplies the bounds
    low, high = _bounds(env.cfg)
    rng = np.random.default_rng(12)
    span = (high - low).astype(np.float64)
    s = rng.uniform(low - 0.1 * span, high + 0.1 * span, (n, 12)).astype(np.float32)  # some rows clip
    s[::7, 3:6] = 0.0
    tgt = rng.uniform(-1.5, 1.5, (n, 3)).astype(np.float32)
    vel = rng.uniform(low[6:9] * 1.1, high[6:9] * 1.1, (n, 3))
    blk = np.zeros((8, n))
    blk[0:3], blk[3], blk[4:7], blk[7] = s[:, 0:3].T, 1.0, vel.T, 1.0
    est = torch.from_numpy(blk).to(DEV)
    obs = env.deploy_obs(torch.from_numpy(s).to(DEV), torch.from_numpy(tgt).to(DEV), 1.01, est, alpha_all=1.0).cpu().numpy()
    want = np.stack([deploy_ref.build_obs(s[i, 0:3], tgt[i], s[i, 3:6], vel[i], s[i, 9:12], low=low, high=high)
                     for i in range(n)])
    assert np.array_equal(obs.view(np.uint32), want.view(np.uint32)), np.argwhere(obs != want)[:8]
    assert (np.abs(want) == 1).any() and (np.abs(want) < 1).mean() > 0.7  # the clip and the interior both occur
    env.close()


# ---------------------------------------------------------------------------------------------
# c. edges, one handle each
EDGES = {
    # above the model's ctrlrange (drone.xml:9, 13 N): the reported motor commands reach 16 N, the physics
    # clamps each at 13 N (physics_step's F_NONNEG clamp, idle at the default)
    "thrust_above_ctrlrange": (CC.STEP4, dict(max_motor_thrust=16.0)),
    "thrust_zero": (CC.STEP4, dict(max_motor_thrust=0.0)),
    "no_voltage_sag": (CC.STEP4, dict(vdrop_base=0.0, vdrop_load=0.0)),
    "min_voltage_is_nominal": (CC.STEP4, None),
    "rate_ki_zero": (CC.RATE3, dict(rate_ki=0.0)),
    "rate_imax_zero": (CC.RATE3, dict(rate_imax=0.0)),
    "timestep_2ms": (CC.STEP4, dict(timestep=0.002)),
}
EDGE_PARAMS = [(e, k, w) for e, (pairs, _) in EDGES.items() for k, w in pairs]


@pytest.mark.parametrize("edge,kind,wrap", EDGE_PARAMS, ids=[f"{e}-{_id(k, w)}" for e, k, w in EDGE_PARAMS])
def test_edge_step_matches_oracle(edge, kind, wrap):
    ov = EDGES[edge][1]
    if ov is None:
        ov = dict(min_voltage=float(CC.default_cfg(kind, wrap).nominal_voltage))
    g, ref, st, acts = _one_step(kind, wrap, ov)
    if edge == "thrust_above_ctrlrange":
        over = (ref["motor_commands"] > 13.0).any(axis=1)
        assert over.sum() >= 20 and ref["motor_commands"].max() > 15.0
        # the clamp has teeth: the oracle whose every motor command stays below 13 N (the same actions on a
        # 13 N drone) moves differently on those rows
        ref13 = O.step_batch(CC.oracle_cfg(kind, wrap), st, acts)
        assert CC.moved(ref["qvel"][over], ref13["qvel"][over]).mean() > 0.5
    elif edge == "thrust_zero":
        assert not ref["motor_commands"].any() and not g["motor"].any()
    elif edge == "no_voltage_sag":
        inside = (st["voltage"] >= np.float32(7.6 if kind == CC.HOVER else 13.2))
        assert np.array_equal(g["voltage"][inside], st["voltage"][inside])
    elif edge == "min_voltage_is_nominal":
        assert np.all(g["voltage"] == np.float32(CC.default_cfg(kind, wrap).nominal_voltage))
    elif edge == "rate_imax_zero":
        assert not g["rate_int"].any()


def test_horizontal_gravity_is_refused():
    """make_phys_consts supports vertical gravity only: quad_create refuses the handle with QUAD_EMODEL."""
    for k, (gx, gy) in enumerate(((0.3, 0.0), (0.0, -0.2))):
        cfg = CC.quad_cfg(CC.HOVER, CC.NONE, dict(gravity=[gx, gy, -9.81]))
        h = C.c_void_p()
        assert N.lib().quad_create(C.byref(cfg), 0, 0, 0, 64, C.byref(h)) == N.QUAD_EMODEL and not h.value
        assert b"gravity" in N.lib().quad_last_error()
    with pytest.raises(N.QuadError):
        _env(CC.HOVER, CC.NONE, 64, dict(gravity=[0.1, 0.0, -9.81]))


# ---------------------------------------------------------------------------------------------
# d. the brax kinds
def _brax_ok(name, kind, ov):
    env, bad = _resynced_rollout(name, kind, n=128, L=40, steps=12, cfg_overrides=ov)
    assert N.lib().quad_kernel_form(env._h) == 64
    assert bad["flags"] == 0 and bad["obs"] == 0 and bad["reward"] == 0, bad
    return env


@pytest.mark.parametrize("name,kind", BRAX_FIELDS, ids=[f"{n}-{CC.ENV_NAME[k]}" for n, k in BRAX_FIELDS])
def test_brax_field_step_matches_oracle_resynced(name, kind):
    env = _brax_ok(CC.ENV_NAME[kind], kind, CC.FIELD_CASES[name].overrides(name, kind, CC.NONE))
    env.close()


@pytest.mark.parametrize("kind", [CC.BRAX_HOVER, CC.BRAX_TRAJ], ids=["brax_hover", "brax_jax_mjx"])
def test_brax_alt_step_and_reset_match_oracle(kind):
    alt = CC.alt_cfg(kind)
    env = _brax_ok(CC.ENV_NAME[kind], kind, alt)
    # reset draws at the alt reset_noise (seed 3 is _resynced_rollout's; a reset advances the episode counter)
    ep = env.get_state()["episode"].copy()
    obs = env.reset().cpu().numpy()
    b = O.BraxEnv(kind)
    b.cfg = CC.oracle_cfg_of(env.cfg)
    ref = np.stack([b.reset_with(b.draw(3, i, int(ep[i]))) for i in range(env.num_envs)])
    if kind == CC.BRAX_HOVER:
        assert np.array_equal(obs, ref)
    else:
        assert np.all(_close(obs, ref, atol=1e-7, rtol=1e-6))
    noise = np.float32(alt["reset_noise"])
    assert np.all(np.abs(obs[:, 11:]) <= noise) and np.abs(obs[:, 11:]).max() > 0.01
    env.close()

# ---------------------------------------------------------------------------------------------
# e. every fused family equals its per-step loop on alt_cfg handles
@contextlib.contextmanager
def alt_handles():
    """Inside, every QuadVecEnv carries alt_cfg of its (kind, wrapper) under whatever cfg_overrides its caller
    gives; a max_episode_steps its caller states stays (the families' tests place their truncations by it).
    The families' own tests then run unchanged: their envs, laws and policies on another plant, other
    bounds, another time step. Yields the kernel forms of the handles made; none may be a SPEC form."""
    from uav_reinforcement_learning_control_amd.envs import vec_env as VE
    init = QuadVecEnv.__init__
    sig = inspect.signature(init)
    forms = []

    def alt_init(self, *a, **kw):
        b = sig.bind(self, *a, **kw)
        b.apply_defaults()
        alt = CC.alt_cfg(VE._ENV_KINDS[b.arguments["env"]], VE._WRAPPERS[b.arguments["wrapper"]])
        if b.arguments["max_episode_steps"] is not None:
            alt.pop("max_episode_steps")
        b.arguments["cfg_overrides"] = {**alt, **(b.arguments["cfg_overrides"] or {})}
        init(*b.args, **b.kwargs)
        forms.append(N.lib().quad_kernel_form(self._h))

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(QuadVecEnv, "__init__", alt_init)
        yield forms
    assert forms and all(f & 16 == 0 for f in forms)


@pytest.fixture
def alt():
    with alt_handles() as forms:
        yield forms


@pytest.fixture(scope="module")
def fp128():
    from uav_reinforcement_learning_control_amd.ppo.fused import FusedPolicy
    f = FusedPolicy(TR._policy())
    f.pack()
    return f


def test_alt_handles_carry_alt_cfg(alt):
    e = QuadVecEnv(8, env="trajectory", wrapper="RateControlWrapper", device=DEV, max_episode_steps=9)
    want = CC.quad_cfg(CC.TRAJ, CC.CTBR, dict(CC.alt_cfg(CC.TRAJ, CC.CTBR), max_episode_steps=9))
    want.auto_reset = e.cfg.auto_reset
    assert bytes(e.cfg) == bytes(want) and e.dt == 0.008
    e.close()


@pytest.mark.parametrize("env_name,wrapper,helper", [("hover", None, "1"), ("trajectory", "RateControlWrapper", "1w")])
def test_alt_step_random_is_the_step_by_step_rollout(alt, monkeypatch, env_name, wrapper, helper):
    TP.test_step_random_is_the_step_by_step_rollout(env_name, wrapper, "0", helper, monkeypatch)


@pytest.mark.parametrize("kind,wrapper,max_steps,chunks,nt", [("hover", "RateControlWrapper", 9, (7, 13), "2"),
                                                             ("trajectory", "RateControlWrapper", 11, (5, 5, 10), "1"),
                                                             ("hover", None, 6, (20,), "2")])
def test_alt_one_launch_rollout_is_bit_identical(alt, monkeypatch, kind, wrapper, max_steps, chunks, nt):
    TR.test_one_launch_rollout_is_bit_identical(kind, wrapper, max_steps, 130, chunks, nt, monkeypatch)


@pytest.mark.parametrize("case", [("hover", None, "deployed", 130, 12, 7, TW.NT2_256),
                                  ("trajectory", "RateControlWrapper", "env", 130, 12, 7, TW.NT2_256),
                                  ("hover", "RateControlWrapper", "deployed", 130, 8, None, {})],
                         ids=["hover-deployed", "traj-ctbr-env", "hover-ctbr-deployed-alt-limit"])
def test_alt_policy_episode_equals_the_per_step_loop(alt, monkeypatch, fp128, case):
    PE.test_fused_episode_equals_the_per_step_loop(fp128, monkeypatch, *case)


@pytest.mark.parametrize("kind,wrapper,mode", [("hover", None, "env"), ("trajectory", "RateControlWrapper", "deployed")])
def test_alt_actor_episode_equals_the_per_step_loop(alt, kind, wrapper, mode):
    TA.test_fused_episode_equals_the_per_step_loop(kind, wrapper, mode, 64, 64, "tanh")


@pytest.mark.parametrize("wrapper,mode", [(None, "deployed"), ("RateControlWrapper", "env")])
def test_alt_actor_laps_equal_the_contract_loop(alt, wrapper, mode):
    TA.test_fused_laps_equal_the_contract_loop(wrapper, mode, 64, 64, "tanh")


@pytest.mark.parametrize("law,limit", [("pid_yaw", 6), ("pid_world", None), ("se3", 6), ("smc", None), ("lqr", 6)])
def test_alt_law_laps_equal_the_contract_loop(alt, monkeypatch, law, limit):
    TW.test_fused_law_laps_equal_the_contract_loop(monkeypatch, law, 130, limit, {})


@pytest.mark.parametrize("wrapper,mode,limit,pins", [(None, "deployed", 6, TW.NT2_256),
                                                    ("RateControlWrapper", "env", None, {"QUADENV_ROLLOUT_NT": "2", "QUADENV_EPISODE_BLOCK": "64"})],
                         ids=["deployed", "ctbr-env"])
def test_alt_policy_laps_equal_the_contract_loop(alt, monkeypatch, fp128, wrapper, mode, limit, pins):
    TW.test_fused_policy_laps_equal_the_contract_loop(fp128, monkeypatch, wrapper, mode, 130, limit, pins)


@pytest.mark.parametrize("kind,mode", [("hover", "yaw_frame"), ("trajectory", "world_frame")])
def test_alt_pid_episode_equals_unfused_loop(alt, kind, mode):
    TPID.test_fused_episode_equals_unfused_loop(kind, mode, 80, 64, TPID.NENV)


@pytest.mark.parametrize("kind,law", [("hover", "se3"), ("trajectory", "smc"), ("hover", "lqr"), ("trajectory", "se3")])
def test_alt_ctrl_episode_equals_unfused_loop(alt, kind, law):
    TC.test_fused_episode_equals_unfused_loop(kind, law, TC.NENV, 80, 64)


@pytest.mark.parametrize("kind,deterministic", [("brax_hover", False), ("brax_jax_mjx", True)])
def test_alt_brax_episode_equals_the_per_step_loop(alt, kind, deterministic):
    TBA.test_fused_episode_equals_the_per_step_loop(kind, deterministic, 64, 64, "tanh")


@pytest.mark.parametrize("kind", ["brax_hover", "brax_jax_mjx"])
def test_alt_brax_unroll_equals_the_contract_loop(alt, kind):
    TBU.test_unroll_equals_the_contract_loop(kind, 64, 64, "tanh")


def test_alt_population_members_equal_standalone_ppo():
    """One PopulationPPO iteration of two members built with cfg_overrides = alt_cfg: each member equals the
    stand-alone PPO on the same overrides, bit for bit (test_members_equal_standalone_ppo's comparison), and
    evaluate() flies its episodes on envs that carry the overrides (evaluate_episodes on alt handles)."""
    from uav_reinforcement_learning_control_amd.evaluate import evaluate_episodes
    from uav_reinforcement_learning_control_amd.ppo import PPO
    from uav_reinforcement_learning_control_amd.ppo.population import PopulationPPO
    ov = CC.alt_cfg(CC.HOVER, CC.CTBR)
    members = list(zip(TPP._configs(), TPP.SEEDS))[:2]
    want = []
    for cfg, seed in members:
        env = QuadVecEnv(TPP.N_ENVS, env="hover", wrapper=TPP.WRAPPER, device=DEV, seed=seed, cfg_overrides=ov)
        _generic(env)
        model = PPO(env, dataclasses.replace(cfg, graph_update=True), seed=seed)
        rs = model.collect_rollouts()
        model.train()
        want.append((TPP._state(model), TPP._stats_key(rs), model.num_timesteps))
    pop = PopulationPPO(members, n_envs=TPP.N_ENVS, env="hover", wrapper=TPP.WRAPPER, device=DEV,
                        env_kwargs=dict(cfg_overrides=ov))
    rs = pop.collect_rollouts()
    pop.train()
    for m in range(2):
        assert bytes(pop.member(m).env.cfg) == bytes(CC.quad_cfg(CC.HOVER, CC.CTBR, ov))
        TPP._same(TPP._state(pop.member(m)), want[m][0], f"member {m}")
        assert TPP._stats_key(rs[m]) == want[m][1] and pop.member(m).num_timesteps == want[m][2]
    seeds = [1_000_003 * (s + 1) + 4 for s in TPP.SEEDS[:2]]
    got = pop.evaluate(num_episodes=10, seeds=seeds)
    with alt_handles():
        refs = [evaluate_episodes(pop.member(m).policy, num_episodes=10, wrapper=TPP.WRAPPER, device=DEV, seed=seeds[m])
                for m in range(2)]
    plain = evaluate_episodes(pop.member(0).policy, num_episodes=10, wrapper=TPP.WRAPPER, device=DEV, seed=seeds[0])
    for m in range(2):
        for k in ("rewards", "lengths", "terminated"):
            assert np.array_equal(np.asarray(got[m][k]), np.asarray(refs[m][k])), (m, k)
    assert not np.array_equal(np.asarray(got[0]["rewards"]), np.asarray(plain["rewards"]))  # (the defaults fly differently)
    pop.close()


# ---------------------------------------------------------------------------------------------
# f. the control laws' plant
LAWS = ("yaw", "world", "se3", "smc", "lqr")
PLANTS = {"alt": lambda: CC.alt_cfg(CC.HOVER, CC.NONE), **{k: (lambda v=v: v) for k, v in CC.PLANT_CASES.items()}}


def _cuda(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


@pytest.mark.parametrize("law", LAWS)
@pytest.mark.parametrize("plant", list(PLANTS))
def test_law_reads_the_handles_plant(plant, law):
    """pid_act (both frames) and ctrl_act (SE(3), sliding mode, LQR) on a handle with another plant,
    against the float64 references built with plant_of(cfg), on the golden fixtures' state and target
    rows, from non-zero integrators, at the laws' existing tolerances."""
    rows = 130
    pid = law in ("yaw", "world")
    fx = np.load(os.path.join(GOLDEN, "golden_pid.npz" if pid else "golden_ctrl.npz"))
    S, T = fx[law + "_state"][:rows], fx[law + "_target9"][:rows]
    env = _env(CC.HOVER, CC.NONE, 8, PLANTS[plant](), auto_reset=False)  # the handle supplies the plant only
    p = CC.plant_of(env.cfg)
    rng = np.random.default_rng(3)
    if pid:
        st0 = rng.uniform(-0.005, 0.005, (6, rows))
        st, diag = _cuda(st0), torch.zeros(rows, 6, dtype=torch.float64, device=DEV)
        a = env.pid_act(_cuda(S), _cuda(T), st, mode={"yaw": "yaw_frame", "world": "world_frame"}[law], diag=diag)
    else:
        st0 = np.concatenate([rng.uniform(-0.005, 0.005, (6, rows)), rng.uniform(-0.3, 0.3, (2, rows))])
        st, diag = _cuda(st0), torch.zeros(rows, 7, dtype=torch.float64, device=DEV)
        a = env.ctrl_act(_cuda(S), _cuda(T), st, law=law, diag=diag)
    a, st, diag = a.cpu().numpy(), st.cpu().numpy(), diag.cpu().numpy()
    env.close()
    used = 6 if (pid or law != "smc") else 8
    for i in range(rows):
        if pid:
            c = pid_ref.PidRef(mode=pid_ref.WORLD_FRAME if law == "world" else pid_ref.YAW_FRAME, plant=p)
            c.integ[:] = st0[:, i]
            ra, rd = c.compute(S[i], T[i])
            rs = c.integ
        else:
            c = ctrl_ref.from_params(law, ctl.CtrlParams())
            c.p.update(p)
            c.state[:] = st0[:, i]
            ra, rd = c.compute(S[i], T[i])
            rs = c.state
        assert np.abs(a[i].astype(np.float64) - ra).max() <= ACT_TOL, (i, a[i], ra)
        assert np.abs(st[:used, i] - rs[:used]).max() <= STATE_TOL, i
        assert np.abs(diag[i] - rd).max() <= DIAG_TOL, i
