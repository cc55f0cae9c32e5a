"""The deployed observation path on the CPU: the product's law (csrc/quad_deploy.h, host instantiation) and
the numpy restatement (tests/deploy_ref.py) against calls recorded from the reference's VelocityEstimator
and build_observation (tests/golden/golden_deploy.npz, tools/gen_golden_deploy.py).

Bars: estimator velocity and state 1e-12 (absolute; velocities here are O(10) m/s and every operation is a
float64 one in the reference's order, so both sides are expected equal); observations bit for bit (norm_obs1
is NumPy's float32 sequence, DESIGN 3, and the clip is exact).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import deploy_host
import deploy_ref
from uav_reinforcement_learning_control_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_deploy.npz")
EST_TOL = 1e-12


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(GOLDEN))


def _runs(fx):
    run = int(fx["est_run"])
    n = len(fx["est_t"])
    return [(r, r + run) for r in range(0, n, run)]


def test_estimator_host_and_ref_match_the_fixture(fx):
    pos, t, max_dt = fx["est_pos"], fx["est_t"], float(fx["est_max_dt"])
    branches = {"first": 0, "bad_dt": 0, "filter": 0}
    nonpos = gap = 0
    for a, alpha in enumerate(fx["est_alphas"]):
        for lo, hi in _runs(fx):
            vel, st = deploy_host.est_calls(alpha, max_dt, pos[lo:hi], t[lo:hi])
            assert np.abs(vel - fx["est_vel"][a, lo:hi]).max() <= EST_TOL
            assert np.abs(st - fx["est_state"][a, lo:hi]).max() <= EST_TOL
            ref = deploy_ref.VelEstRef(alpha, max_dt)
            for i in range(lo, hi):
                v = ref.update(pos[i].astype(np.float64), t[i])
                assert np.abs(v - fx["est_vel"][a, i]).max() <= EST_TOL
                assert np.abs(ref.state() - fx["est_state"][a, i]).max() <= EST_TOL
            for k in branches:
                branches[k] += ref.branches[k]
            if a == 0:
                dt = np.diff(t[lo:hi])
                nonpos += int((dt <= 0).sum())
                gap += int((dt > max_dt).sum())
    # the first-call branch once per run, and both reset branches (dt <= 0, dt > max_dt) recorded
    assert branches["first"] == len(fx["est_alphas"]) * len(_runs(fx))
    assert nonpos >= 3 and gap >= 3 and branches["bad_dt"] == len(fx["est_alphas"]) * (nonpos + gap)
    assert branches["filter"] > 0.9 * fx["est_vel"][..., 0].size
    # a reset really zeroes the velocity in the fixture
    lo, hi = _runs(fx)[1]
    j = lo + 1 + int(np.nonzero(np.diff(t[lo:hi]) <= 0)[0][0])
    assert np.all(fx["est_vel"][3, j] == 0.0) and np.any(fx["est_vel"][3, j - 1] != 0.0)


def _state12(fx):
    n = len(fx["obs_out"])
    s = np.zeros((n, 12), np.float32)
    s[:, 0:3], s[:, 3:6], s[:, 9:12] = fx["obs_drone_pos"], fx["obs_attitude"], fx["obs_angular_vel"]
    s[:, 6:9] = 777.0  # the true velocity columns are not read
    return s


def test_observations_host_and_ref_equal_the_fixture_bit_for_bit(fx):
    want = fx["obs_out"]
    got = deploy_host.deploy_obs(_state12(fx), fx["obs_target"], fx["obs_linear_vel"])
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    ref = np.stack([deploy_ref.build_obs(fx["obs_drone_pos"][i], fx["obs_target"][i], fx["obs_attitude"][i],
                                         fx["obs_linear_vel"][i], fx["obs_angular_vel"][i]) for i in range(len(want))])
    assert np.array_equal(ref.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(deploy_ref.OBS_LOW, fx["obs_low"]) and np.array_equal(deploy_ref.OBS_HIGH, fx["obs_high"])
    # the clip binds on about a third of the components, and some sit exactly on a bound
    clipped = np.abs(want) == 1.0
    assert 0.25 < clipped.mean() < 0.5
    raw = np.concatenate([(fx["obs_target"].astype(np.float64) - fx["obs_drone_pos"]), fx["obs_attitude"],
                          fx["obs_linear_vel"], fx["obs_angular_vel"]], axis=1)
    on = (raw.astype(np.float32) == fx["obs_low"]) | (raw.astype(np.float32) == fx["obs_high"])
    assert on.sum() >= 50 and np.all(np.abs(want[on]) == 1.0)
    assert np.abs(want).max() <= 1.0


def test_non_finite_positions_and_alphas_follow_the_ref():
    rng = np.random.default_rng(5)
    n = 400
    pos = rng.normal(0, 1, (n, 3)).astype(np.float32)
    t = np.arange(n) * 0.01
    special = np.array([np.nan, np.inf, -np.inf], np.float32)
    for i in range(7, n, 29):
        pos[i, i % 3] = special[(i // 29) % 3]
    t[100], t[200] = np.nan, np.inf
    for alpha in (0.5, np.nan, np.inf, -np.inf, 1.0):
        vel, st = deploy_host.est_calls(alpha, 0.1, pos, t)
        ref = deploy_ref.VelEstRef(alpha, 0.1)
        rv = np.array([ref.update(pos[i].astype(np.float64), t[i]) for i in range(n)])
        assert np.array_equal(np.isnan(vel), np.isnan(rv)) and np.array_equal(np.isinf(vel), np.isinf(rv))
        fin = np.isfinite(rv)
        assert np.abs(vel[fin] - rv[fin]).max() <= EST_TOL * max(1.0, np.abs(rv[fin]).max())
        assert np.isnan(rv).any() or alpha == 0.5
        # the builder: NaN passes the clip as np.clip lets it, infinities land on +-1
        s = np.zeros((n, 12), np.float32)
        s[:, 0:3] = pos
        tg = np.zeros((n, 3), np.float32)
        got = deploy_host.deploy_obs(s, tg, vel)
        want = np.stack([deploy_ref.build_obs(pos[i], tg[i], s[i, 3:6], rv[i], s[i, 9:12]) for i in range(n)])
        assert np.array_equal(np.isnan(got), np.isnan(want))
        assert np.array_equal(got[~np.isnan(want)], want[~np.isnan(want)])
        assert np.isnan(want).any()


def test_deploy_struct_layouts_match_the_header(tmp_path):
    header = os.path.join(ROOT, "include", "quadenv.h")
    prog = tmp_path / "layout.c"
    prog.write_text(f'''#include <stdio.h>
#include <stddef.h>
#include "{os.path.abspath(header)}"
int main(void) {{
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d %d\\n", sizeof(QuadVelEst),
         offsetof(QuadVelEst, alpha_all), offsetof(QuadVelEst, max_dt), offsetof(QuadVelEst, state),
         sizeof(QuadPolicyRun), offsetof(QuadPolicyRun, max_steps), offsetof(QuadPolicyRun, trace_envs),
         offsetof(QuadPolicyRun, est), offsetof(QuadPolicyRun, est_dt), offsetof(QuadPolicyRun, trace_actions),
         offsetof(QuadPolicyRun, trace_obs), offsetof(QuadPolicyRun, trace_vel_est), offsetof(QuadPolicyRun, metrics),
         offsetof(QuadPolicyRun, vel_err_sq), QUAD_EST_NSTATE, QUAD_OBS_ENV, QUAD_OBS_DEPLOYED, QUADENV_ABI_VERSION);
  return 0;
}}''')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(prog)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    V, R = N.QuadVelEst, N.QuadPolicyRun
    want = [C.sizeof(V), V.alpha_all.offset, V.max_dt.offset, V.state.offset, C.sizeof(R), R.max_steps.offset,
            R.trace_envs.offset, R.est.offset, R.est_dt.offset, R.trace_actions.offset, R.trace_obs.offset,
            R.trace_vel_est.offset, R.metrics.offset, R.vel_err_sq.offset, N.EST_NSTATE, N.OBS_ENV, N.OBS_DEPLOYED,
            N.ABI_VERSION]
    assert got == want and got[0] == 32 and got[-1] == 8
    assert "quad_deploy_obs" in N.EXPORTS and "quad_policy_episode" in N.EXPORTS


def test_velocity_rmse_arithmetic_on_a_synthetic_trace():
    """evaluate_velocity_estimator's figures (velocity_summary) against numpy on a trace built here: two alphas
    x three episodes of different lengths, the error sums from deploy_ref on a synthetic flight."""
    from uav_reinforcement_learning_control_amd.evaluate import vel_rmse, velocity_summary
    rng = np.random.default_rng(11)
    alphas, E, dt = [0.0, 0.7], 3, 0.01
    lengths = [40, 25, 1]
    sums, steps, all_sq = [], [], {a: [] for a in alphas}
    for alpha in alphas:
        for e in range(E):
            T = lengths[e]
            v = np.cumsum(rng.normal(0, 0.05, (T + 1, 3)), axis=0)
            p = np.cumsum(v * dt, axis=0).astype(np.float32)
            s = np.zeros((T, 12), np.float32)
            s[:, 0:3], s[:, 6:9] = p[1:], v[1:]
            tot, vs = deploy_ref.vel_err_sq(s, p[0], alpha, dt)
            sq = ((vs - s[:, 6:9].astype(np.float64)) ** 2).sum(axis=1)
            assert abs(tot - sq.sum()) <= 1e-12 * max(1.0, sq.sum())
            sums.append(tot); steps.append(T); all_sq[alpha].append(sq)
    m = {"vel_err_sq": np.array(sums), "steps": np.array(steps, np.int32), "status": np.array([2, 2, 1] * 2, np.int32),
         "total_reward": np.arange(6, dtype=np.float64), "pos_err_sum": np.array(steps, np.float64) * 0.5}
    out = velocity_summary(alphas, E, m, closed_loop=True)
    for a, alpha in enumerate(alphas):
        flat = np.concatenate(all_sq[alpha])
        want = np.sqrt(np.sum(np.array(sums[a * E:(a + 1) * E])) / sum(lengths))
        assert out["rmse"][a] == want
        assert abs(out["rmse"][a] - np.sqrt(flat.mean())) <= 1e-12 * out["rmse"][a]
        assert out["steps"][a] == sum(lengths)
    assert np.array_equal(out["mean_reward"], [1.0, 4.0]) and np.allclose(out["survival"], 2.0 / 3.0)
    assert np.allclose(out["mean_pos_error"], 0.5) and np.array_equal(out["mean_length"], [22.0, 22.0])
    assert out["rmse"][0] < out["rmse"][1]  # alpha = 0 is the plain finite difference: the smallest lag
    assert len(out["table"].splitlines()) == 3 and "survival" in out["table"]
    assert "survival" not in velocity_summary(alphas, E, m, closed_loop=False)["table"]
    assert vel_rmse([0.0], [0]) == 0.0


def test_sanitized_deploy_law_is_clean():
    """csrc/quad_deploy.h (host instantiation) under ASan + UBSan: the stand-alone program
    tools/san/san_deploy.hip drives it over random, huge and non-finite inputs (every finding aborts)."""
    san = os.path.join(ROOT, "tools", "san")
    subprocess.run(["make", "-s", "-C", san, "_build/san_deploy"], check=True, timeout=600)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(san, "_build", "san_deploy")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "san_deploy OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
