"""CPU checks of the controller family (SE(3), sliding mode, LQR): the product's laws compiled for the host
(tests/native_ctrl, csrc/quad_ctrl.h) and the float64 numpy restatement (tests/ctrl_ref.py) against the
reference controllers' recorded calls (tests/golden/golden_ctrl.npz, tools/gen_golden_ctrl.py); the
hand-written Householder QR against np.linalg.qr; the defaults; the JSON round trip; bad inputs; the struct
layouts; and the CPU closed loop (ctrl_ref.py on the float64 oracle env) against the reference's recorded
hover episodes, whose measured figure sets the GPU closed-loop bar."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import ctrl_host
import ctrl_ref
import pid_host
import pid_ref
from oracle import oracle as O
from uav_reinforcement_learning_control_amd import _native as N
from uav_reinforcement_learning_control_amd import controllers as ctl

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ACT_TOL = 2.0 ** -23  # one float32 rounding step at 1.0
STATE_TOL = 1e-12
DIAG_TOL = 1e-9       # measured on the host build: SE(3) 4.4e-15 with the Householder chain, so the bar stands
RUN = 50
SEQS = {"se3h": "se3", "se3": "se3", "smc": "smc", "lqr": "lqr"}  # fixture prefix -> law
LAW_ID = {"se3": N.CTRL_SE3, "smc": N.CTRL_SMC, "lqr": N.CTRL_LQR}


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "golden_ctrl.npz"))


def _check(name, a, d, cs, fx, seq):
    ea = np.abs(a.astype(np.float64) - fx[seq + "_action"]).max()
    ec = np.abs(cs - fx[seq + "_cstate"]).max()
    ed = np.abs(d - fx[seq + "_diag"]).max()
    print(f"{name}: max action err {ea:.3g}, controller state {ec:.3g}, diag {ed:.3g}")
    assert ea <= ACT_TOL
    assert ec <= STATE_TOL
    assert ed <= DIAG_TOL
    # the reference handed float32 arrays (its closed loops) lands within the same action bar
    assert np.abs(a.astype(np.float64) - fx[seq + "_action_f32in"]).max() <= ACT_TOL


@pytest.mark.parametrize("seq", list(SEQS))
def test_host_law_matches_reference_calls(fx, seq):
    S, T = fx[seq + "_state"], fx[seq + "_target9"]
    assert len(S) % RUN == 0 and len(S) >= 400
    p = ctrl_host.default_params()
    A, D, Cs = [], [], []
    for r in range(0, len(S), RUN):
        a, d, cs = ctrl_host.calls(p, LAW_ID[SEQS[seq]], S[r:r + RUN], T[r:r + RUN])
        A.append(a); D.append(d); Cs.append(cs)
    _check("host law " + seq, np.concatenate(A), np.concatenate(D), np.concatenate(Cs), fx, seq)
    if SEQS[seq] != "smc":  # rows 6-7 are SMC's alone
        assert not np.concatenate(Cs)[:, 6:8].any()


@pytest.mark.parametrize("seq", list(SEQS))
def test_numpy_restatement_matches_reference_calls(fx, seq):
    S, T = fx[seq + "_state"], fx[seq + "_target9"]
    A, D, Cs = [], [], []
    for r in range(0, len(S), RUN):
        c = ctrl_ref.CtrlRef(SEQS[seq])
        for k in range(r, r + RUN):
            a, d = c.compute(S[k], T[k])
            A.append(a); D.append(d); Cs.append(c.state.copy())
            assert c.margin_all >= 1e-3 * (1 - 1e-6)  # the generator's rejection sampling
    _check("ctrl_ref " + seq, np.array(A), np.array(D), np.array(Cs), fx, seq)


def test_fixture_rows_exercise_the_laws(fx):
    for seq in ("se3", "smc", "lqr"):
        T = fx[seq + "_target9"]
        assert (np.abs(T[:, 3:9]) > 0.1).mean() > 0.5
    assert not fx["se3h_target9"][:, 3:9].any()
    # both signs of x_d[0] (the np.linalg.qr flip), at least a quarter of the rows each
    for seq in ("se3h", "se3"):
        c = ctrl_ref.CtrlRef("se3")
        pos = []
        for s, t in zip(fx[seq + "_state"], fx[seq + "_target9"]):
            c.reset()
            c.compute(s, t)
            pos.append(c.xd0 > 0)
        assert 0.25 <= np.mean(pos) <= 0.75
    # the SMC rows leave the deadband on most calls and use both extra states
    assert (np.abs(fx["smc_cstate"][:, 6]) > 0).mean() > 0.9 and (np.abs(fx["smc_cstate"][:, 7]) > 0).mean() > 0.9
    # LQR's ay reads xy_integral[0]: rows whose two xy integrals differ
    assert (np.abs(fx["lqr_cstate"][:, 0] - fx["lqr_cstate"][:, 1]) > 1e-3).mean() > 0.5


@pytest.mark.parametrize("law", ["se3", "smc", "lqr"])
def test_host_law_on_the_recorded_trajectory_episodes(fx, law):
    """The inputs the reference's closed loop fed its controller on TrajectoryFollowEnv (float32 arrays),
    through the host law with the state carried: the recorded actions, up to the first step near a
    discontinuity of the law."""
    p = ctrl_host.default_params()
    for e in range(len(fx[law + "_traj_length"])):
        cut = int(fx[law + "_traj_cut"][e])
        assert cut >= 150
        a, _, _ = ctrl_host.calls(p, LAW_ID[law], fx[law + "_traj_state"][e, :cut], fx[law + "_traj_target9"][e, :cut])
        err = np.abs(a.astype(np.float64) - fx[law + "_traj_actions"][e, :cut]).max()
        print(law, "episode", e, "steps", cut, "max action err", err)
        assert err <= ACT_TOL


def _sign_pattern(A):
    Q = np.linalg.qr(A)[0]
    return tuple((np.sign(np.sum(Q * A, axis=0)) > 0).tolist()[:2])


def test_householder_qr_matches_numpy_with_its_column_signs():
    rng = np.random.default_rng(5)
    seen = set()
    worst = 0.0
    for k in range(1000):
        # an orthonormal triad (what the law hands np.linalg.qr), every fourth one slightly off orthonormal
        M = rng.standard_normal((3, 3))
        A = np.linalg.qr(M)[0] * rng.choice([-1.0, 1.0], 3)
        if np.linalg.det(A) < 0:
            A[:, 2] = -A[:, 2]
        if k % 4 == 3:
            A = A + 1e-3 * rng.standard_normal((3, 3))
        want = np.linalg.qr(A)[0]
        seen.add(_sign_pattern(A))
        for got in (ctrl_ref.householder_q(A), ctrl_host.qr_q(A)):
            worst = max(worst, np.abs(got - want).max())
    print("largest |Q - np.linalg.qr| over 1,000 triads:", worst)
    assert worst <= 1e-14
    assert len(seen) == 4  # (x, y) kept / flipped in all four combinations
    # a first column already along +e1 or -e1: dlarfg's tau = 0 (identity) and tau = 2
    for A in (np.eye(3), np.diag([-1.0, -1.0, 1.0]), np.diag([1.0, -1.0, -1.0])):
        want = np.linalg.qr(A)[0]
        assert np.abs(ctrl_ref.householder_q(A) - want).max() <= 1e-14
        assert np.abs(ctrl_host.qr_q(A) - want).max() <= 1e-14


def test_defaults(fx):
    ref = json.load(open(os.path.join(GOLDEN, "pid_gains.json")))
    g = N.QuadCtrlParams()
    assert N.lib().quad_ctrl_default_params(C.byref(g)) == N.QUAD_OK
    assert N.lib().quad_ctrl_default_params(None) == N.QUAD_EINVAL
    h = ctrl_host.default_params()
    d = ctl.CtrlParams()
    for p in (g, h):
        for (sec, key), field in zip(pid_ref.FIELDS, N.PID_GAIN_FIELDS):
            assert getattr(p.base, field) == float(ref[sec][key]), (sec, key)
        assert p.base.mass == 0.2227
        assert np.abs(np.array(p.lqr_k[:]) - fx["lqr_K"]).max() <= 1e-12
        for k, v in ctrl_ref.SMC_DEFAULTS.items():
            assert getattr(p, k) == v, k
        assert p.se3_reorthonormalize == 1.0
        assert np.array_equal(np.frombuffer(bytes(p), np.float64), d.vector())
    assert (g.yaw_stw_k1, g.yaw_stw_k2, g.yaw_stw_boundary, g.yaw_v_int_max, g.yaw_rate_max, g.yaw_rate_lpf_alpha) == \
        (1.2, 2.0, 0.05, 2.0, 3.0, 0.2) and g.yaw_deadband == np.deg2rad(1.0)
    assert np.abs(np.array(ctrl_ref.LQR_K) - fx["lqr_K"]).max() <= 1e-12
    # the PID ids are the PID modes
    assert (N.CTRL_PID_YAW, N.CTRL_PID_WORLD) == (N.PID_YAW_FRAME, N.PID_WORLD_FRAME)


def test_pid_ids_run_the_pid_law():
    fxp = np.load(os.path.join(GOLDEN, "golden_pid.npz"))
    for mode, law in (("yaw", N.CTRL_PID_YAW), ("world", N.CTRL_PID_WORLD)):
        S, T = fxp[mode + "_state"][:RUN], fxp[mode + "_target9"][:RUN]
        a, d, cs = ctrl_host.calls(ctrl_host.default_params(), law, S, T)
        pa, pd_, pi = pid_host.calls(pid_host.default_gains(), law, S, T)
        assert np.array_equal(a, pa) and np.array_equal(d[:, :6], pd_) and np.array_equal(cs[:, :6], pi)
        assert not cs[:, 6:].any() and not d[:, 6].any()


def test_params_json_round_trip(tmp_path):
    src = os.path.join(GOLDEN, "pid_gains.json")
    p = ctl.CtrlParams.from_json(src)  # a plain pid_gains.json: the extras take their defaults
    assert p == ctl.CtrlParams()
    p.lqr_k1, p.yaw_stw_k2, p.yaw_deadband, p.se3_reorthonormalize, p.kp_att = 3.25, 1.5, 0.03, 0.0, 150.0
    out = tmp_path / "params.json"
    p.to_json(str(out))
    back = ctl.CtrlParams.from_json(str(out))
    assert back == p and np.array_equal(back.vector(), p.vector())
    d = json.load(open(out))
    assert d["lqr"]["k1"] == 3.25 and d["se3"]["reorthonormalize"] == 0.0 and d["attitude"]["kp"] == 150.0
    # the file keeps pid_gains.json's layout: the PID loader and the reference's constructors read it
    assert ctl.PIDGains.from_json(str(out)).kp_att == 150.0
    assert pid_ref.gains_vector(d)[6] == 150.0
    assert ctl.params_from_vector(p.vector()) == p
    assert ctl.param_table([ctl.PIDGains(kp_xy=2.0)], "cpu")[0, 0] == 2.0  # a PIDGains takes the default extras
    assert ctl.param_table(None, "cpu").shape == (1, 33)


def _bad_rows():
    s0 = np.zeros(12, np.float32); s0[2] = 1.0
    t0 = np.zeros(9, np.float32); t0[2] = 1.0
    rows = []
    for idx, val in ((0, np.nan), (4, np.nan), (5, np.inf), (7, -np.inf), (10, np.nan), (2, 1e30), (3, 1e6)):
        s = s0.copy(); s[idx] = val
        rows.append((s, t0.copy()))
    for idx, val in ((1, np.nan), (3, np.inf), (4, np.nan), (8, np.nan), (2, -1e30)):
        t = t0.copy(); t[idx] = val
        rows.append((s0.copy(), t))
    # saturated: far from the target, fast, tilted past the tilt clamp
    s = s0.copy(); s[0:3] = (-50, 40, -30); s[3:5] = (1.4, -1.4); s[6:12] = (30, -30, 30, 50, -50, 50)
    rows.append((s, t0.copy()))
    # zero thrust vector: az = -g exactly needs az_min <= -g (second parameter set below); and the thrust
    # axis along the desired x axis (y_norm fallback) cannot be reached inside the acceleration clamps, so the
    # fallbacks are reached through the parameter set as well
    rows.append((s0.copy(), t0.copy()))
    return rows


@pytest.mark.parametrize("law", ["se3", "smc", "lqr"])
def test_bad_inputs_give_the_restatements_pattern(law):
    sets = [ctl.CtrlParams(), ctl.CtrlParams(az_min=-20.0, axy_max=0.0, kp_z=0.0, kd_z=0.0, ki_z=0.0),
            ctl.CtrlParams(se3_reorthonormalize=0.0, mass=0.0)]
    for cp in sets:
        for s, t in _bad_rows():
            t = t.copy()
            if cp.az_min == -20.0:
                t[8] = np.float32(-9.81)  # feed-forward cancels gravity: |thrust vector| ~ 0
            ref = ctrl_ref.from_params(law, cp)
            ra, rd = ref.compute(s, t)
            a, d, cs = ctrl_host.calls(ctrl_host.params_of(cp.vector()), LAW_ID[law], s, t)
            assert np.array_equal(np.isnan(a[0]), np.isnan(ra)), (law, s, t, a, ra)
            assert np.array_equal(np.isnan(cs[0]), np.isnan(ref.state)), (law, s, t, cs, ref.state)
            assert np.array_equal(np.isnan(d[0]), np.isnan(rd)), (law, s, t, d, rd)
            fin = ~np.isnan(ra)
            assert np.all(np.abs(a[0][fin]) <= 1.0)
            assert np.abs(a[0][fin].astype(np.float64) - ra[fin]).max(initial=0.0) <= ACT_TOL, (law, s, t, a, ra)


def test_zero_thrust_vector_takes_the_fallbacks():
    """mass 0: the thrust vector is zero, its norm clips to 0.1, z_d = 0, and both < 1e-3 fallbacks fire
    (y_d = e3, x_d = e1); finite action, minimum thrust."""
    cp = ctl.CtrlParams(mass=0.0)
    s = np.zeros(12, np.float32); s[2] = 1.0
    t = np.zeros(9, np.float32); t[2] = 1.0
    for reortho in (1.0, 0.0):
        cp.se3_reorthonormalize = reortho
        a, d, _ = ctrl_host.calls(ctrl_host.params_of(cp.vector()), N.CTRL_SE3, s, t)
        ra, rd = ctrl_ref.from_params("se3", cp).compute(s, t)
        assert np.all(np.isfinite(a)) and np.abs(a[0].astype(np.float64) - ra).max() <= ACT_TOL
        assert abs(a[0, 0] - np.float32(2.0 * 0.1 / 52.0 - 1.0)) <= ACT_TOL
        assert np.abs(d[0] - rd).max() <= DIAG_TOL


def test_ctrl_struct_layouts_match_the_header(tmp_path):
    header = os.path.join(os.path.dirname(GOLDEN), os.pardir, "include", "quadenv.h")
    prog = tmp_path / "layout.c"
    prog.write_text(f'''#include <stdio.h>
#include <stddef.h>
#include "{os.path.abspath(header)}"
int main(void) {{
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d\\n", sizeof(QuadCtrlParams), offsetof(QuadCtrlParams, lqr_k),
         offsetof(QuadCtrlParams, yaw_deadband), offsetof(QuadCtrlParams, se3_reorthonormalize), sizeof(QuadCtrlRun),
         offsetof(QuadCtrlRun, law), offsetof(QuadCtrlRun, state), offsetof(QuadCtrlRun, trace_state12),
         offsetof(QuadCtrlRun, metrics), QUAD_CTRL_NSTATE, QUAD_CTRL_NDIAG);
  return 0;
}}''')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(prog)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    want = [C.sizeof(N.QuadCtrlParams), N.QuadCtrlParams.lqr_k.offset, N.QuadCtrlParams.yaw_deadband.offset,
            N.QuadCtrlParams.se3_reorthonormalize.offset, C.sizeof(N.QuadCtrlRun), N.QuadCtrlRun.law.offset,
            N.QuadCtrlRun.state.offset, N.QuadCtrlRun.trace_state12.offset, N.QuadCtrlRun.metrics.offset,
            N.CTRL_NSTATE, N.CTRL_NDIAG]
    assert got == want and got[0] == 33 * 8


# the figure the GPU closed-loop bar rests on (tests/test_gpu_ctrl.py): under 1e-5, so that bar is 1e-4
CPU_LOOP_TOL = 1e-5


@pytest.mark.parametrize("name,law,reortho", [("se3nq", "se3", False), ("smc", "smc", True), ("lqr", "lqr", True)])
def test_cpu_closed_loop_matches_reference_episodes(fx, name, law, reortho):
    """ctrl_ref.py on the float64 oracle env against the reference's own float32-input loop, over the recorded
    steps of every hover episode up to its cut."""
    cfg = O.default_cfg(O.ENV_HOVER, O.WRAP_NONE)
    worst, compared, recorded = 0.0, 0, 0
    for e in range(len(fx[name + "_hov_length"])):
        env = O.Env(cfg=cfg)
        env.set_full_state(fx[name + "_hov_qpos0"][e], fx[name + "_hov_qvel0"][e], cfg.nominal_voltage,
                           fx[name + "_hov_target"][e], 0)
        s12 = np.array(env.s.state12[:], np.float32)
        c = ctrl_ref.CtrlRef(law, se3_reorthonormalize=reortho)
        cut = int(fx[name + "_hov_cut"][e])
        rec = min(int(fx[name + "_hov_length"][e]), fx[name + "_hov_pos"].shape[1])
        pos = []
        for _ in range(cut):
            a, _ = c.compute(s12, fx[name + "_hov_target"][e])
            s12 = O.out_to_dict(env.step(a))["state12"]
            pos.append(s12[:3])
        worst = max(worst, np.abs(np.array(pos) - fx[name + "_hov_pos"][e, :cut]).max())
        compared += cut; recorded += rec
    print(name, "largest position difference, CPU loop vs the reference's episodes:", worst, "over", compared, "of",
          recorded, "recorded steps")
    assert compared >= 0.9 * recorded
    assert worst <= CPU_LOOP_TOL
