"""The cascaded PID baseline on the GPU (quad_pid_*: the controller kernels of csrc/ctrl.hip on gain rows): the
law alone against the reference controllers' recorded calls, the fused episode kernel against the unfused loop
(bit for bit), against the CPU loop (float64 oracle env + tests/pid_ref.py) and against the reference's own
episodes, its metrics, per-env gain sets, the gain rows' own output widths, argument checks, the tuner and the
controller comparison.

N = 130 is two full 64-thread blocks of the episode kernel plus a ragged one."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import pid_ref
from oracle import oracle as O
from uav_reinforcement_learning_control_amd import _native as N
from uav_reinforcement_learning_control_amd import controllers as ctl
from uav_reinforcement_learning_control_amd.envs import QuadVecEnv

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ACT_TOL, INTEG_TOL, DIAG_TOL = 2.0 ** -23, 1e-12, 1e-9
RUN = 50
NENV = 130
NWIDE = 2 * 256 + 2  # for the kernels with 256-thread blocks
DEV = "cuda:0"
MODE_ID = {"yaw": "yaw_frame", "world": "world_frame"}


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "golden_pid.npz"))


def _cuda(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


# ---------------------------------------------------------------------------------------------
# 5. pid_act vs fixture (a), and scattered gain sets vs pid_ref
@pytest.mark.parametrize("mode", ["yaw", "world"])
def test_pid_act_matches_reference_calls(fx, mode):
    S, T = fx[mode + "_state"], fx[mode + "_target9"]
    runs = len(S) // RUN
    env = QuadVecEnv(runs, device=DEV, auto_reset=False)
    # row r of call k is call k of run r: the runs advance side by side, integrators carried on the device
    S3, T3 = S.reshape(runs, RUN, 12), T.reshape(runs, RUN, 9)
    integ = torch.zeros(6, runs, dtype=torch.float64, device=DEV)
    diag = torch.zeros(runs, 6, dtype=torch.float64, device=DEV)
    A, D, I = np.zeros((runs, RUN, 4), np.float32), np.zeros((runs, RUN, 6)), np.zeros((runs, RUN, 6))
    for k in range(RUN):
        a = env.pid_act(_cuda(S3[:, k]), _cuda(T3[:, k]), integ, mode=MODE_ID[mode], diag=diag)
        A[:, k], D[:, k], I[:, k] = a.cpu().numpy(), diag.cpu().numpy(), integ.cpu().numpy().T
    env.close()
    A, D, I = A.reshape(-1, 4), D.reshape(-1, 6), I.reshape(-1, 6)
    print(f"{mode}: action err {np.abs(A - fx[mode + '_action']).max():.3g} integ "
          f"{np.abs(I - fx[mode + '_integ']).max():.3g} diag {np.abs(D - fx[mode + '_diag']).max():.3g}")
    assert np.abs(A.astype(np.float64) - fx[mode + "_action"]).max() <= ACT_TOL
    assert np.abs(I - fx[mode + "_integ"]).max() <= INTEG_TOL
    assert np.abs(D - fx[mode + "_diag"]).max() <= DIAG_TOL


def _three_sets():
    g0 = ctl.PIDGains()
    g1 = ctl.PIDGains(kp_xy=2.0, kd_xy=2.5, kp_yaw=40.0, kd_yaw=12.0, yaw_torque_scale=0.3, tilt_max=0.4)
    g2 = ctl.PIDGains(kp_z=3.0, ki_z=0.2, kp_att=120.0, kd_att=20.0, ki_rate_torque=0.015, axy_max=2.0, mass=0.25)
    return [g0, g1, g2]


# (the act kernel and k_target_info run 256-thread blocks: NWIDE = 2 * 256 + 2 rows cross two block boundaries
# and leave a ragged third block)
@pytest.mark.parametrize("rows", [NENV, NWIDE])
@pytest.mark.parametrize("mode", ["yaw", "world"])
def test_pid_act_with_scattered_gain_sets(fx, mode, rows):
    S, T = fx[mode + "_state"][:rows], fx[mode + "_target9"][:rows]
    assert len(S) == rows
    sets = _three_sets()
    set_of = (np.arange(rows) * 7 + 1) % 3
    env = QuadVecEnv(8, device=DEV, auto_reset=False)  # the handle supplies the plant constants only
    integ0 = np.random.default_rng(3).uniform(-0.005, 0.005, (6, rows))
    integ = _cuda(integ0)
    diag = torch.zeros(rows, 6, dtype=torch.float64, device=DEV)
    a = env.pid_act(_cuda(S), _cuda(T), integ, gains=sets, set_of=set_of, mode=MODE_ID[mode], diag=diag).cpu().numpy()
    env.close()
    integ, diag = integ.cpu().numpy(), diag.cpu().numpy()
    for i in range(rows):
        g = sets[set_of[i]]
        c = pid_ref.PidRef(g.to_dict(), pid_ref.WORLD_FRAME if mode == "world" else pid_ref.YAW_FRAME,
                           plant={"mass": g.mass})
        c.integ[:] = integ0[:, i]
        ra, rd = c.compute(S[i], T[i])
        assert np.abs(a[i].astype(np.float64) - ra).max() <= ACT_TOL, i
        assert np.abs(integ[:, i] - c.integ).max() <= INTEG_TOL, i
        assert np.abs(diag[i] - rd).max() <= DIAG_TOL, i


SENTINEL = 0x7FF8DEADBEEF1234  # a NaN no law produces; compared as bits


def _guarded(words, guard, fill=None):
    """One float64 allocation of words + guard doubles: (all of it as int64 bits, the leading `words` doubles).
    The tail is the guard; the head holds `fill` or the sentinel too."""
    buf = torch.full((words + guard,), SENTINEL, dtype=torch.int64, device=DEV)
    head = buf[:words].view(torch.float64)
    if fill is not None:
        head.copy_(_cuda(fill).reshape(-1))
    return buf, head


def _bits(t):
    return t.contiguous().view(torch.int64).cpu().numpy()


@pytest.mark.parametrize("mode", ["yaw", "world"])
def test_pid_rows_keep_their_widths_and_equal_the_family(fx, mode):
    """quad_pid_* run the controller family's kernels on 22-double gain rows: diag is [n,6] and integ [6][n], not
    the family's [n,7] and [8][n]. Each output sits in one allocation with a sentinel tail (a [n,7] diag or an
    [8][n] state block would land in it, never past it); the tails stay as they were and the outputs equal
    quad_ctrl_*'s with the same PID law, bit for bit."""
    law = "pid_" + mode
    sets = _three_sets()
    # the law alone, NWIDE rows: two 256-thread blocks plus two rows
    n = NWIDE
    S, T = _cuda(fx[mode + "_state"][:n]), _cuda(fx[mode + "_target9"][:n])
    assert S.shape[0] == n
    set_of = (np.arange(n) * 7 + 1) % 3
    integ0 = np.random.default_rng(3).uniform(-0.005, 0.005, (6, n))
    env = QuadVecEnv(8, device=DEV, auto_reset=False)  # the handle supplies the plant constants only
    dbuf, dhead = _guarded(n * 6, n)
    ibuf, ihead = _guarded(6 * n, 2 * n, integ0)
    diag, integ = dhead.view(n, 6), ihead.view(6, n)
    a = env.pid_act(S, T, integ, gains=sets, set_of=set_of, mode=MODE_ID[mode], diag=diag)
    state = torch.zeros(N.CTRL_NSTATE, n, dtype=torch.float64, device=DEV)
    state[:6] = _cuda(integ0)
    diag7 = torch.zeros(n, N.CTRL_NDIAG, dtype=torch.float64, device=DEV)
    ac = env.ctrl_act(S, T, state, params=sets, set_of=set_of, law=law, diag=diag7)
    env.close()
    assert np.all(_bits(dbuf[n * 6:]) == SENTINEL) and np.all(_bits(ibuf[6 * n:]) == SENTINEL)
    assert not np.any(_bits(diag) == SENTINEL) and not np.array_equal(integ.cpu().numpy(), integ0)
    assert np.array_equal(_bits(diag), _bits(diag7[:, :6])) and np.array_equal(_bits(integ), _bits(state[:6]))
    assert np.array_equal(a.cpu().numpy().view(np.uint32), ac.cpu().numpy().view(np.uint32))
    # the fused episode, NENV envs: two 64-thread blocks plus a ragged one, 8 steps
    n = NENV
    set_of = (np.arange(n) * 5) % 3
    integ0 = np.random.default_rng(4).uniform(-0.005, 0.005, (6, n))
    envs = [QuadVecEnv(n, device=DEV, seed=11, auto_reset=False) for _ in range(2)]
    for e in envs:
        e.reset()
    ibuf, ihead = _guarded(6 * n, 2 * n, integ0)
    integ = ihead.view(6, n)
    f = envs[0].pid_episode(sets, set_of=set_of, mode=MODE_ID[mode], max_steps=8, integ=integ)
    state = torch.zeros(N.CTRL_NSTATE, n, dtype=torch.float64, device=DEV)
    state[:6] = _cuda(integ0)
    c = envs[1].ctrl_episode(sets, set_of=set_of, law=law, max_steps=8, state=state)
    for e in envs:
        e.close()
    assert np.all(_bits(ibuf[6 * n:]) == SENTINEL)
    assert np.all(f["steps"].cpu().numpy() == 8) and not np.array_equal(integ.cpu().numpy(), integ0)
    assert np.array_equal(_bits(integ), _bits(state[:6])) and not state[6:].any()
    for k, _ in N.PID_METRIC_FIELDS:
        assert np.array_equal(f[k].cpu().numpy().view(np.uint8), c[k].cpu().numpy().view(np.uint8)), k


# ---------------------------------------------------------------------------------------------
def _edge_states(env, kind):
    """A handful of envs just inside a position bound and moving outward: they terminate within a few
    steps whatever the controller does."""
    st = env.get_state()
    d = 1.2 * env.dt  # 0.012 m at the default time step: 0.8 of a step at 1.5 m/s
    for j, i in enumerate((3, 64, 65, 127, 129)):
        ax = j % 2
        st["qpos"][i, ax] = float(env.cfg.term_high[ax]) - d * (j + 1)  # (2 m hover, 3 m trajectory at the defaults)
        st["qvel"][i, ax] = 1.5
        st["qpos"][i, 3:7] = (1, 0, 0, 0)
    env.set_state(qpos=st["qpos"], qvel=st["qvel"])


def _unfused(env, gains, set_of, mode, T):
    """observe -> (pid_act -> step)*, every env stepped for T steps (auto_reset = 0)."""
    n = env.num_envs
    _, s12 = env.observe(state=True)
    s12 = s12.clone()
    ti = env.current_target_info()
    integ = torch.zeros(6, n, dtype=torch.float64, device=env.device)
    out = {k: [] for k in ("actions", "state12", "reward", "terminated", "truncated", "target")}
    for _ in range(T):
        a = env.pid_act(s12, ti, integ, gains=gains, set_of=set_of, mode=mode)
        out["target"].append(ti[:, 0:3].clone())
        _, rew, te, tr, info = env.step(a, info="full")
        s12 = info["state"].clone()
        ti = env.target_info.clone()
        out["actions"].append(a.clone()); out["state12"].append(s12)
        out["reward"].append(rew.clone()); out["terminated"].append(te.clone()); out["truncated"].append(tr.clone())
    return {k: torch.stack(v).cpu().numpy() for k, v in out.items()}


def _lengths(term, trunc):
    done = term | trunc
    T = done.shape[0]
    first = np.where(done.any(0), done.argmax(0) + 1, T)
    status = np.where(~done.any(0), N.PID_RUNNING,
                      np.where(term[first - 1, np.arange(done.shape[1])], N.PID_TERMINATED, N.PID_TRUNCATED))
    return first.astype(np.int32), status.astype(np.int32)


@pytest.mark.parametrize("kind", ["hover", "trajectory"])
def test_current_target_info_is_what_step_reports(kind):
    """k_target_info over three 256-thread blocks: after a step it equals that step's info["target*"], bit for
    bit; before the first step it is reset()'s info (the target, and for the trajectory kind the spline's first
    sample: the start position with non-zero velocity and acceleration)."""
    env = QuadVecEnv(NWIDE, env=kind, device=DEV, seed=13, auto_reset=False)
    env.reset()
    st = env.get_state()
    t0 = env.current_target_info().cpu().numpy()
    if kind == "trajectory":  # the spline evaluated at t = 0 (float64, rounded to float32) is its first waypoint
        assert np.abs(t0[:, 0:3] - st["qpos"][:, 0:3]).max() <= 2.0 ** -22 and np.all(np.abs(t0[:, 3:9]).max(1) > 0)
    else:
        assert np.array_equal(t0[:, 0:3], st["target"]) and not t0[:, 3:9].any()
    for k in range(3):
        _, _, _, _, info = env.step(env.random_actions(k), info="full")
        want = env.target_info.cpu().numpy()
        got = env.current_target_info().cpu().numpy()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), k
    if kind == "trajectory":
        assert not np.array_equal(got, t0)  # the spline sample moves with the step count
    env.close()


# 6. fused = unfused, bit for bit
# (time limit 64: truncation inside the run, generic constant block; the last case keeps the default
# 512-step limit, whose handles take the kernels with compiled-in constants)
# (NWIDE envs: the unfused loop's act kernel and k_target_info run three 256-thread blocks)
@pytest.mark.parametrize("kind,mode,T,limit,n", [("hover", "yaw_frame", 80, 64, NENV),
                                                 ("trajectory", "world_frame", 80, 64, NENV),
                                                 ("hover", "yaw_frame", 40, 64, NENV),
                                                 ("hover", "world_frame", 24, None, NENV),
                                                 ("trajectory", "world_frame", 70, 64, NWIDE)])
def test_fused_episode_equals_unfused_loop(kind, mode, T, limit, n):
    envs = [QuadVecEnv(n, env=kind, device=DEV, seed=11, max_episode_steps=limit, auto_reset=False)
            for _ in range(2)]
    spec_off = os.environ.get("QUADENV_SPEC", "1") == "0"
    assert bool(N.lib().quad_kernel_form(envs[0]._h) & 16) == (limit is None and not spec_off)  # bit 4: compiled-in constants
    for e in envs:
        e.reset()
        _edge_states(e, kind)
    sets = _three_sets()
    set_of = (np.arange(n) * 5) % 3
    f = envs[0].pid_episode(sets, set_of=set_of, mode=mode, max_steps=T, trace_envs=n)
    f = {k: v.cpu().numpy() for k, v in f.items()}
    u = _unfused(envs[1], sets, set_of, mode, T)
    length, status = _lengths(u["terminated"], u["truncated"])
    assert np.array_equal(f["steps"], length) and np.array_equal(f["status"], status)
    assert (status == N.PID_TERMINATED).sum() >= 5 and length.min() < 10
    assert ((status == N.PID_TRUNCATED) & (length == 64)).any() == (T >= 64)
    assert (status == N.PID_RUNNING).any() == (T < 64)
    live = np.arange(T)[:, None] < length[None, :]
    for k in ("actions", "state12"):
        assert np.array_equal(f[k][live].view(np.uint32), u[k][live].view(np.uint32)), k
        assert not f[k][~live].any()  # rows past an env's last step are not written
    # stored state: the state after each env's last step; equal to the unfused handle's for envs still running
    sf, su = envs[0].get_state(), envs[1].get_state()
    run = status == N.PID_RUNNING
    for k in ("qpos", "qvel", "voltage", "step_count", "target"):
        assert np.array_equal(sf[k][run], su[k][run]), k
    assert np.array_equal(sf["step_count"], length)
    last = f["state12"][length - 1, np.arange(n)]
    assert np.array_equal(sf["qpos"][:, 0:3], last[:, 0:3])
    for e in envs:
        e.close()


# ---------------------------------------------------------------------------------------------
# 7. against the CPU loop: float64 oracle env + pid_ref
def test_episode_matches_cpu_loop():
    n, T = 16, 512
    env = QuadVecEnv(n, device=DEV, seed=7, auto_reset=False)
    env.reset()
    f = {k: v.cpu().numpy() for k, v in env.pid_episode(mode="yaw_frame", trace_envs=n).items()}
    env.close()
    cfg = O.default_cfg(O.ENV_HOVER, O.WRAP_NONE)
    worst = 0.0
    for i in range(n):
        i12, t3 = O.reset_draw(cfg, 7, i, 0)
        e = O.Env(cfg=cfg)
        e.reset_with(i12, t3)
        c = pid_ref.PidRef()
        s12, total, steps, pos = i12, 0.0, 0, []
        while True:
            a, _ = c.compute(s12, t3)
            o = O.out_to_dict(e.step(a))
            s12 = o["state12"]
            total += o["reward"]; steps += 1; pos.append(s12[:3])
            if o["terminated"] or o["truncated"]:
                break
        assert steps == T, (i, steps)  # every reference episode runs the full 512 steps
        assert f["steps"][i] == steps
        err = np.abs(f["state12"][:steps, i, 0:3] - np.array(pos)).max()
        worst = max(worst, err)
        assert err <= 1e-4, (i, err)
        assert abs(f["total_reward"][i] - total) <= 1e-4 * max(1.0, abs(total)), (i, f["total_reward"][i], total)
    print("largest position difference vs the CPU loop:", worst)


# 8. against the reference's own episodes
@pytest.mark.parametrize("mode", ["yaw", "world"])
def test_episode_matches_reference_episodes(fx, mode):
    n = len(fx[mode + "_ep_length"])
    env = QuadVecEnv(n, device=DEV, seed=0, auto_reset=False)
    env.reset()
    env.set_state(qpos=fx[mode + "_ep_qpos0"].astype(np.float32), qvel=fx[mode + "_ep_qvel0"].astype(np.float32),
                  target=fx[mode + "_ep_target"], voltage=np.full(n, env.cfg.nominal_voltage, np.float32),
                  step_count=np.zeros(n, np.int32))
    f = {k: v.cpu().numpy() for k, v in env.pid_episode(mode=MODE_ID[mode], trace_envs=n).items()}
    env.close()
    assert np.array_equal(f["steps"], fx[mode + "_ep_length"])
    pos = f["state12"][:200, :, 0:3].transpose(1, 0, 2)
    err = np.abs(pos - fx[mode + "_ep_pos"][:, :200]).max()
    print(mode, "largest position difference vs the reference's episodes over 200 steps:", err)
    assert err <= 1e-4
    # the recorded actions of those steps, to the same bar: no gain of the law from a state component to an
    # action component exceeds 0.16 (torque per radian of attitude error: I kd kp_att / kd_att / MAX_TORQUE), so
    # an action differs by less than the state it was computed from does
    aerr = np.abs(f["actions"][:200].transpose(1, 0, 2) - fx[mode + "_ep_actions"]).max()
    print(mode, "largest action difference over those steps:", aerr)
    assert fx[mode + "_ep_actions"].shape == (n, 200, 4) and aerr <= 1e-4


# ---------------------------------------------------------------------------------------------
# 9. metrics = numpy on the kernel's own traces
@pytest.mark.parametrize("kind,mode", [("hover", "yaw_frame"), ("trajectory", "world_frame")])
def test_metrics_equal_numpy_on_traces(kind, mode):
    envs = [QuadVecEnv(NENV, env=kind, device=DEV, seed=5, max_episode_steps=96, auto_reset=False) for _ in range(2)]
    for e in envs:
        e.reset()
        _edge_states(e, kind)
    f = {k: v.cpu().numpy() for k, v in envs[0].pid_episode(mode=mode, trace_envs=NENV).items()}
    # rewards and the targets read before each step come from the unfused loop (bit-identical, test 6)
    u = _unfused(envs[1], None, None, mode, 96)
    for e in envs:
        e.close()
    length, status = _lengths(u["terminated"], u["truncated"])
    assert np.array_equal(f["steps"], length) and np.array_equal(f["status"], status)
    for i in range(NENV):
        L = length[i]
        s = f["state12"][:L, i]
        d = (s[:, 0:3] - u["target"][:L, i]).astype(np.float64)  # float32 difference
        pe = np.sqrt((d[:, 0] ** 2 + d[:, 1] ** 2) + d[:, 2] ** 2)
        yr = s[:, 11].astype(np.float64)
        exact = {"pos_err_max": pe.max(), "yaw_rate_abs_max": np.abs(yr).max(),
                 "yaw_rate_sign_changes": np.sum(np.diff(np.sign(yr)) != 0)}
        sums = {"total_reward": u["reward"][:L, i].astype(np.float64).sum(), "pos_err_sum": pe.sum(),
                "pos_err_sq": (pe ** 2).sum(), "yaw_rate_abs_sum": np.abs(yr).sum(), "yaw_rate_sum": yr.sum(),
                "yaw_rate_sq": (yr ** 2).sum(), "yaw_rate_delta_sum": np.abs(np.diff(yr)).sum()}
        for k, v in exact.items():
            assert f[k][i] == v, (k, i, f[k][i], v)
        for k, v in sums.items():
            scale = max(abs(v), np.abs(yr).sum() if k == "yaw_rate_sum" else 0.0)
            assert abs(f[k][i] - v) <= 1e-9 * scale + 1e-300, (k, i, f[k][i], v)


# ---------------------------------------------------------------------------------------------
# 10. per-env gains
def test_per_env_gain_sets():
    dead = ctl.PIDGains(kp_xy=0.0, kd_xy=0.0, ki_xy=0.0, kp_z=0.0, kd_z=0.0, ki_z=0.0, kp_att=0.0)
    sets = [ctl.PIDGains(), dead, _three_sets()[1]]
    set_of = np.arange(NENV) % 3

    def run(table, so):
        env = QuadVecEnv(NENV, device=DEV, seed=21, auto_reset=False)
        env.reset()
        r = {k: v.cpu().numpy() for k, v in env.pid_episode(table, set_of=so, trace_envs=NENV).items()}
        r["final_qpos"] = env.get_state()["qpos"]
        env.close()
        return r

    a = run(sets, set_of)
    assert np.all(a["status"][set_of == 1] == N.PID_TERMINATED) and a["steps"][set_of == 1].max() < 512
    assert np.all(a["status"][set_of == 0] == N.PID_TRUNCATED) and np.all(a["steps"][set_of == 0] == 512)
    # permuting the table and set_of together changes nothing, bit for bit
    perm = np.array([2, 0, 1])  # new table row j = old row perm[j]
    inv = np.argsort(perm)
    b = run([sets[j] for j in perm], inv[set_of])
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
    # an out-of-range entry: "invalid", no step, state untouched, the others unaffected
    bad = set_of.copy()
    bad[[1, 70, 129]] = [3, -1, 1 << 30]
    env = QuadVecEnv(NENV, device=DEV, seed=21, auto_reset=False)
    env.reset()
    before = env.get_state()["qpos"]
    c = {k: v.cpu().numpy() for k, v in env.pid_episode(sets, set_of=bad, trace_envs=NENV).items()}
    after = env.get_state()["qpos"]
    env.close()
    isbad = np.zeros(NENV, bool)
    isbad[[1, 70, 129]] = True
    assert np.all(c["status"][isbad] == N.PID_INVALID) and np.all(c["steps"][isbad] == 0)
    assert np.array_equal(before[isbad], after[isbad]) and not c["state12"][:, isbad].any()
    for k in c:
        ck, ak = (c[k][:, ~isbad], a[k][:, ~isbad]) if k in ("actions", "state12") else (c[k][~isbad], a[k][~isbad])
        assert np.array_equal(ck.view(np.uint8), ak.view(np.uint8)), k
    assert np.array_equal(after[~isbad], a["final_qpos"][~isbad])


# ---------------------------------------------------------------------------------------------
# 11. argument checks: every QUAD_EINVAL case, no launch
def test_argument_checks():
    L = N.lib()
    n = 8
    tab = ctl.gain_table(None, DEV)
    s12 = torch.zeros(n, 12, device=DEV); t9 = torch.zeros(n, 9, device=DEV)
    integ = torch.zeros(6, n, dtype=torch.float64, device=DEV); act = torch.zeros(n, 4, device=DEV)
    m = {k: torch.zeros(n, dtype=getattr(torch, dt), device=DEV) for k, dt in N.PID_METRIC_FIELDS}
    p = lambda t: C.c_void_p(t.data_ptr())

    def act_rc(h, gains=tab, n_sets=1, mode=0, s=s12, t=t9, rows=n, ig=integ, a=act):
        return L.quad_pid_act(h, None if gains is None else p(gains), n_sets, None, mode, None if s is None else p(s),
                              None if t is None else p(t), rows, None if ig is None else p(ig),
                              None if a is None else p(a), None, None)

    def ep_rc(h, gains=tab, n_sets=1, mode=0, max_steps=4, trace_envs=0, ta=None, drop=None):
        mm = {k: (None if k == drop else v.data_ptr()) for k, v in m.items()}
        run = N.QuadPidRun(gains=None if gains is None else gains.data_ptr(), set_of=None, n_sets=n_sets, mode=mode,
                           max_steps=max_steps, trace_envs=trace_envs, integ=None, trace_actions=ta,
                           trace_state12=None, metrics=N.QuadPidMetrics(**mm))
        return L.quad_pid_episode(h, C.byref(run), None)

    good = QuadVecEnv(n, device=DEV, auto_reset=False)
    good.reset()
    before = good.get_state()
    for rc in (act_rc(good._h, mode=2), act_rc(good._h, mode=-1), act_rc(good._h, n_sets=0), act_rc(good._h, gains=None),
               act_rc(good._h, s=None), act_rc(good._h, t=None), act_rc(good._h, ig=None), act_rc(good._h, a=None),
               act_rc(good._h, rows=0), act_rc(None),
               ep_rc(good._h, mode=2), ep_rc(good._h, n_sets=0), ep_rc(good._h, gains=None), ep_rc(good._h, max_steps=0),
               ep_rc(good._h, drop="steps"), ep_rc(good._h, drop="yaw_rate_delta_sum"), ep_rc(good._h, trace_envs=n + 1),
               L.quad_pid_episode(good._h, None, None), L.quad_target_info(good._h, None, None)):
        assert rc == N.QUAD_EINVAL
        assert len(L.quad_last_error()) > 0
    # trace sizes that overflow 32-bit offsets (the check precedes any access: the pointer is never read)
    big = QuadVecEnv(1 << 16, device=DEV, auto_reset=False)
    mb = {k: torch.zeros(1 << 16, dtype=getattr(torch, dt), device=DEV) for k, dt in N.PID_METRIC_FIELDS}
    run = N.QuadPidRun(gains=tab.data_ptr(), set_of=None, n_sets=1, mode=0, max_steps=2048, trace_envs=1 << 16,
                       integ=None, trace_actions=act.data_ptr(), trace_state12=None,
                       metrics=N.QuadPidMetrics(**{k: v.data_ptr() for k, v in mb.items()}))
    assert L.quad_pid_episode(big._h, C.byref(run), None) == N.QUAD_EINVAL and b"32-bit" in L.quad_last_error()
    big.close()
    torch.cuda.synchronize()
    after = good.get_state()
    assert all(np.array_equal(before[k], after[k]) for k in before)  # nothing was launched
    assert act_rc(good._h) == N.QUAD_OK and ep_rc(good._h) == N.QUAD_OK
    good.close()
    # a brax kind, and every wrapper other than NONE
    for kw in (dict(env="brax_hover"), dict(wrapper="RateControlWrapper"), dict(wrapper="RelPosActWrapper"),
               dict(wrapper="ctbr_relpos")):
        e = QuadVecEnv(n, device=DEV, auto_reset=False, **kw)
        assert act_rc(e._h) == N.QUAD_EINVAL and ep_rc(e._h) == N.QUAD_EINVAL
        e.close()


# ---------------------------------------------------------------------------------------------
# 12. the tuner
def test_tuner_is_deterministic_and_never_worse_than_its_start(tmp_path):
    from uav_reinforcement_learning_control_amd.tune_pid import SEARCH, tune
    out = tmp_path / "tuned.json"
    kw = dict(candidates=8, episodes=8, generations=2, max_episode_steps=128, seed=3, final_top=3, final_episodes=16)
    a = tune(out=str(out), **kw)
    b = tune(**kw)
    assert a["gains"] == b["gains"] and a["history"] == b["history"] and a["fresh_score"] == b["fresh_score"]
    assert a["tuning_score"] >= a["start_tuning_score"]
    assert a["history"][0] >= a["start_tuning_score"] and a["history"][1] >= a["history"][0]
    g = ctl.PIDGains.from_json(str(out))
    assert g == a["gains"]
    for f, lo, hi in SEARCH:
        assert lo <= getattr(g, f) <= hi
    # only the six searched quantities moved
    moved = {f for f in N.PID_GAIN_FIELDS if getattr(g, f) != getattr(ctl.PIDGains(), f)}
    assert moved <= {f for f, _, _ in SEARCH}
    assert 0.0 < a["fresh_score"] <= 1.0 and 0.0 < a["fresh_start_score"] <= 1.0
    for bad in (dict(generations=0), dict(candidates=0), dict(episodes=0)):
        with pytest.raises(ValueError):
            tune(**bad)


# 13. the comparison
def test_compare_controllers_flies_identical_episodes():
    from uav_reinforcement_learning_control_amd.evaluate import compare_controllers, evaluate_pid_episodes
    from uav_reinforcement_learning_control_amd.ppo.policy import ActorCritic
    torch.manual_seed(0)
    r = compare_controllers(ActorCritic(), num_episodes=256, seed=9, wrapper=None)
    pol, pid = r["policy"], r["pid"]
    assert np.array_equal(pol["reset_obs"], pid["reset_obs"]) and pol["reset_obs"].shape == (256, 12)
    assert np.abs(pol["reset_obs"]).max() > 0
    for d in (pol, pid):
        for k in ("rewards", "lengths", "terminated", "mean_reward", "std_reward", "mean_length", "std_length",
                  "mean_pos_error", "survival"):
            assert k in d
        assert d["rewards"].shape == (256,) and np.all(d["lengths"] >= 1) and np.all(d["lengths"] <= 512)
    # the PID at the reference's gains hovers (the reference's 8 episodes all run 512 steps); an untrained policy does not
    assert pid["survival"] > 0.9 and pid["mean_reward"] > pol["mean_reward"]
    assert "policy" in r["table"] and "pid" in r["table"]
    again = evaluate_pid_episodes(num_episodes=256, seed=9)
    assert np.array_equal(again["rewards"], pid["rewards"])
