"""The waypoint tracker on the CPU: the product's law (csrc/quad_waypoints.h, host instantiation) against the
numpy restatement of the reference's loop (tests/waypoints_ref.py) on synthetic position / reward / flag
sequences. Both sides run float64 on the same float32 words in the same order, so every comparison is exact.
"""
import ctypes as C
import os
import subprocess

import numpy as np

import waypoints_host
import waypoints_ref
from uav_reinforcement_learning_control_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(wp, radius, pos, rew, term, trunc):
    got = waypoints_host.lap(wp, radius, pos, rew, term, trunc)
    want = waypoints_ref.lap(wp, radius, pos, rew, term, trunc)
    assert got[0] == want[0]
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32))
    assert np.array_equal(got[3].view(np.uint32), want[3].view(np.uint32))
    return got


def _flags(n, term_at=None, trunc_at=None):
    te, tr = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    if term_at is not None:
        te[term_at] = 1
    if trunc_at is not None:
        tr[trunc_at] = 1
    return te, tr


def test_distance_equal_to_the_radius_is_not_reached():
    # |(0.75, 1, 0)| = 1.25 with every square and the sum exact; the next float32 below reaches
    wp = np.array([[5.0, 5.0, 5.0], [0.0, 0.0, 0.0], [9.0, 9.0, 9.0]])
    pos = np.array([[0.75, 1.0, 0.0]] * 3, np.float32)
    rew = np.array([0.5, 0.25, 0.125], np.float32)
    steps, track, target, _ = _same(wp, 1.25, pos, rew, *_flags(3))
    assert steps == 3 and np.all(track[:, 1] == 0) and np.all(track[:, 4] == 0) and track[-1, 5] == 0.875
    assert np.all(target == 0.0)
    pos[1, 1] = np.nextafter(np.float32(1.0), np.float32(0.0))
    steps, track, target, _ = _same(wp, 1.25, pos, rew, *_flags(3))
    assert list(track[:, 1]) == [0, 1, 1] and list(track[:, 0]) == [1, 2, 2] and np.all(target[2] == 9.0)


def test_distances_within_rounding_of_the_radius_follow_the_square_root():
    """Distances a few ulps to 1e-9 (relative) on either side of the radius, set through the float64 waypoint."""
    rng = np.random.default_rng(7)
    hits = 0
    for radius in (0.25, 0.3, 1e-3, 7.0):
        r = float(np.float32(radius))
        for delta in (0.0, 1e-16, 2e-16, 1e-15, 1e-13, 4.9e-13, 5.1e-13, 9.9e-13, 1.01e-12, 2e-12, 1e-9):
            for sign in (1.0, -1.0):
                for _ in range(4):
                    pos = rng.uniform(-1, 1, 3).astype(np.float32)
                    u = rng.normal(0, 1, 3)
                    u /= np.linalg.norm(u)
                    wp = np.array([[9.0, 9.0, 9.0], pos.astype(np.float64) - u * r * (1.0 + sign * delta), [5.0, 5.0, 5.0]])
                    _, track, _, _ = _same(wp, radius, pos[None], np.zeros(1, np.float32), *_flags(1))
                    hits += int(track[0, 1])
    assert 100 < hits < 250  # both outcomes occur


def test_one_point_set_ends_the_lap_on_the_first_reach():
    wp = np.array([[1.0, 2.0, 3.0]])
    pos = np.array([[4.0, 2.0, 3.0], [1.1, 2.0, 3.0], [1.0, 2.0, 3.0]], np.float32)
    steps, track, target, pos0 = _same(wp, 0.25, pos, np.ones(3, np.float32), *_flags(3))
    assert steps == 2 and list(pos0) == [1.0, 2.0, 3.0]
    assert list(track[1]) == [0, 1, 1, 2, 1, 2.0] and np.array_equal(track[2], track[1])  # frozen afterwards
    assert np.all(target == np.float32([1.0, 2.0, 3.0]))  # 1 % 1 = 0: the target is the start, never rewritten


def test_lap_wins_over_terminated_which_wins_over_truncated():
    wp = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 1.0], [2.0, 0.0, 1.0]])
    near1, near2, far = [1.0, 0.0, 1.0], [2.0, 0.0, 1.0], [5.0, 5.0, 5.0]
    # lap and terminated (and truncated) on the same step: status 1
    pos = np.array([near1, near2], np.float32)
    te, tr = _flags(2, term_at=1, trunc_at=1)
    steps, track, _, _ = _same(wp, 0.25, pos, np.ones(2, np.float32), te, tr)
    assert steps == 2 and track[1, 4] == 1 and track[1, 2] == 1 and track[1, 1] == 2
    # terminated beside truncated: status 2; truncated alone: 3
    pos = np.array([far, far], np.float32)
    assert _same(wp, 0.25, pos, np.ones(2, np.float32), *_flags(2, term_at=0, trunc_at=0))[1][0, 4] == 2
    assert _same(wp, 0.25, pos, np.ones(2, np.float32), *_flags(2, trunc_at=1))[1][1, 4] == 3
    # a switch on the terminating step is still counted, and the target is rewritten
    pos = np.array([near1], np.float32)
    _, track, target, _ = _same(wp, 0.25, pos, np.ones(1, np.float32), *_flags(1, term_at=0))
    assert list(track[0, :5]) == [2, 1, 0, 1, 2] and list(target[1]) == [2.0, 0.0, 1.0]


def test_waypoints_are_compared_in_float64_and_written_as_float32():
    w1 = 0.1 + 2.0 ** -30  # not a float32: the target register holds its rounding, the distance the float64
    assert float(np.float32(w1)) != w1
    wp = np.array([[0.0, 0.0, 0.0], [w1, 0.0, 0.0], [0.3, 0.7, 1.1]])
    radius = 1e-10
    d32 = abs(float(np.float32(w1)) - w1)
    assert d32 > radius  # sitting on the float32 target is outside this radius of the float64 waypoint
    pos = np.array([[np.float32(w1), 0.0, 0.0]] * 2, np.float32)
    steps, track, target, _ = _same(wp, radius, pos, np.zeros(2, np.float32), *_flags(2))
    assert steps == 2 and np.all(track[:, 1] == 0)
    assert target[0, 0] == np.float32(w1) and float(target[0, 0]) != w1
    steps, track, target, _ = _same(wp, 1e-6, pos, np.zeros(2, np.float32), *_flags(2))
    assert track[0, 1] == 1 and np.array_equal(target[1], np.float32([0.3, 0.7, 1.1]))


def test_random_flights_follow_the_restatement():
    rng = np.random.default_rng(3)
    ended = set()
    for case in range(60):
        cnt = int(rng.integers(1, 7))
        wp = rng.uniform(-1, 1, (cnt, 3))
        n = 40
        # hop between the neighbourhoods of the waypoints so switches, laps and misses all occur
        pos = (wp[rng.integers(0, cnt, n)] + rng.normal(0, 0.2, (n, 3))).astype(np.float32)
        rew = rng.normal(0, 1, n).astype(np.float32)
        te = (rng.random(n) < 0.02).astype(np.uint8)
        tr = (rng.random(n) < 0.02).astype(np.uint8)
        _, track, _, _ = _same(wp, 0.3, pos, rew, te, tr)
        ended.add(int(track[-1, 4]))
    assert ended == {0, 1, 2, 3}


def test_waypoint_run_layout_matches_the_header(tmp_path):
    header = os.path.join(ROOT, "include", "quadenv.h")
    prog = tmp_path / "layout.c"
    prog.write_text(f'''#include <stdio.h>
#include <stddef.h>
#include "{os.path.abspath(header)}"
int main(void) {{
  printf("%zu %zu %zu %zu %zu %zu %zu %d %d\\n", sizeof(QuadWaypointRun), offsetof(QuadWaypointRun, w),
         offsetof(QuadWaypointRun, s), offsetof(QuadWaypointRun, trace_reward), offsetof(QuadWaypointRun, trace_wp_idx),
         sizeof(QuadWaypoints), sizeof(QuadWaypointState), QUAD_PID_LAP, QUADENV_ABI_VERSION);
  return 0;
}}''')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(prog)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    R = N.QuadWaypointRun
    want = [C.sizeof(R), R.w.offset, R.s.offset, R.trace_reward.offset, R.trace_wp_idx.offset,
            C.sizeof(N.QuadWaypoints), C.sizeof(N.QuadWaypointState), N.PID_LAP, N.ABI_VERSION]
    assert got == want and got[0] == 96 and got[-2] == 4
    assert "quad_ctrl_waypoints" in N.EXPORTS and "quad_policy_waypoints" in N.EXPORTS
    L = N.lib()
    assert L.quad_abi_version() == N.ABI_VERSION and hasattr(L, "quad_ctrl_waypoints") and hasattr(L, "quad_policy_waypoints")


def test_sanitized_waypoint_law_is_clean():
    """csrc/quad_waypoints.h (host instantiation) under ASan + UBSan: the stand-alone program
    tools/san/san_waypoints.hip drives it over random, huge and non-finite inputs (every finding aborts)."""
    san = os.path.join(ROOT, "tools", "san")
    subprocess.run(["make", "-s", "-C", san, "_build/san_waypoints"], check=True, timeout=600)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(san, "_build", "san_waypoints")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "san_waypoints OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
