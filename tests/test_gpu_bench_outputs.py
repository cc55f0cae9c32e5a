"""bench.py's plain run and --dump-outputs: a run without --full prints the headline keys only (none
of the extra measurements), times exactly --steps steps, and writes the last timed step's outputs,
which equal stepping the same envs W + K times in this process with the same action batches
(a step count that is no multiple of --graph-chunk included); a second run with the same arguments
writes the same bytes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, K, W = 4096, 7, 3
NAMES = ("obs", "reward", "terminated", "truncated", "terminal_observation")


def _run(out_dir) -> dict:
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "LOCAL_WORLD_SIZE"):
        e.pop(k, None)
    r = subprocess.run([sys.executable, "-u", os.path.join(REPO, "bench.py"), "--gpus", "1", "--envs", str(N),
                        "--steps", str(K), "--warmup", str(W), "--graph-chunk", "4", "--dump-outputs", str(out_dir)],
                       env=e, capture_output=True, text=True, timeout=120, cwd=REPO)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def first(tmp_path_factory):
    d = tmp_path_factory.mktemp("dump_a")
    return d, _run(d)


def test_plain_line_and_outputs_match_in_process_steps(first):
    import torch
    from uav_reinforcement_learning_control_amd.envs import QuadVecEnv
    d, line = first
    assert line["steps"] == K and line["warmup"] == W and line["n_gpus"] == 1 and line["full"] is False
    assert line["unit"] == "env-steps/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["ms_per_step"] > 0.0
    assert line["value"] == pytest.approx(N / (line["ms_per_step"] * 1e-3), rel=1e-9)
    for k in ("roofline", "rollout_phase", "end_to_end", "configs", "large_batch", "large_batch_dram",
              "cpu_baseline", "cpu_baseline_ppo"):
        assert k not in line, k
    assert sorted(os.listdir(d)) == sorted(n + ".npy" for n in NAMES)
    env = QuadVecEnv(N, env="hover", device="cuda:0", seed=0)
    env.reset()
    for k in range(W + K):
        obs, rew, te, tr, inf = env.step(env.random_actions(k), info="raw")
    torch.cuda.synchronize()
    want = dict(zip(NAMES, (obs, rew, te, tr, inf["terminal_observation"])))
    for name in NAMES:
        got = np.load(os.path.join(d, name + ".npy"))
        assert got.dtype == np.float32 and got.shape == tuple(want[name].shape), name
        np.testing.assert_array_equal(got, want[name].float().cpu().numpy(), err_msg=name)
    env.close()
    assert 0.0 < np.load(os.path.join(d, "reward.npy")).std()  # (not a buffer nobody wrote)


def test_second_run_writes_the_same_bytes(first, tmp_path):
    d, _ = first
    _run(tmp_path)
    for name in NAMES:
        a, b = (open(os.path.join(p, name + ".npy"), "rb").read() for p in (d, tmp_path))
        assert a == b, name
