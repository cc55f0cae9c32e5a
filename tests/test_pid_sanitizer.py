"""The PID control law (csrc/quad_pid.h, host instantiation) under AddressSanitizer +
UndefinedBehaviorSanitizer: the stand-alone program tools/san/san_pid.hip drives both modes over
random, saturated and non-finite states, targets and gains (every finding aborts)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = os.path.join(ROOT, "tools", "san")


def test_sanitized_pid_law_is_clean():
    subprocess.run(["make", "-s", "-C", SAN, "_build/san_pid"], check=True, timeout=600)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(SAN, "_build", "san_pid")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "san_pid OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
