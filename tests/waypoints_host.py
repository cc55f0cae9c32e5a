"""ctypes binding of tests/native_waypoints (TEST INFRASTRUCTURE ONLY): the product's waypoint tracker
(csrc/quad_waypoints.h) instantiated on the host. Builds on first use, like tests/deploy_host.py."""
import ctypes as C
import os
import subprocess

import numpy as np

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native_waypoints")
_PATH = os.path.join(_DIR, "_build", "libwaypointshost.so")
_H = None
dp = C.POINTER(C.c_double)
fp = C.POINTER(C.c_float)
bp = C.POINTER(C.c_ubyte)


def lib():
    global _H
    if _H is None:
        subprocess.run(["make", "-s", "-C", _DIR], check=True)
        H = C.CDLL(_PATH)
        H.host_lap.argtypes = [dp, C.c_int, C.c_float, fp, fp, bp, bp, C.c_int, dp, fp, fp]
        _H = H
    return _H


def lap(wp, reach_radius, pos, reward, term, trunc):
    """One env's lap over the rows. Returns (steps taken, track [n,6] float64 = wp_idx, reached, laps, steps,
    status, total_reward after each row, target [n+1,3] float32, start position [3] float32)."""
    w = np.ascontiguousarray(wp, np.float64).reshape(-1, 3)
    p = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    n = len(p)
    r = np.ascontiguousarray(reward, np.float32).reshape(n)
    te = np.ascontiguousarray(term, np.uint8).reshape(n)
    tr = np.ascontiguousarray(trunc, np.uint8).reshape(n)
    track = np.zeros((n, 6), np.float64)
    target = np.zeros((n + 1, 3), np.float32)
    pos0 = np.zeros(3, np.float32)
    steps = lib().host_lap(w.ctypes.data_as(dp), len(w), float(reach_radius), p.ctypes.data_as(fp), r.ctypes.data_as(fp),
                           te.ctypes.data_as(bp), tr.ctypes.data_as(bp), n, track.ctypes.data_as(dp),
                           target.ctypes.data_as(fp), pos0.ctypes.data_as(fp))
    assert steps >= 0
    return steps, track, target, pos0
