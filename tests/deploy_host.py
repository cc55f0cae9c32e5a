"""ctypes binding of tests/native_deploy (TEST INFRASTRUCTURE ONLY): the product's deployed-observation law
(csrc/quad_deploy.h) instantiated on the host. Builds on first use, like tests/pid_host.py."""
import ctypes as C
import os
import subprocess

import numpy as np

from uav_reinforcement_learning_control_amd import _native as N

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native_deploy")
_PATH = os.path.join(_DIR, "_build", "libdeployhost.so")
_H = None
dp = C.POINTER(C.c_double)
fp = C.POINTER(C.c_float)


def lib():
    global _H
    if _H is None:
        subprocess.run(["make", "-s", "-C", _DIR], check=True)
        H = C.CDLL(_PATH)
        H.host_est_calls.argtypes = [C.c_double, C.c_double, fp, dp, C.c_int, dp, dp, dp]
        H.host_deploy_obs.argtypes = [C.POINTER(N.QuadCfg), fp, fp, dp, C.c_int, fp]
        _H = H
    return _H


def est_calls(alpha: float, max_dt: float, pos, t, state=None):
    """update() over the rows in order, state carried. Returns (velocity [n,3], state after each call [n,8])."""
    p = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    ts = np.ascontiguousarray(t, np.float64).reshape(-1)
    n = len(p)
    st = np.zeros(8, np.float64) if state is None else np.array(state, np.float64)
    vel = np.zeros((n, 3), np.float64); so = np.zeros((n, 8), np.float64)
    rc = lib().host_est_calls(float(alpha), float(max_dt), p.ctypes.data_as(fp), ts.ctypes.data_as(dp), n,
                              st.ctypes.data_as(dp), vel.ctypes.data_as(dp), so.ctypes.data_as(dp))
    assert rc == 0
    return vel, so


def deploy_obs(state12, target, vel, cfg=None):
    """build_observation per row with the reference default bounds. Returns obs [n,12] float32."""
    s = np.ascontiguousarray(state12, np.float32).reshape(-1, 12)
    tg = np.ascontiguousarray(target, np.float32).reshape(-1, 3)
    v = np.ascontiguousarray(vel, np.float64).reshape(-1, 3)
    n = len(s)
    obs = np.zeros((n, 12), np.float32)
    cfg = N.default_cfg(N.ENV_HOVER, N.WRAP_NONE) if cfg is None else cfg
    rc = lib().host_deploy_obs(C.byref(cfg), s.ctypes.data_as(fp), tg.ctypes.data_as(fp), v.ctypes.data_as(dp), n,
                               obs.ctypes.data_as(fp))
    assert rc == 0
    return obs
