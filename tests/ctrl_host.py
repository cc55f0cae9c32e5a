"""ctypes binding of tests/native_ctrl (TEST INFRASTRUCTURE ONLY): the product's controller-family laws
(csrc/quad_ctrl.h) instantiated on the host. Builds on first use, like tests/pid_host.py."""
import ctypes as C
import os
import subprocess

import numpy as np

from uav_reinforcement_learning_control_amd import _native as N

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native_ctrl")
_PATH = os.path.join(_DIR, "_build", "libctrlhost.so")
_H = None
dp = C.POINTER(C.c_double)
fp = C.POINTER(C.c_float)


def lib():
    global _H
    if _H is None:
        subprocess.run(["make", "-s", "-C", _DIR], check=True)
        H = C.CDLL(_PATH)
        H.host_ctrl_default_params.argtypes = [C.POINTER(N.QuadCtrlParams)]
        H.host_ctrl_default_params.restype = None
        H.host_ctrl_calls.argtypes = [C.POINTER(N.QuadCfg), C.POINTER(N.QuadCtrlParams), C.c_int, fp, fp, C.c_int,
                                      dp, fp, dp, dp]
        H.host_ctrl_qr.argtypes = [dp, dp]
        H.host_ctrl_qr.restype = None
        _H = H
    return _H


def default_params() -> N.QuadCtrlParams:
    p = N.QuadCtrlParams()
    lib().host_ctrl_default_params(C.byref(p))
    return p


def params_of(vector) -> N.QuadCtrlParams:
    """QuadCtrlParams from the 33 numbers in N.CTRL_PARAM_FIELDS order (CtrlParams.vector())."""
    v = np.ascontiguousarray(vector, np.float64)
    assert v.shape == (len(N.CTRL_PARAM_FIELDS),)
    return N.QuadCtrlParams.from_buffer_copy(v.tobytes())


def default_cfg() -> N.QuadCfg:
    return N.default_cfg(N.ENV_HOVER, N.WRAP_NONE)


def calls(params: N.QuadCtrlParams, law: int, state12, target9, cs=None, cfg=None):
    """Run the law over the rows in order, controller state carried. Returns (actions [n,4] f32,
    diag [n,7], controller state after each call [n,8])."""
    s = np.ascontiguousarray(state12, np.float32).reshape(-1, 12)
    t = np.ascontiguousarray(target9, np.float32).reshape(-1, 9)
    n = len(s)
    cs = np.zeros(N.CTRL_NSTATE, np.float64) if cs is None else np.array(cs, np.float64)
    a = np.zeros((n, 4), np.float32); d = np.zeros((n, N.CTRL_NDIAG), np.float64)
    so = np.zeros((n, N.CTRL_NSTATE), np.float64)
    cfg = default_cfg() if cfg is None else cfg
    rc = lib().host_ctrl_calls(C.byref(cfg), C.byref(params), int(law), s.ctypes.data_as(fp), t.ctypes.data_as(fp), n,
                               cs.ctypes.data_as(dp), a.ctypes.data_as(fp), d.ctypes.data_as(dp),
                               so.ctypes.data_as(dp))
    assert rc == 0
    return a, d, so


def qr_q(a) -> np.ndarray:
    a = np.ascontiguousarray(a, np.float64).reshape(3, 3)
    q = np.zeros((3, 3), np.float64)
    lib().host_ctrl_qr(a.ctypes.data_as(dp), q.ctypes.data_as(dp))
    return q
