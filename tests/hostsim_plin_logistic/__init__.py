"""TEST INFRASTRUCTURE ONLY: ctypes front-end of tests/hostsim_plin_logistic/libhostsim_plin_logistic.so, which runs the per-step arithmetic of the
logistic-linear Kalman factory (csrc/kalman_plin.h::plin_step_logistic, the text the HIP kernel compiles) on the CPU.  A plain g++ build, made on first use; a
sibling of tests/hostsim_plin.  Never imported by the product package."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "libhostsim_plin_logistic.so")
_SRC = os.path.join(_HERE, "hostsim_plin_logistic.cpp")
_CSRC = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "aux_ssm_samplers_amd", "csrc")


def build(force=False):
    deps = [_SRC] + [os.path.join(_CSRC, f) for f in ("smallmat.h", "rtc_compat.h", "kalman_plin.h")]
    if not force and os.path.exists(_SO) and all(os.path.getmtime(_SO) >= os.path.getmtime(d) for d in deps):
        return _SO
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", _SRC, "-o", _SO])
    return _SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
    return _lib


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def steps(x, u, y, H, c, s, w, delta, order, dtype=np.float64):
    """x, u (T, dx), y (T, dy), H (dy, dx), c, s, w (dy) -> (value (T,) float64, ys (T, dx), Om (T, dx, dx) or None for order 1) by plin_step_logistic, step by
    step; [c; s; w] is handed over as the (3, dy) array the device model carries"""
    dt = np.dtype(dtype)
    x, u, y, H = (np.ascontiguousarray(a, dt) for a in (x, u, y, H))
    csw = np.ascontiguousarray(np.stack([c, s, w]), dt)
    T, d = x.shape
    dy = y.shape[1]
    assert u.shape == (T, d) and H.shape == (dy, d) and csw.shape == (3, dy) and y.shape[0] == T
    value, ys, Om = np.zeros(T), np.zeros((T, d), dt), np.zeros((T, d, d), dt)
    rc = lib().hs_plin_logistic_steps(0 if dt == np.float32 else 1, d, T, dy, int(order), C.c_double(float(delta)), _vp(x), _vp(u), _vp(y), _vp(H), _vp(csw),
                                      value.ctypes.data_as(C.POINTER(C.c_double)), _vp(ys), _vp(Om))
    assert rc == 0, rc
    return value, ys, (Om if order == 2 else None)
