"""TEST INFRASTRUCTURE ONLY: ctypes front-end of tests/hostsim_plin/libhostsim_plin.so, which runs the per-step arithmetic of the Poisson-linear Kalman factory
(csrc/kalman_plin.h::plin_step / plin_norm_logpdf, the text the HIP kernels compile) on the CPU.  A plain g++ build.  Never imported by the product package."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "libhostsim_plin.so")
_SRC = os.path.join(_HERE, "hostsim_plin.cpp")
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


def steps(x, u, y, H, c, delta, order, dtype=np.float64):
    """x, u (T, dx), y (T, dy), H (dy, dx), c (dy) -> (value (T,) float64, ys (T, dx), Om (T, dx, dx) or None for order 1) by plin_step, step by step"""
    dt = np.dtype(dtype)
    x, u, y, H, c = (np.ascontiguousarray(a, dt) for a in (x, u, y, H, c))
    T, d = x.shape
    dy = y.shape[1]
    assert u.shape == (T, d) and H.shape == (dy, d) and c.shape == (dy,) and y.shape[0] == T
    value, ys, Om = np.zeros(T), np.zeros((T, d), dt), np.zeros((T, d, d), dt)
    rc = lib().hs_plin_steps(0 if dt == np.float32 else 1, d, T, dy, int(order), C.c_double(float(delta)), _vp(x), _vp(u), _vp(y), _vp(H), _vp(c),
                             value.ctypes.data_as(C.POINTER(C.c_double)), _vp(ys), _vp(Om))
    assert rc == 0, rc
    return value, ys, (Om if order == 2 else None)


def norm_logpdf(y, x, Om, dtype=np.float64):
    """log N(y_t; x_t, Om_t) per step, y, x (T, dx), Om (T, dx, dx), by plin_norm_logpdf -> (T,) float64"""
    dt = np.dtype(dtype)
    y, x, Om = (np.ascontiguousarray(a, dt) for a in (y, x, Om))
    T, d = x.shape
    out = np.zeros(T)
    rc = lib().hs_plin_norm(0 if dt == np.float32 else 1, d, T, _vp(y), _vp(x), _vp(Om), out.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == 0, rc
    return out
