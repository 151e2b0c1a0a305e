"""TEST INFRASTRUCTURE ONLY: ctypes front-end of tests/hostsim_dynamics_theta/libhostsim_dynamics_theta.so, which runs the arithmetic of the conjugate dynamics step
(csrc/dynamics_theta.h: statistics, posterior, draw, gamma generator -- the text the HIP kernels compile) on the CPU.  A plain g++ build.  Never imported by the
product package."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "libhostsim_dynamics_theta.so")
_SRC = os.path.join(_HERE, "hostsim_dynamics_theta.cpp")
_CSRC = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "aux_ssm_samplers_amd", "csrc")


def build(force=False):
    deps = [_SRC] + [os.path.join(_CSRC, f) for f in ("dynamics_theta.h", "rng.h", "rng_tables.h", "smallmat.h", "det_math.h", "rtc_compat.h")]
    if not force and os.path.exists(_SO) and all(os.path.getmtime(_SO) >= os.path.getmtime(d) for d in deps):
        return _SO
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", _SRC, "-o", _SO])
    return _SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.hs_dt_update.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_double] + [C.c_void_p] * 6
        _lib.hs_dt_gamma.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.hs_dt_gamma_variates.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_longlong, C.c_int, C.c_void_p]
        _lib.hs_dt_stats.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    return _lib


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def segment_len(T):
    return lib().hs_dt_segment_len(int(T))


def stats(x):
    """x (T, d) -> the FULL statistics [S_zz | S_xz | S_xx] flat, by dt_accumulate transition by transition"""
    x = np.ascontiguousarray(x, np.float64)
    T, d = x.shape
    n = d + 1
    full = np.zeros(n * n + d * n + d * d)
    assert lib().hs_dt_stats(d, T, _vp(x), _vp(full)) == 0
    return full


def update(full, ntrans, M0, K0, nu0, Psi0, chi, ew, ea, chi_scale=1.0):
    """-> (flag, post flat [M_n | K_n | nu_n | Psi_n], Q (d, d), A (d, d + 1)) by dt_posterior + dt_draw"""
    M0, K0, Psi0, chi, ew, ea, full = (np.ascontiguousarray(a, np.float64) for a in (M0, K0, Psi0, chi, ew, ea, full))
    d = Psi0.shape[0]
    n = d + 1
    post, Q, A = np.zeros(d * n + n * n + 1 + d * d), np.zeros((d, d)), np.zeros((d, n))
    flag = lib().hs_dt_update(d, int(ntrans), _vp(full), _vp(M0), _vp(K0), float(nu0), _vp(Psi0), float(chi_scale), _vp(chi), _vp(ew), _vp(ea), _vp(post),
                              _vp(Q), _vp(A))
    assert flag >= 0
    return flag, post, Q, A


def gamma(key, stream, n, shapes):
    """-> (out (n, m), margin (n, m)): the draws and the accepted attempts' threshold - log u"""
    shapes = np.ascontiguousarray(shapes, np.float64)
    m = shapes.size
    out, margin = np.zeros((n, m)), np.zeros((n, m))
    assert lib().hs_dt_gamma(int(key[0]), int(key[1]), int(stream), n, m, _vp(shapes), _vp(out), _vp(margin)) == 0
    return out, margin


def gamma_variates(key, stream, g, k):
    xuu = np.zeros(3)
    assert lib().hs_dt_gamma_variates(int(key[0]), int(key[1]), int(stream), int(g), int(k), _vp(xuu)) == 0
    return xuu
