"""TEST INFRASTRUCTURE ONLY: ctypes front-end of tests/hostsim_observation_theta/libhostsim_observation_theta.so, which runs the arithmetic of the conjugate
observation step (csrc/observation_theta.h: statistics, both posteriors, draw -- the text the HIP kernels compile) on the CPU.  A plain g++ build.  Never imported
by the product package."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "libhostsim_observation_theta.so")
_SRC = os.path.join(_HERE, "hostsim_observation_theta.cpp")
_CSRC = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "aux_ssm_samplers_amd", "csrc")


def build(force=False):
    deps = [_SRC] + [os.path.join(_CSRC, f) for f in ("observation_theta.h", "dynamics_theta.h", "rng.h", "rng_tables.h", "smallmat.h", "det_math.h",
                                                      "rtc_compat.h")]
    if not force and os.path.exists(_SO) and all(os.path.getmtime(_SO) >= os.path.getmtime(d) for d in deps):
        return _SO
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", _SRC, "-o", _SO])
    return _SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.hs_ot_stats.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.hs_ot_update.argtypes = ([C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_double]
                                      + [C.c_void_p] * 6)
    return _lib


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def num_segments(T):
    return lib().hs_ot_num_segments(int(T))


def stats(x, y):
    """x (T, dx), y (T, dy) -> the FULL statistics [So_zz | S_yz] flat, by ot_accumulate over the observed rows"""
    x, y = np.ascontiguousarray(x, np.float64), np.ascontiguousarray(y, np.float64)
    (T, dx), dy = x.shape, y.shape[1]
    n = dx + 1
    full = np.zeros(n * n + dy * n)
    assert lib().hs_ot_stats(dx, dy, T, _vp(x), _vp(y), _vp(full)) == 0
    return full


def update(dx, full, syy, nobs, M0, K0, nu0, Psi0, chi, ew, ea, mode=1, A0=None, chi_scale=1.0):
    """-> (flag, post flat [M_n | K_n | nu_n | Psi_n], R (dy, dy), A (dy, dx + 1)) by ot_posterior_joint / ot_posterior_r + ot_draw; mode 2: A0 = the fixed [H c],
    returned unchanged"""
    n = dx + 1
    Psi0 = np.ascontiguousarray(Psi0, np.float64)
    dy = Psi0.shape[0]
    M0 = np.ascontiguousarray(M0 if M0 is not None else np.zeros((dy, n)), np.float64)
    K0 = np.ascontiguousarray(K0 if K0 is not None else np.zeros((n, n)), np.float64)
    ea = np.ascontiguousarray(ea if ea is not None else np.zeros((dy, n)), np.float64)
    full, syy, chi, ew = (np.ascontiguousarray(a, np.float64) for a in (full, syy, chi, ew))
    post, R = np.zeros(dy * n + n * n + 1 + dy * dy), np.zeros((dy, dy))
    A = np.zeros((dy, n)) if A0 is None else np.array(A0, np.float64).reshape(dy, n).copy()
    flag = lib().hs_ot_update(dx, dy, int(mode), _vp(full), _vp(syy), float(nobs), _vp(M0), _vp(K0), float(nu0), _vp(Psi0), float(chi_scale), _vp(chi), _vp(ew),
                              _vp(ea), _vp(post), _vp(R), _vp(A))
    assert flag >= 0
    return flag, post, R, A
