"""TEST INFRASTRUCTURE ONLY: ctypes front-end of tests/hostsim_lgssm_em/libhostsim_lgssm_em.so, which runs the arithmetic of EM for a linear-Gaussian state-space
model (csrc/lgssm_em.h: lag-one covariance, per-step statistics, the three M-step blocks -- the text the HIP kernels compile) on the CPU.  A plain g++ build.
Never imported by the product package."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "libhostsim_lgssm_em.so")
_SRC = os.path.join(_HERE, "hostsim_lgssm_em.cpp")
_CSRC = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "aux_ssm_samplers_amd", "csrc")


def build(force=False):
    deps = [_SRC] + [os.path.join(_CSRC, f) for f in ("lgssm_em.h", "dynamics_theta.h", "rng.h", "rng_tables.h", "smallmat.h", "det_math.h", "rtc_compat.h")]
    if not force and os.path.exists(_SO) and all(os.path.getmtime(_SO) >= os.path.getmtime(d) for d in deps):
        return _SO
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", _SRC, "-o", _SO])
    return _SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        vp = C.c_void_p
        _lib.hs_em_lag_one.argtypes = [C.c_int] + [vp] * 5
        _lib.hs_em_stats.argtypes = [C.c_int, C.c_int, C.c_int] + [vp] * 8
        _lib.hs_em_mstep_dyn.argtypes = [C.c_int, vp, vp, vp, C.c_double, vp, vp, vp]
        _lib.hs_em_mstep_obs.argtypes = [C.c_int, C.c_int, vp, vp, C.c_double, vp, vp]
        _lib.hs_em_mstep_init.argtypes = [C.c_int, C.c_int, vp, C.c_longlong, vp, vp]
    return _lib


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _f64(*arrays):
    return [np.ascontiguousarray(a, np.float64) for a in arrays]


def ns(dx, dy):
    return lib().hs_em_ns(int(dx), int(dy))


def lag_one(F, Q, P, sPn):
    """-> (failed, X (d, d)) by em_lag_one"""
    F, Q, P, sPn = _f64(F, Q, P, sPn)
    d = F.shape[0]
    X = np.zeros((d, d))
    rc = lib().hs_em_lag_one(d, _vp(F), _vp(Q), _vp(P), _vp(sPn), _vp(X))
    assert rc >= 0
    return rc, X


def stats(F, Q, ys, Ps, sms, sPs):
    """one sequence -> (cross (T - 1, d, d), FULL statistics flat), step by step in ascending time"""
    F, Q, ys, Ps, sms, sPs = _f64(F, Q, ys, Ps, sms, sPs)
    T, d = sms.shape
    dy = ys.shape[1]
    cross, full = np.zeros((T - 1, d, d)), np.zeros(ns(d, dy))
    assert lib().hs_em_stats(d, dy, T, _vp(F), _vp(Q), _vp(ys), _vp(Ps), _vp(sms), _vp(sPs), _vp(cross), _vp(full)) == 0
    return cross, full


def mstep_dyn(d, full, prior=None):
    """full: [S_zz | S_xz | S_xx] flat; prior None or (M0, K0, nu0, Psi0) -> (flag, A (d, d + 1), Q (d, d)); A and Q start as NaN"""
    full, = _f64(full)
    A, Q = np.full((d, d + 1), np.nan), np.full((d, d), np.nan)
    if prior is None:
        flag = lib().hs_em_mstep_dyn(d, _vp(full), None, None, 0.0, None, _vp(A), _vp(Q))
    else:
        M0, K0, Psi0 = _f64(prior[0], prior[1], prior[3])
        flag = lib().hs_em_mstep_dyn(d, _vp(full), _vp(M0), _vp(K0), float(prior[2]), _vp(Psi0), _vp(A), _vp(Q))
    assert flag >= 0
    return flag, A, Q


def mstep_obs(d, dy, obs, Syy, nobs):
    """obs: [So_zz | S_yz] flat -> (flag, HC (dy, d + 1), R (dy, dy))"""
    obs, Syy = _f64(obs, Syy)
    HC, R = np.full((dy, d + 1), np.nan), np.full((dy, dy), np.nan)
    flag = lib().hs_em_mstep_obs(d, dy, _vp(obs), _vp(Syy), float(nobs), _vp(HC), _vp(R))
    assert flag >= 0
    return flag, HC, R


def mstep_init(sm0, sP0):
    """sm0 (S, d), sP0 (S, d, d) -> (flag, m0, P0)"""
    sm0, sP0 = _f64(sm0, sP0)
    S, d = sm0.shape
    init = np.ascontiguousarray(np.concatenate([sm0, sP0.reshape(S, d * d)], axis=1))
    m0, P0 = np.zeros(d), np.zeros((d, d))
    flag = lib().hs_em_mstep_init(d, S, _vp(init), d + d * d, _vp(m0), _vp(P0))
    assert flag >= 0
    return flag, m0, P0
