"""TEST INFRASTRUCTURE ONLY: ctypes front-end of tests/hostsim_chain_dynamics/libhostsim_chain_dynamics.so, which runs the per-chain body of
auxssm_csmc_dynamics_commit (csrc/chain_dynamics.h -- the text the HIP kernel compiles) on the CPU.  A plain g++ build.  Never imported by the product package."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "libhostsim_chain_dynamics.so")
_SRC = os.path.join(_HERE, "hostsim_chain_dynamics.cpp")
_CSRC = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "aux_ssm_samplers_amd", "csrc")


def build(force=False):
    deps = [_SRC] + [os.path.join(_CSRC, f) for f in ("chain_dynamics.h", "dynamics_theta.h", "rng.h", "rng_tables.h", "smallmat.h", "det_math.h", "rtc_compat.h")]
    if not force and os.path.exists(_SO) and all(os.path.getmtime(_SO) >= os.path.getmtime(d) for d in deps):
        return _SO
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", _SRC, "-o", _SO])
    return _SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.hs_cd_commit.argtypes = [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 9
    return _lib


def commit(F_new, b_new, Q_new, step_flags, F, b, Q, chol_Q):
    """cd_commit chain by chain on arrays of one dtype (float32 / float64): staging (C, d, d), (C, d), (C, d, d) and step_flags (C,) ->
    (F, b, Q, chol_Q, flags) -- copies of the live arrays after the commit, and its codes"""
    dtype = np.dtype(np.asarray(F).dtype)
    assert dtype in (np.dtype(np.float32), np.dtype(np.float64))
    stage = [np.ascontiguousarray(a, dtype) for a in (F_new, b_new, Q_new)]
    live = [np.array(a, dtype, order="C") for a in (F, b, Q, chol_Q)]
    Cn, d = live[1].shape
    sf = np.ascontiguousarray(step_flags, np.int32)
    flags = np.full(Cn, -1, np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib().hs_cd_commit(0 if dtype == np.float32 else 1, Cn, d, *(vp(a) for a in stage), vp(sf), *(vp(a) for a in live), vp(flags)) == 0
    return (*live, flags)
