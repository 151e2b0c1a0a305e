"""TEST INFRASTRUCTURE ONLY: ctypes front-end of tests/hostsim_smooth/libhostsim_smooth.so, which runs the product's RTS-smoother scan
operator (csrc/kalman_bodies.h::SmoothOp / SmoothOpFly) on the CPU through a chunked host scan.  Never imported by the product package."""
import ctypes as C
import os
import subprocess

import numpy as np

from aux_ssm_samplers_amd import _layout
from aux_ssm_samplers_amd._lib import Arr

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "libhostsim_smooth.so")
_SRC = os.path.join(_HERE, "hostsim_smooth.cpp")
_CSRC = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "aux_ssm_samplers_amd", "csrc")


def build(force=False):
    deps = [_SRC] + [os.path.join(_CSRC, f) for f in ("smallmat.h", "kalman_math.h", "kalman_bodies.h")]
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


def smoothing(ms, Ps, lgssm, E=0, fly=False, dtype=np.float64):
    """ms (T, [B,] dx), Ps (T, [B,] dx, dx) -> (sms, sPs) by SmoothOp over chunks of E elements (0: one chunk, the sequential recursion);
    fly: elements built in every pass by SmoothOpFly instead of being materialised."""
    ms = np.asarray(ms)
    batched = ms.ndim == 3
    T, dx = ms.shape[0], ms.shape[-1]
    B = ms.shape[1] if batched else 1
    desc = _layout.describe_lgssm(list(lgssm[:5]) + [None, None, None], 1, T, B, dx, 1, batched, dtype, False)
    g = (Arr * 8)()
    for i, k in enumerate(_layout.LGSSM_FIELDS):
        if k in desc:
            g[i] = Arr(desc[k].buf.ctypes.data, desc[k].sc, desc[k].st, desc[k].sb)
    msd = np.ascontiguousarray(np.asarray(ms, dtype).reshape(1, T, B, dx))
    Psd = np.ascontiguousarray(np.asarray(Ps, dtype).reshape(1, T, B, dx, dx))
    sms, sPs = np.empty_like(msd), np.empty_like(Psd)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = lib().hs_smooth(0 if np.dtype(dtype) == np.float32 else 1, dx, 1, T, B, g, vp(msd), vp(Psd), int(E), int(bool(fly)), vp(sms), vp(sPs))
    assert rc == 0, rc
    return (sms[0], sPs[0]) if batched else (sms[0, :, 0], sPs[0, :, 0])
