"""Smoothing marginals of an LGSSM (Rauch-Tung-Striebel) on the GPU: E[x_t | y_{0:T-1}] and Cov[x_t | y_{0:T-1}].

The reference has no smoother of its own -- its tests compare the pathwise sampler with `explicit_kalman_smoothing`
(test_kalman/common.py:5-24); this is that recursion as a backward associative scan built from the sampler's gain
(sampling.py:86-98), see include/auxssm.h::auxssm_kalman_smooth."""
import ctypes as C

import numpy as np

from ... import _layout, _lib
from .base import DeviceLGSSM, _common_dtype, _upload_arr

MAX_DX = 4


def _check_moments(ms, Ps):
    """(T, B, dx, batched) of filtered moments ms (T, [B,] dx), Ps (T, [B,] dx, dx); raises before any device is touched."""
    ms_shape, Ps_shape = np.shape(ms), np.shape(Ps)
    if len(ms_shape) not in (2, 3):
        raise ValueError(f"ms must be (T, [B,] dx); got shape {ms_shape}")
    if Ps_shape != ms_shape + ms_shape[-1:]:
        raise ValueError(f"Ps: expected shape {ms_shape + ms_shape[-1:]} to go with ms {ms_shape}, got {Ps_shape}")
    batched = len(ms_shape) == 3
    T, dx = ms_shape[0], ms_shape[-1]
    if T < 1 or dx < 1:
        raise ValueError(f"ms must hold at least one time step and one component; got shape {ms_shape}")
    _check_dx(dx)
    return T, (ms_shape[1] if batched else 1), dx, batched


def _check_dx(dx):
    if dx > MAX_DX:
        raise NotImplementedError(f"the smoother is instantiated for dx <= {MAX_DX} (dx = {dx}); sampling() covers wide states")


def _real_dtype(*arrays):
    """float32 / float64 working type of real-valued inputs (as _common_dtype), refusing anything else"""
    for a in arrays:
        dt = np.asarray(a).dtype
        if dt.kind not in "fiub":
            raise ValueError(f"arrays must be real-valued, got dtype {dt}")
    return _common_dtype(*arrays)


def _smooth_device(handle, dl, msd, Psd, dims, dtype, parallel):
    sms = handle.empty(msd.shape, dtype)
    sPs = handle.empty(Psd.shape, dtype)
    _lib.check(handle.lib.auxssm_kalman_smooth(handle.h, _lib.dtype_code(dtype), C.byref(dims), C.byref(dl.c),
                                                msd.ptr, Psd.ptr, int(bool(parallel)), sms.ptr, sPs.ptr))
    return sms, sPs


def _to_host(sms, sPs, batched):
    sm, sP = sms.to_host()[0], sPs.to_host()[0]
    return (sm, sP) if batched else (sm[:, 0], sP[:, 0])


def smoothing(ms, Ps, lgssm, parallel, handle=None):
    """smoothing(ms, Ps, lgssm, parallel) -> (sms, sPs): the smoothing means and covariances from the filtered moments of `filtering`.

    ms (T, dx), Ps (T, dx, dx) or batched (T, B, dx), (T, B, dx, dx); of `lgssm` only Fs, Qs, bs are read.  parallel=True runs the
    backward associative scan, False the same kernels as one chunk per sequence, i.e. the sequential recursion.  dx <= 4."""
    T, B, dx, batched = _check_moments(ms, Ps)
    dtype = _real_dtype(ms, Ps, *lgssm[:5])
    lg = list(lgssm[:5]) + [None, None, None]
    _layout.describe_lgssm(lg, 1, T, B, dx, 1, batched, dtype, False)  # shape errors of the model before a handle is taken
    handle = handle or _lib.default_handle()
    dl = DeviceLGSSM(handle, lg, 1, T, B, dx, 1, batched, dtype)
    msd = handle.to_device(np.asarray(ms, dtype).reshape(1, T, B, dx))
    Psd = handle.to_device(np.asarray(Ps, dtype).reshape(1, T, B, dx, dx))
    sms, sPs = _smooth_device(handle, dl, msd, Psd, _lib.Dims(1, T, B, dx, 1), dtype, parallel)
    return _to_host(sms, sPs, batched)


def filter_smoothing(ys, lgssm, parallel, handle=None):
    """filter_smoothing(ys, lgssm, parallel) -> (sms, sPs, ell): `filtering` then `smoothing` with the filtered moments kept on the device.

    ys (T, dy) or batched (T, B, dy); NaN entries are missing observations, as in `filtering`; ell is the filter's marginal log-likelihood."""
    C_, T, B, dx, dy, batched = _layout.infer_dims(ys, lgssm, False)
    _check_dx(dx)
    dtype = _real_dtype(ys, *lgssm)
    _layout.describe_lgssm(lgssm, C_, T, B, dx, dy, batched, dtype, False)
    handle = handle or _lib.default_handle()
    dl = DeviceLGSSM(handle, lgssm, C_, T, B, dx, dy, batched, dtype)
    ybuf, yarr = _upload_arr(handle, ys, (dy,), C_, T, B, batched, False, dtype, "ys")
    ms = handle.empty((C_, T, B, dx), dtype)
    Ps = handle.empty((C_, T, B, dx, dx), dtype)
    ell = handle.empty((C_,), dtype)
    dims = _lib.Dims(C_, T, B, dx, dy)
    _lib.check(handle.lib.auxssm_kalman_filter(handle.h, _lib.dtype_code(dtype), C.byref(dims), C.byref(dl.c),
                                                C.byref(yarr), int(bool(parallel)), ms.ptr, Ps.ptr, ell.ptr))
    sms, sPs = _smooth_device(handle, dl, ms, Ps, dims, dtype, parallel)
    return _to_host(sms, sPs, batched) + (ell.to_host()[0],)
