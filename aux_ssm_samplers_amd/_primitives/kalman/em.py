"""Point estimation of a time-invariant LGSSM by EM on the GPU, and the lag-one smoothing covariances its E-step needs.

The reference has neither.  The E-step is `filtering` + `smoothing` plus one statistics pass (include/auxssm.h::auxssm_kalman_smooth_stats: the lag-one
covariances Cov[x_{t+1}, x_t | y] and the expected sufficient statistics of the dynamics and the observations); the M-step is closed form
(auxssm_lgssm_em_mstep).  A fit enqueues filter, smoother, statistics and M-step per iteration without returning to the host."""
import ctypes as C

import numpy as np

from ... import _lib
from .base import LGSSM, DeviceLGSSM, _upload_arr
from .smoothing import MAX_DX, _real_dtype, _smooth_device, _to_host

MAX_DY = 8
NAMES = ("F", "b", "Q", "H", "c", "R", "m0", "P0")
_BLOCKS = ((1, ("F", "b", "Q")), (2, ("H", "c", "R")), (4, ("m0", "P0")))
_FIELD = dict(F="Fs", b="bs", Q="Qs", H="Hs", c="cs", R="Rs", m0="m0", P0="P0")


def _time_invariant(a):
    a = np.asarray(a)
    return a.shape[0] <= 1 or a.strides[0] == 0 or bool(np.all(a == a[:1]))


def _check_sizes(who, T, dx, dy):
    if dx > MAX_DX or dy > MAX_DY:
        raise ValueError(f"{who}: covers the narrow filter's range, dx <= {MAX_DX} and dy <= {MAX_DY} (got dx = {dx}, dy = {dy})")
    if T < 2:
        raise ValueError(f"{who}: needs at least one transition, T >= 2 (got T = {T})")


def _stats_size(dx, dy):
    n = dx + 1
    return 2 * n * n + dx * n + dx * dx + dy * n + dx + dx * dx


def smoothing_lag_one(ys, lgssm, parallel, handle=None):
    """smoothing_lag_one(ys, lgssm, parallel) -> (sms, sPs, cross, ell): `filter_smoothing`'s answers (bit for bit) and the lag-one smoothing covariances
    cross[t] = Cov[x_{t+1}, x_t | y_{0:T-1}], shape (T - 1, dx, dx) -- or (T - 1, B, dx, dx) for batched ys (T, B, dy).

    cross[t] = sPs[t + 1] G_t^T with the smoother's gain G_t = P_t F^T sym(F P_t F^T + Q)^-1, recomputed from the filtered covariances in double.  The dynamics
    must be time-invariant (Fs, Qs, bs broadcast views or equal rows); dx <= 4, dy <= 8, T >= 2."""
    from ... import _layout
    C_, T, B, dx, dy, batched = _layout.infer_dims(ys, lgssm, False)
    _check_sizes("smoothing_lag_one", T, dx, dy)
    lg = list(lgssm)
    for k, name in ((2, "Fs"), (3, "Qs"), (4, "bs")):
        a = np.asarray(lg[k])
        if not _time_invariant(a):
            raise ValueError(f"smoothing_lag_one: {name} varies in time; the lag-one pass covers time-invariant dynamics")
        lg[k] = np.broadcast_to(a[0], a.shape)
    dtype = _real_dtype(ys, *lgssm)
    _layout.describe_lgssm(lg, C_, T, B, dx, dy, batched, dtype, False)
    handle = handle or _lib.default_handle()
    dl = DeviceLGSSM(handle, lg, C_, T, B, dx, dy, batched, dtype)
    ybuf, yarr = _upload_arr(handle, ys, (dy,), C_, T, B, batched, False, dtype, "ys")
    ms, Ps, ell = handle.empty((C_, T, B, dx), dtype), handle.empty((C_, T, B, dx, dx), dtype), handle.empty((C_,), dtype)
    dims = _lib.Dims(C_, T, B, dx, dy)
    code = _lib.dtype_code(dtype)
    _lib.check(handle.lib.auxssm_kalman_filter(handle.h, code, C.byref(dims), C.byref(dl.c), C.byref(yarr), int(bool(parallel)), ms.ptr, Ps.ptr, ell.ptr))
    sms, sPs = _smooth_device(handle, dl, ms, Ps, dims, dtype, parallel)
    cross = handle.empty((C_, T - 1, B, dx, dx), dtype)
    stats = handle.empty((C_ * B, _stats_size(dx, dy)), np.float64)
    _lib.check(handle.lib.auxssm_kalman_smooth_stats(handle.h, code, C.byref(dims), C.byref(dl.c), C.byref(yarr), ms.ptr, Ps.ptr, sms.ptr, sPs.ptr, cross.ptr,
                                                      stats.ptr))
    X = cross.to_host()[0]
    return _to_host(sms, sPs, batched) + (X if batched else X[:, 0], ell.to_host()[0])


class _Fit:
    """The device side of one fit: the model's eight parameter buffers (time and chain stride 0), the data, the moment arrays and the per-iteration outputs, and
    the four calls of an iteration.  Nothing here synchronises with the host."""

    def __init__(self, handle, ys, start, dtype, parallel, n_iter):
        S, T, dy = ys.shape
        dx = np.shape(start["m0"])[-1]
        self.handle, self.dtype, self.code, self.parallel = handle, np.dtype(dtype), _lib.dtype_code(dtype), int(bool(parallel))
        self.S, self.T, self.dx, self.dy = S, T, dx, dy
        self.par = {name: handle.to_device(start[name], dtype) for name in NAMES}
        self.arr = {name: self.par[name].arr(0, 0, 0) for name in NAMES}
        self.lg = _lib.Lgssm()
        for name in NAMES:
            setattr(self.lg, _FIELD[name], self.arr[name])
        self.ybuf = handle.to_device(np.ascontiguousarray(ys, dtype).reshape(S, T, 1, dy))
        self.yarr = self.ybuf.arr(T * dy, dy, 0)
        self.dims = _lib.Dims(S, T, 1, dx, dy)
        self.ms, self.Ps = handle.empty((S, T, 1, dx), dtype), handle.empty((S, T, 1, dx, dx), dtype)
        self.sms, self.sPs = handle.empty((S, T, 1, dx), dtype), handle.empty((S, T, 1, dx, dx), dtype)
        self.stats = handle.empty((S, _stats_size(dx, dy)), np.float64)
        self.ells = handle.zeros((n_iter + 1, S), dtype)
        self.flags = handle.zeros((max(n_iter, 1), 4), np.int32)

    def filter(self, k):
        """ell of this filter -> row k of ells"""
        h, ell_k = self.handle, C.c_void_p(self.ells.ptr.value + k * self.S * self.dtype.itemsize)
        _lib.check(h.lib.auxssm_kalman_filter(h.h, self.code, C.byref(self.dims), C.byref(self.lg), C.byref(self.yarr), self.parallel, self.ms.ptr, self.Ps.ptr,
                                              ell_k))

    def smooth(self):
        h = self.handle
        _lib.check(h.lib.auxssm_kalman_smooth(h.h, self.code, C.byref(self.dims), C.byref(self.lg), self.ms.ptr, self.Ps.ptr, self.parallel, self.sms.ptr,
                                              self.sPs.ptr))

    def statistics(self, cross=None):
        h = self.handle
        _lib.check(h.lib.auxssm_kalman_smooth_stats(h.h, self.code, C.byref(self.dims), C.byref(self.lg), C.byref(self.yarr), self.ms.ptr, self.Ps.ptr,
                                                    self.sms.ptr, self.sPs.ptr, cross.ptr if cross is not None else None, self.stats.ptr))

    def mstep(self, k, syy_c, prior_c, mask):
        """flags of this M-step -> row k of flags"""
        h = self.handle
        _lib.check(h.lib.auxssm_lgssm_em_mstep(h.h, self.code, self.dx, self.dy, self.S, self.stats.ptr, syy_c, C.byref(prior_c) if prior_c is not None else None,
                                               mask, *[C.byref(self.arr[name]) for name in NAMES], C.c_void_p(self.flags.ptr.value + k * 16)))


def _check_update(update):
    update = tuple(update)
    for name in update:
        if name not in NAMES:
            raise ValueError(f"fit_em: unknown parameter {name!r} in update; the names are {NAMES}")
    mask = 0
    for bit, names in _BLOCKS:
        hit = [n in update for n in names]
        if any(hit) and not all(hit):
            raise ValueError(f"fit_em: {names} are one block of the M-step: update all of them or none (got {update})")
        mask |= bit if all(hit) else 0
    return mask


def fit_em(ys, lgssm, n_iter, update=NAMES, prior=None, parallel=True, handle=None):
    """fit_em(ys, lgssm, n_iter) -> (fitted LGSSM, ells (n_iter + 1,), flags (n_iter, 4)): maximum-likelihood (or, with `prior`, maximum a posteriori) estimation
    of a time-invariant LGSSM by EM, started at `lgssm`, every iteration on the device.

    ys (T, dy), or (S, T, dy) for S sequences of ONE model (the sequences ride on the library's chain axis with chain stride 0 on every parameter: they share
    (m0, P0, F, b, Q, H, c, R) and their statistics are pooled -- this is NOT `filtering`'s batch axis B of independent models).  Rows of NaNs are missing steps.
    lgssm: the start, reference shapes, time-invariant (every array with a time axis a broadcast view or equal rows); dx <= 4, dy <= 8, T >= 2.
    update: the parameters the M-step estimates, by block -- ("F", "b", "Q"), ("H", "c", "R"), ("m0", "P0"); a block is updated whole or not at all.
    prior: a loop.MNIWPrior on the dynamics ([F b] and Q go to the joint mode of their matrix-normal inverse-Wishart posterior); needs the dynamics block.
    With the observation block in `update`, a row of ys with some but not all entries NaN is refused (its M-step term is not the one summed here); a fit that
    leaves (H, c, R) alone accepts whatever `filtering` accepts.

    ells[k] is the log-likelihood (summed over the sequences) at the parameters before M-step k, ells[n_iter] that of the fitted model (one final filter); it
    does not decrease.  flags[k] = (dynamics, observations, initial state, 0) of M-step k: 0, or why that block kept its values (include/auxssm.h:
    auxssm_lgssm_em_mstep).  The fitted LGSSM carries broadcast views over time, ready for `filtering` or, as starting values, for loop(..., theta_step=...).
    Filter, smoother, statistics and M-step of all iterations are enqueued without a host synchronisation; ells and flags are read once at the end."""
    from ...loop import MNIWPrior
    ys = np.asarray(ys)
    if ys.ndim == 2:
        ys = ys[None]
    if ys.ndim != 3:
        raise ValueError(f"fit_em: ys must be (T, dy) or (S, T, dy); got shape {ys.shape}")
    S, T, dy = ys.shape
    if len(lgssm) != 8:
        raise ValueError("fit_em: lgssm must be (m0, P0, Fs, Qs, bs, Hs, Rs, cs)")
    dx = np.shape(lgssm[0])[-1]
    mask = _check_update(update)
    n_iter = int(n_iter)
    if n_iter < 0 or S < 1:
        raise ValueError(f"fit_em: needs n_iter >= 0 and at least one sequence (got n_iter = {n_iter}, S = {S})")
    _check_sizes("fit_em", T, dx, dy)
    shapes = dict(m0=(dx,), P0=(dx, dx), Fs=(T - 1, dx, dx), Qs=(T - 1, dx, dx), bs=(T - 1, dx), Hs=(T, dy, dx), Rs=(T, dy, dy), cs=(T, dy))
    model = dict(zip(LGSSM._fields, (np.asarray(a) for a in lgssm)))
    for name, a in model.items():
        if a.shape != shapes[name]:
            raise ValueError(f"fit_em: {name}: expected shape {shapes[name]}, got {a.shape}")
        if name not in ("m0", "P0") and not _time_invariant(a):
            raise ValueError(f"fit_em: {name} varies in time; EM estimates ONE time-invariant model")
    if prior is not None:
        if not isinstance(prior, MNIWPrior):
            raise ValueError("fit_em: prior must be a loop.MNIWPrior")
        if prior.d != dx:
            raise ValueError(f"fit_em: the prior is for d = {prior.d}, the model has dx = {dx}")
        if not mask & 1:
            raise ValueError("fit_em: the prior is on (F, b, Q); it needs the dynamics block in update")
    dtype = _real_dtype(ys, *lgssm)
    ys = np.ascontiguousarray(ys, dtype)
    fin = np.isfinite(ys)
    seen = fin.all(axis=-1)
    if mask & 2 and np.any(fin.any(axis=-1) & ~seen):
        raise ValueError("fit_em: a row of ys is partly NaN; the observation block's M-step covers rows that are observed whole or not at all "
                         "(leave H, c, R out of update, or mask the whole row)")
    y64 = np.where(seen[..., None], ys, 0.0).astype(np.float64).reshape(S * T, dy)
    syy_nobs = np.concatenate([(y64.T @ y64).ravel(), [float(seen.sum())]])

    fit = _Fit(handle or _lib.default_handle(), ys, {name: model[_FIELD[name]] if name in ("m0", "P0") else model[_FIELD[name]][0] for name in NAMES}, dtype,
               parallel, n_iter)
    syy_c = (C.c_double * len(syy_nobs))(*[float(v) for v in syy_nobs])
    prior_c = prior.struct(1.0) if prior is not None else None
    for k in range(n_iter):
        fit.filter(k)
        fit.smooth()
        fit.statistics()
        fit.mstep(k, syy_c, prior_c, mask)
    fit.filter(n_iter)
    par, ells, flags = fit.par, fit.ells, fit.flags
    out = {name: par[name].to_host() for name in NAMES}
    bt = np.broadcast_to
    fitted = LGSSM(out["m0"], out["P0"], bt(out["F"], shapes["Fs"]), bt(out["Q"], shapes["Qs"]), bt(out["b"], shapes["bs"]), bt(out["H"], shapes["Hs"]),
                   bt(out["R"], shapes["Rs"]), bt(out["c"], shapes["cs"]))
    return fitted, ells.to_host().astype(np.float64).sum(axis=1), flags.to_host()[:n_iter]
