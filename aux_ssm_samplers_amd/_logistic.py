"""What the two samplers' binomial / negative-binomial models share (kalman.BinomialModel / NegBinomialModel, csmc.BinomialPotential / NegBinomialPotential):
the data rules and the SIZE m of the one logistic potential  log g = sum_k [y_k x_k - m_k softplus(x_k)]  over the finite y_k.

    binomial            m = trials           finite y in [0, trials], trials > 0
    negative binomial   m = y + r            finite y >= 0, r > 0

A NaN y is a missing observation: its size is never looked at (it may be anything; the cSMC side stores 0 there)."""
import numpy as np


def per_observation(a, shape, name):
    """a scalar, (dx,) or (T, dx) parameter as a (T, dx) float64 array"""
    a = np.asarray(a, np.float64)
    if a.ndim > 2 or (a.ndim == 2 and a.shape != shape) or (a.ndim == 1 and a.shape != shape[1:]):
        raise ValueError(f"{name} must be a scalar, ({shape[1]},) or {shape}, got shape {a.shape}")
    return np.array(np.broadcast_to(a, shape))


def binomial_size(ys, trials, who):
    """the (T, dx) trials of binomial data ys (T, dx), validated; who: the class named in the messages"""
    yv = np.asarray(ys, np.float64)
    n = per_observation(trials, yv.shape, f"{who}: trials")
    seen = np.isfinite(yv)
    if np.any(seen & ~np.isfinite(n)):
        raise ValueError(f"{who}: trials must be finite wherever y is observed")
    if np.any(n[np.isfinite(n)] <= 0):
        raise ValueError(f"{who}: trials must be > 0; got a minimum of {float(np.nanmin(n))}")
    if np.any(seen & ((yv < 0) | (yv > np.where(seen, n, np.inf)))):
        raise ValueError(f"{who}: every observed y must lie in [0, trials]")
    return n


def negbinomial_r(ys, r, who):
    """the (T, dx) dispersion r of negative-binomial counts ys (T, dx), validated (the potential's size is ys + r); who: the class named in the messages"""
    yv = np.asarray(ys, np.float64)
    rr = per_observation(r, yv.shape, f"{who}: r")
    seen = np.isfinite(yv)
    if np.any(seen & ~np.isfinite(rr)):
        raise ValueError(f"{who}: r must be finite wherever y is observed")
    if np.any(rr[np.isfinite(rr)] <= 0):
        raise ValueError(f"{who}: r must be > 0; got a minimum of {float(np.nanmin(rr))}")
    if np.any(yv[seen] < 0):
        raise ValueError(f"{who}: counts must be >= 0 or NaN (missing); got a minimum of {float(np.nanmin(yv))}")
    return rr


def log_g(x, y, m):
    """the NumPy formula, batched over the leading axes of x: sum_k [y_k x_k - m_k softplus(x_k)] over the finite y_k, softplus(x) = max(x, 0) + log1p(exp(-|x|))"""
    x, y, m = np.asarray(x, np.float64), np.asarray(y, np.float64), np.asarray(m, np.float64)
    with np.errstate(invalid="ignore"):
        v = y * x - m * (np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x))))
    return np.sum(np.where(np.isfinite(y), v, 0.0), axis=-1)
