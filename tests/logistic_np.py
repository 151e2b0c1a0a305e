"""The logistic potential (AUXSSM_POT_LOGISTIC: binomial and negative-binomial counts with a logit link) for the literal NumPy cSMC (tests/potential_np.py on
oracle/csmc_np.py, oracle/pit_np.py, tests/guided_np.py) and the cases the tests of this potential share.  Test infrastructure only, written independently of the
package:

    log g_t(x) = sum_k [ y_{t,k} x_k - m_{t,k} softplus(x_k) ]   over the components whose y_{t,k} is finite (the combinatorial constant left out)

with m = the trials (binomial) or y + r (negative binomial), softplus = np.logaddexp(0, x) and a masked np.sum -- neither the kernels' det_exp / det_log nor
their fused multiply-add: agreement is to rounding.

The data of every case contain a missing entry, a wholly missing row, y = 0, y = size's upper end (y = trials) and a size of 1 (binary data; for the negative
binomial family r = 1 under y = 0).  Sizes stay <= 40 here (the fp64 tolerances of the literal comparison are the Poisson tests', valid at such sizes)."""
import functools

import numpy as np

from oracle import csmc_np as L
from tests import pit_cases as PC
from tests import potential_np as P

FAMILIES = ("binomial", "negbinomial")


def log_g(x, y, m):
    x, y, m = np.asarray(x, np.float64), np.asarray(y, np.float64), np.asarray(m, np.float64)
    with np.errstate(invalid="ignore"):
        v = y * np.atleast_2d(x) - m * np.logaddexp(0.0, np.atleast_2d(x))
    v = np.sum(np.where(np.isfinite(y), v, 0.0), axis=-1)
    return v if x.ndim > 1 else v[0]


def grad_log_g(x, y, m):
    """d log g / dx_k = y_k - m_k sigma(x_k); 0 for a missing component"""
    x, y, m = np.asarray(x, np.float64), np.asarray(y, np.float64), np.asarray(m, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(y), y - m * np.exp(x - np.logaddexp(0.0, x)), 0.0)


def bound(y, m):
    """sup_x log g: the binomial log-likelihood at p = y / m, sum_k [y log(y / m) + (m - y) log((m - y) / m)] with 0 log 0 = 0, over the finite y_k"""
    y, m = np.asarray(y, np.float64), np.asarray(m, np.float64)
    ok = np.isfinite(y)
    ys, ms = np.where(ok, y, 0.0), np.where(ok, m, 1.0)
    a = np.where(ys > 0, ys * np.log(np.where(ys > 0, ys, 1.0) / ms), 0.0)
    n = ms - ys
    c = np.where(n > 0, n * np.log(np.where(n > 0, n, 1.0) / ms), 0.0)
    return float(np.sum(np.where(ok, a + c, 0.0)))


def softplus_device_order(x, dtype):
    """the kernels' softplus in NumPy at precision dtype: e = exp(-|x|), l = log(1 + e) (the sum rounded first: there is no log1p), max(x, 0) + l"""
    x = np.asarray(x, dtype)
    e = np.exp(-np.abs(x))
    return np.maximum(x, dtype(0)) + np.log(dtype(1) + e)


def split(row):
    """a parameter row [y | m] of width 2 d -> (y, m)"""
    d = row.shape[-1] // 2
    return row[..., :d], row[..., d:]


def potential(y, m, first=False):
    """g_t as a protocol object of oracle/csmc_np.py: of the rows [y | m][1:] or (first) of the row [y_0 | m_0]"""
    return P.RowPotential(KIND, np.concatenate([np.asarray(y), np.asarray(m)], axis=-1), (), first)


def scalar_steps(y, size):
    """log g_t(x) = y_t x - size_t softplus(x) of the scalar model for tests/potential_np.py::posterior_by_quadrature (NaN y_t: not observed)"""
    return [functools.partial(log_g, y=[a], m=[b]) for a, b in zip(np.asarray(y, np.float64).reshape(-1), np.asarray(size, np.float64).reshape(-1))]


# ---- cases: the model on both sides ---------------------------------------------------------------------------------------------------------------------
def build(m0, P0, F, b, Q, y, family, par):
    """(device objects (M0, G0, Mt, Gt), literal Model with size = m (T, d)) of one model; par: the trials (T, d) (binomial) or r (T, d) (negative binomial)"""
    from aux_ssm_samplers_amd import csmc
    T = y.shape[0]
    M0, Mt = csmc.GaussianInit(m0=m0, P0=P0), csmc.LinearGaussianDynamics(F=F, b=b, Q=Q)
    if family == "binomial":
        dev = (M0, csmc.BinomialPotential(par[0], y=y[0]), Mt, csmc.BinomialPotential(par[1:], params=y[1:]))
        size = par
    else:
        dev = (M0, csmc.NegBinomialPotential(par[0], y=y[0]), Mt, csmc.NegBinomialPotential(par[1:], params=y[1:]))
        size = y + par
    size = np.where(np.isfinite(y), size, 0.0)
    return dev, P.Model(KIND, m0, P0, L.LinearGaussianDynamics(F, b, np.linalg.cholesky(Q), T), Q, np.concatenate([y, size], axis=1), size=size)


def case(d, T, rng, family="binomial", nan_steps=()):
    """tests/potential_np.py::dynamics around log-odds 0, observed as binomial counts (trials drawn from 1 .. 40, component 0 binary) or negative-binomial counts
    (r drawn from {0.5, 1, 3}, r = 1 in component 0).  The first two steps outside nan_steps are set to y = 0 and to y = trials (negative binomial: to y = 0 twice)
    in component 0, whose size is 1 there.  nan_steps: up to three time steps with missing data (tests/potential_np.py::knock_out).  Returns (device objects
    (M0, G0, Mt, Gt), literal Model, a trajectory, delta in [0.1, 0.4] / d)."""
    assert family in FAMILIES
    m0, P0, F, b, Q = P.dynamics(d, rng)
    x = P.trajectory(m0, P0, F, b, Q, T, rng)
    free = [t for t in range(T) if t not in nan_steps][:2]
    if family == "binomial":
        par = rng.integers(1, 41, size=(T, d)).astype(np.float64)
        par[:, 0] = 1.0
        y = rng.binomial(par.astype(np.int64), 1.0 / (1.0 + np.exp(-x))).astype(np.float64)
        y[free[0], 0], y[free[1], 0] = 0.0, par[free[1], 0]
    else:
        par = rng.choice([0.5, 1.0, 3.0], size=(T, d))
        par[:, 0] = 1.0
        y = np.minimum(rng.poisson(rng.gamma(par, np.exp(x))), 30).astype(np.float64)  # (sizes y + r stay <= 40)
        y[free[0], 0] = y[free[1], 0] = 0.0
    P.knock_out(y, nan_steps)
    dev, m = build(m0, P0, F, b, Q, y, family, par)
    return dev, m, x, (0.1 + 0.3 * rng.random(T)) / d


def has_every_feature(m):
    """the data of a case: a missing entry, a wholly missing row, y = 0, y = the size's upper end or (negative binomial) size = r, and a size of 1"""
    y, s = m.y, m.size
    ok = np.isfinite(y)
    return bool((~ok).any() and (~ok).all(axis=1).any() and (y[ok] == 0).any() and (s[ok] == 1).any() and (s[ok] <= 40).all() and (s[ok] > 0).all())


def program(dev, grad=False):
    """the same model with the potential as user source (device_models.BUILTIN_LOGISTIC: value, bound and gradient in one source; no theta) over rows [y | m],
    p = 2 d"""
    from aux_ssm_samplers_amd.csmc import DevicePotential, device_models as U
    M0, G0, Mt, Gt = dev
    d = int(np.size(G0.y))
    r0 = np.concatenate([np.reshape(G0.y, (1, d)), G0.sizes()], axis=1)[0]
    rt = np.concatenate([np.reshape(Gt.params, (-1, d)), Gt.sizes()], axis=1)
    return M0, DevicePotential(U.BUILTIN_LOGISTIC, y=r0, p=2 * d), Mt, DevicePotential(U.BUILTIN_LOGISTIC, params=rt, p=2 * d)


# ---- the cases of tests/test_gpu_logistic.py, shared with the CPU tests that vouch for them (well-posedness of the ancestor comparison) -------------------------
PROGRAM_SHAPES = [(d, N) for d in (1, 2, 4) for N in (64, 100, 1024)]  # (d, N) at T = 40, 3 chains
PROGRAM_T, PROGRAM_CHAINS = 40, 3
REGISTER = [(d, N, 33) for d in (1, 3) for N in (64, 100)]       # (d, N, T)
WIDE = [(d, N, 25) for d in (5, 13, 32) for N in (25, 64)]
PIT_CELLS = ((1, 32, 25), (3, 100, 33), (1, 100, 25), (6, 25, 25), (13, 32, 33))  # (d, N, T): three register cells, two wide ones


def family_of(shape):
    """the family of a literal or tree shape: the two alternate over the shapes of every group, so that every sampler style meets both"""
    shapes = REGISTER + WIDE + [c for c in PIT_CELLS if c not in REGISTER + WIDE]
    return FAMILIES[shapes.index(tuple(shape)) % 2]


def _literal_model(shape, rng):
    """NaN entries at t = 0 (one component), mid-series (the whole row) and T - 1 (all but the last component)"""
    d, N, T = shape
    return shape + case(d, T, rng, family_of(shape), nan_steps=(0, T // 2, T - 1))


def _pit_model(cell, rng):
    """missing data at t = 0 (one component), on the top-level stitch boundary (the whole row) and at the last step (all but the last component)"""
    d, N, T = cell
    return cell + case(d, T, rng, family_of(cell), nan_steps=(0, PC.top_boundary(T), T - 1))


KIND = P.Kind("logistic", 8, log_g, grad_log_g, split=split, cells=lambda style, gradient, backward: REGISTER + WIDE, literal_model=_literal_model,
              seeds=lambda style, gradient, backward, shape: ([8000 + P.seed_index(style, gradient, backward), *shape, bump] for bump in range(P.MAX_BUMPS)),
              label=lambda shape: "{} d={} N={} T={}".format(family_of(shape), *shape),
              pit_cells=PIT_CELLS, pit_model=_pit_model, pit_seeds=lambda cell, gradient: ([19, *cell, int(gradient), bump] for bump in range(P.MAX_BUMPS)),
              program=program)
