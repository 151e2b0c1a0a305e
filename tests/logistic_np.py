"""The logistic potential (AUXSSM_POT_LOGISTIC: binomial and negative-binomial counts with a logit link) as GENERIC protocol objects for the literal NumPy cSMC
(oracle/csmc_np.py, oracle/pit_np.py, tests/guided_np.py), the cases the tests of this potential share, and the posterior of the scalar model by quadrature.
Test infrastructure only, written independently of the package (the arrangement of tests/poisson_np.py):

    log g_t(x) = sum_k [ y_{t,k} x_k - m_{t,k} softplus(x_k) ]   over the components whose y_{t,k} is finite (the combinatorial constant left out)

with m = the trials (binomial) or y + r (negative binomial), softplus = np.logaddexp(0, x) and a masked np.sum -- neither the kernels' det_exp / det_log nor
their fused multiply-add: agreement is to rounding.

The data of every case contain a missing entry, a wholly missing row, y = 0, y = size's upper end (y = trials) and a size of 1 (binary data; for the negative
binomial family r = 1 under y = 0).  Sizes stay <= 40 here (the fp64 tolerances of the literal comparison are the Poisson tests', valid at such sizes)."""
import functools

import numpy as np

from oracle import csmc_np as L
from tests import guided_np as G
from tests import pit_cases as PC

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


class LogisticPotential:
    """g_t as a `Potential` with params = [y | m][1:] (rows of 2 d) and as the `UnivariatePotential` of row 0 (oracle.csmc_np.ObsPotential's two roles)"""

    def __init__(self, y, m, first=False):
        self.first = first
        self.params = None if first else np.concatenate([np.asarray(y), np.asarray(m)], axis=1)
        self.y0, self.m0 = (np.asarray(y), np.asarray(m)) if first else (None, None)

    def __call__(self, *a):
        if self.first:
            return log_g(a[0], self.y0, self.m0)
        d = a[2].shape[-1] // 2
        return log_g(a[0], a[2][..., :d], a[2][..., d:])


class Model(G.Model):
    """tests/guided_np.py's model record with this potential (time-invariant transitions); size: m (T, d)"""

    def __init__(self, m0, P0, dyn, Q, y, size):
        super().__init__(m0, P0, dyn, Q, LogisticPotential(y[0], size[0], first=True), LogisticPotential(y[1:], size[1:]), "logistic", y)
        self.size = size
        self.F, self.b = np.asarray(dyn.params[0][0], float), np.asarray(dyn.params[1][0], float)

    def literal(self):
        """(M0, G0, Mt, Gt) of the literal sampler"""
        return L.GaussianInit(self.m0, self.LP0), self.G0, self.dyn, self.Gt


def pot_grad(m, u):
    return np.stack([grad_log_g(u[t], m.y[t], m.size[t]) for t in range(u.shape[0])])


def joint_grad(m, u):
    """the gradient at u (T, d) of log M0(u_0) + G0(u_0) + sum_t [log Mt(u_{t+1} | u_t) + Gt(u_{t+1})] (csmc/independent.py:121-134), in closed form"""
    T = u.shape[0]
    g = pot_grad(m, u)
    g[0] -= np.linalg.solve(m.P0, u[0] - m.m0)
    for t in range(1, T):
        w = np.linalg.solve(m.Q, u[t] - (m.F @ u[t - 1] + m.b))
        g[t] -= w
        g[t - 1] += m.F.T @ w
    return g


def guided_kernel(m, N, backward=False, gradient=False):
    """the literal guided sampler of tests/guided_np.py; its gradient variant shifts u by s^2 grad log g_t(u_t)"""
    def f(u, scale):
        T = u.shape[0]
        tab = [G.tables(m.P0 if t == 0 else m.Q, float(scale[t])) for t in range(T)]
        Ks, Cs = np.stack([a for a, _ in tab]), np.stack([b for _, b in tab])
        ut = u + (scale * scale)[:, None] * pot_grad(m, u) if gradient else u
        return (G.GuidedM0(m, ut[0], Ks[0], Cs[0]), G.GuidedG0(m, u[0], scale[0], ut[0], Ks[0], Cs[0]),
                G.GuidedMt(m, (ut[1:], Ks[1:], Cs[1:], m.dyn.params)),
                G.GuidedGt(m, (u[1:], scale[1:], ut[1:], Ks[1:], Cs[1:], m.dyn.params, m.Gt.params)))
    return L.get_generic_kernel(f, N, backward, m.dyn)


def independent_kernel(m, N, backward=False, gradient=False):
    """oracle.csmc_np.get_independent_kernel on this model; gradient: False, True (the reference's weighting) or "exact", with joint_grad for jax.grad"""
    M0, G0, Mt, Gt = m.literal()
    if not gradient:
        return L.get_independent_kernel(M0, G0, Mt, Gt, N, backward=backward, Pt=Mt)

    def f(u, scale):
        gp = joint_grad(m, u)
        return (L.AuxiliaryM0(u[0], scale[0], gp[0]), L.GradientAuxiliaryG0(M0, G0, u[0], scale[0], gp[0]),
                L.AuxiliaryMtDynamics((u[1:], scale[1:], gp[1:])), L.GradientAuxiliaryGt(Mt, Gt, (u[1:], scale[1:], gp[1:]), gradient == "exact"))
    return L.get_generic_kernel(f, N, backward, Mt)


def bootstrap_kernel(m, N, backward=False):
    M0, G0, Mt, Gt = m.literal()
    return L.get_kernel(M0, G0, Mt, Gt, N, backward=backward, Pt=Mt)


def posterior_by_quadrature(y, size, m0, P0, F, Q, b, n=1601, width=9.0):
    """(T, 2): posterior mean and variance of every x_t of the SCALAR model x_0 ~ N(m0, P0), x_t ~ N(F x_{t-1} + b, Q), log g_t(x) = y_t x - size_t softplus(x)
    (NaN y_t: not observed), by a forward-backward pass on one uniform grid that covers the prior marginals of all steps by `width` standard deviations (the
    likelihood only narrows them): tests/poisson_np.py::posterior_by_quadrature with this potential.  Independent of every sampler and oracle."""
    y, size = np.asarray(y, np.float64).reshape(-1), np.asarray(size, np.float64).reshape(-1)
    m0, P0, F, Q, b = (float(np.reshape(a, -1)[0]) for a in (m0, P0, F, Q, b))
    T = y.shape[0]
    mu, var, lo, hi = m0, P0, np.inf, -np.inf
    for t in range(T):
        if t > 0:
            mu, var = F * mu + b, F * F * var + Q
        lo, hi = min(lo, mu - width * np.sqrt(var)), max(hi, mu + width * np.sqrt(var))
    g = np.linspace(lo, hi, n)
    assert g[1] - g[0] < 0.05 * np.sqrt(min(Q, P0))
    lg = np.stack([np.zeros(n) if not np.isfinite(y[t]) else y[t] * g - size[t] * np.logaddexp(0.0, g) for t in range(T)])
    tr = np.exp(-0.5 * (g[None, :] - (F * g[:, None] + b)) ** 2 / Q)  # [x, x']

    def nrm(v):
        return v / v.sum()
    alpha = [nrm(np.exp(-0.5 * (g - m0) ** 2 / P0 + lg[0] - lg[0].max()))]
    for t in range(1, T):
        alpha.append(nrm((alpha[-1] @ tr) * np.exp(lg[t] - lg[t].max())))
    beta = [np.ones(n)]
    for t in range(T - 1, 0, -1):
        beta.append(nrm(tr @ (beta[-1] * np.exp(lg[t] - lg[t].max()))))
    beta = beta[::-1]
    out = []
    for t in range(T):
        p = nrm(alpha[t] * beta[t])
        assert p[0] < 1e-12 and p[-1] < 1e-12  # the grid holds the posterior
        mean = float(p @ g)
        out.append((mean, float(p @ (g - mean) ** 2)))
    return np.array(out)


# ---- cases: the model on both sides ---------------------------------------------------------------------------------------------------------------------
def build(m0, P0, F, b, Q, y, family, par):
    """(device objects (M0, G0, Mt, Gt), literal Model) of one model; par: the trials (T, d) (binomial) or r (T, d) (negative binomial)"""
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
    return dev, Model(m0, P0, L.LinearGaussianDynamics(F, b, np.linalg.cholesky(Q), T), Q, y, size)


def case(d, T, rng, family="binomial", nan_steps=()):
    """tests/guided_np.py::sv_case's linear-Gaussian dynamics around log-odds 0, observed as binomial counts (trials drawn from 1 .. 40, component 0 binary) or
    negative-binomial counts (r drawn from {0.5, 1, 3}, r = 1 in component 0).  The first two steps outside nan_steps are set to y = 0 and to y = trials
    (negative binomial: to y = 0 twice) in component 0, whose size is 1 there.  nan_steps: up to three time steps with missing data -- the first loses
    component 0, the second its WHOLE row, the third every component but the last (for d >= 2 a row that is partly NaN; d = 1: its only component).  Returns
    (device objects (M0, G0, Mt, Gt), literal Model, a trajectory, delta in [0.1, 0.4] / d)."""
    assert family in FAMILIES
    F = 0.9 * np.eye(d) + 0.02 * rng.standard_normal((d, d)) / np.sqrt(d)
    b = 0.05 * rng.standard_normal(d)
    Q, P0, m0 = G.spd(d, rng), G.spd(d, rng, 0.5), 0.1 * rng.standard_normal(d)
    x = np.zeros((T, d))
    x[0] = m0 + np.linalg.cholesky(P0) @ rng.standard_normal(d)
    for t in range(1, T):
        x[t] = F @ x[t - 1] + b + np.linalg.cholesky(Q) @ rng.standard_normal(d)
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
    for i, t in enumerate(nan_steps):
        if i % 3 == 0:
            y[t, 0] = np.nan
        elif i % 3 == 1:
            y[t, :] = np.nan
        else:
            y[t, :max(d - 1, 1)] = np.nan
    dev, m = build(m0, P0, F, b, Q, y, family, par)
    return dev, m, x, (0.1 + 0.3 * rng.random(T)) / d


def has_every_feature(m):
    """the data of a case: a missing entry, a wholly missing row, y = 0, y = the size's upper end or (negative binomial) size = r, and a size of 1"""
    y, s = m.y, m.size
    ok = np.isfinite(y)
    return bool((~ok).any() and (~ok).all(axis=1).any() and (y[ok] == 0).any() and (s[ok] == 1).any() and (s[ok] <= 40).all() and (s[ok] > 0).all())


def program(dev):
    """the same model with the potential as user source (device_models.BUILTIN_LOGISTIC: value, bound and gradient; no theta) over rows [y | m], p = 2 d"""
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
LITERAL_CELLS = ([("independent", g, bw) for g in (False, True, "exact") for bw in (False, True)]
                 + [("guided", g, bw) for g in (False, True) for bw in (False, True)]
                 + [("bootstrap", False, bw) for bw in (False, True)])
GAP_BAR = 1e-8  # tests/test_lingauss_potential.py's bar on the smallest distance of a draw from a cumulative-weight edge
MAX_BUMPS = 32


def family_of(shape):
    """the family of a literal or tree shape: the two alternate over the shapes of every group, so that every sampler style meets both"""
    shapes = REGISTER + WIDE + [c for c in PIT_CELLS if c not in REGISTER + WIDE]
    return FAMILIES[shapes.index(tuple(shape)) % 2]


def _seed(style, gradient, backward, shape, bump):
    si = dict(independent=0, guided=1, bootstrap=2)[style]
    gi = {False: 0, True: 1, "exact": 2}[gradient]
    d, N, T = shape
    return [8000 + 1000 * si + 100 * gi + 50 * int(backward), d, N, T, bump]


def literal_case(shape, seed):
    """(d, N, T, device objects, Model, reference trajectory, delta, noise) of one literal case: NaN entries at t = 0 (one component), mid-series (the whole
    row) and T - 1 (all but the last component)"""
    d, N, T = shape
    rng = np.random.default_rng(seed)
    dev, m, xtrue, delta = case(d, T, rng, family_of(shape), nan_steps=(0, T // 2, T - 1))
    x0 = xtrue + 0.3 * rng.standard_normal((T, d))
    nz = dict(eps_aux=rng.standard_normal((T, d)), eps_prop=rng.standard_normal((T, N, d)), u_res=rng.random((T - 1, N)), u_bwd=rng.random(T))
    return d, N, T, dev, m, x0, delta, nz


def _sweep(style, gradient, backward, shape, bump):
    cs = literal_case(shape, _seed(style, gradient, backward, shape, bump))
    d, N, T, dev, m, x0, delta, nz = cs
    nz = dict(nz)
    if style == "bootstrap":
        nz.pop("eps_aux")
        return bootstrap_kernel(m, N, backward)[1](L.Noise(**nz), x0), cs
    if style == "guided":
        return guided_kernel(m, N, backward, gradient)[1](L.Noise(**nz), x0, delta), cs
    return independent_kernel(m, N, backward, gradient)[1](L.Noise(**nz), x0, delta), cs


def _gap(out, cs, backward):
    """the smallest distance of a resampling or backward draw r = c[-1] (1 - u) from a cumulative-weight edge c[j] (weights normalised to sum 1):
    tests/lingauss_np.py::wellposedness's gap"""
    (x, B, h), (d, N, T, dev, m, x0, delta, nz) = out, cs

    def gap(w, u):
        c = np.cumsum(w)
        r = c[-1] * (1 - np.atleast_1d(u))
        return float(np.min(np.abs(r[:, None] - c[None, :])))
    gaps = [gap(L.normalize(h["log_ws"][t]), nz["u_res"][t][1:]) for t in range(T - 1)]
    gaps.append(gap(h["w_T"], nz["u_bwd"][T - 1]))
    if backward:
        for t in range(T - 2, -1, -1):
            lw = m.dyn.logpdf(x[t + 1], h["xs"][t], L._tree_index(m.dyn.params, t)) + h["log_ws"][t]
            gaps.append(gap(L.normalize(lw), nz["u_bwd"][t]))
    return min(gaps)


@functools.lru_cache(maxsize=None)
def literal_sweep(style, gradient, backward, shape):
    """the literal sampler's sweep of one (cell, shape): ((x, ancestors, history), the case, the gap, the seed's bump); computed once per process and shared,
    never modified by a test.  The seed is advanced, here on the CPU and from the literal alone, until no draw lies within GAP_BAR of a cumulative-weight edge."""
    for bump in range(MAX_BUMPS):
        out, cs = _sweep(style, gradient, backward, shape, bump)
        g = _gap(out, cs, backward)
        if g >= GAP_BAR:
            return out, cs, g, bump
    raise AssertionError(f"no well-posed seed among {MAX_BUMPS} for {(style, gradient, backward, shape)}")


def literal_cells():
    """every (style, gradient, backward, shape) of the fp64 literal comparison"""
    return [(s, g, bw, shape) for s, g, bw in LITERAL_CELLS for shape in REGISTER + WIDE]


# ---- parallel in time ----------------------------------------------------------------------------------------------------------------------------------------
PIT_CELLS = [(1, 32, 25), (3, 100, 33), (1, 100, 25), (6, 25, 25), (13, 32, 33)]  # (d, N, T): three register cells, two wide ones


class PitCase(PC._Sides):
    """tests/pit_cases.py's sides of one cell on this file's objects: missing data at t = 0 (one component), on the top-level stitch boundary (the whole row)
    and at the last step (all but the last component)"""

    def __init__(self, d, N, T, gradient, bump=0):
        self.d, self.N, self.T, self.gradient = d, N, T, bool(gradient)
        rng = np.random.default_rng([19, d, N, T, int(gradient), bump])
        self.dev, self.m, xtrue, self.delta = case(d, T, rng, family_of((d, N, T)), nan_steps=(0, PC.top_boundary(T), T - 1))
        self.x0 = xtrue + 0.3 * rng.standard_normal((T, d))
        self.noise = dict(eps_aux=rng.standard_normal((T, d)), eps_prop=rng.standard_normal((T, N, d)), u_res=rng.random((T, N)))

    def literal_objects(self):
        return self.m.literal()

    def joint_grad(self, u):
        return joint_grad(self.m, u)

    def device_objects(self):
        return self.dev


@functools.lru_cache(maxsize=None)
def pit_literal(d, N, T, gradient):
    """(the case, its literal tree sweep (x, origins, history)) of one cell, the seed advanced on the CPU until the literal's smallest draw margin is at least
    tests/pit_cases.py::margin_threshold(N)"""
    for bump in range(MAX_BUMPS):
        c = PitCase(d, N, T, gradient, bump)
        out = c.literal_sweep()
        if out[2]["min_margin"] >= PC.margin_threshold(N):
            return c, out
    raise AssertionError(f"no well-posed seed among {MAX_BUMPS} for the tree cell {(d, N, T, gradient)}")
