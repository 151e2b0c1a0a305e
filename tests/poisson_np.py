"""The Poisson count potential (AUXSSM_POT_POISSON) as GENERIC protocol objects for the literal NumPy cSMC (oracle/csmc_np.py, oracle/pit_np.py,
tests/guided_np.py), the cases the tests of this potential share, and the posterior of the scalar model by quadrature.  Test infrastructure only, written
independently of the package:

    log g_t(x) = sum_k [ y_{t,k} x_k - exp(x_k) ]   over the components whose y_{t,k} is finite (the -log y! constant left out)

with np.exp and a masked np.sum -- neither the kernels' det_exp nor their fused multiply-add: agreement is to rounding.

The literal independent sampler with gradient proposals differentiates the joint log-density by central differences (oracle/csmc_np.py), whose error is far
above the 1e-12 the particles are held to; `independent_kernel` builds the same sampler from the same oracle classes with the gradient in closed form
(`joint_grad`), which tests/test_poisson_potential.py holds against those central differences (the arrangement of tests/lingauss_np.py)."""
import functools

import numpy as np

from oracle import csmc_np as L
from tests import guided_np as G
from tests import pit_cases as PC


def log_g(x, y):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        v = y * np.atleast_2d(x) - np.exp(np.atleast_2d(x))
    v = np.sum(np.where(np.isfinite(y), v, 0.0), axis=-1)
    return v if x.ndim > 1 else v[0]


def grad_log_g(x, y):
    """d log g / dx_k = y_k - exp(x_k); 0 for a missing component"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        g = np.where(np.isfinite(y), y - np.exp(x), 0.0)
    return g


def bound(y):
    """sup_x log g = sum_k (y_k > 0 ? y_k (log y_k - 1) : 0), attained at x_k = log y_k"""
    y = np.asarray(y, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.sum(np.where(y > 0, y * (np.log(np.where(y > 0, y, 1.0)) - 1.0), 0.0)))


class PoissonPotential:
    """g_t as a `Potential` with params = y[1:] and as the `UnivariatePotential` of y[0] (oracle.csmc_np.ObsPotential's two roles)"""

    def __init__(self, y, first=False):
        self.first = first
        self.params = None if first else np.asarray(y)
        self.y0 = np.asarray(y) if first else None

    def __call__(self, *a):
        return log_g(a[0], self.y0 if self.first else a[2])


class Model(G.Model):
    """tests/guided_np.py's model record with this potential (time-invariant transitions)"""

    def __init__(self, m0, P0, dyn, Q, y):
        super().__init__(m0, P0, dyn, Q, PoissonPotential(y[0], first=True), PoissonPotential(y[1:]), "poisson", y)
        self.F, self.b = np.asarray(dyn.params[0][0], float), np.asarray(dyn.params[1][0], float)

    def literal(self):
        """(M0, G0, Mt, Gt) of the literal sampler"""
        return L.GaussianInit(self.m0, self.LP0), self.G0, self.dyn, self.Gt


def joint_grad(m, u):
    """the gradient at u (T, d) of log M0(u_0) + G0(u_0) + sum_t [log Mt(u_{t+1} | u_t) + Gt(u_{t+1})] (csmc/independent.py:121-134), in closed form"""
    T = u.shape[0]
    g = np.stack([grad_log_g(u[t], m.y[t]) for t in range(T)])
    g[0] -= np.linalg.solve(m.P0, u[0] - m.m0)
    for t in range(1, T):
        w = np.linalg.solve(m.Q, u[t] - (m.F @ u[t - 1] + m.b))
        g[t] -= w
        g[t - 1] += m.F.T @ w
    return g


def guided_kernel(m, N, backward=False, gradient=False):
    """the literal guided sampler of tests/guided_np.py; its gradient variant shifts u by s^2 grad log g_t(u_t)"""
    def shifted(u, scale):
        if not gradient:
            return u
        return u + (scale * scale)[:, None] * np.stack([grad_log_g(u[t], m.y[t]) for t in range(u.shape[0])])

    def f(u, scale):
        T = u.shape[0]
        tab = [G.tables(m.P0 if t == 0 else m.Q, float(scale[t])) for t in range(T)]
        Ks, Cs = np.stack([a for a, _ in tab]), np.stack([b for _, b in tab])
        ut = shifted(u, scale)
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


def posterior_by_quadrature(y, m0, P0, F, Q, b, n=1601, width=9.0):
    """(T, 2): posterior mean and variance of every x_t of the SCALAR model x_0 ~ N(m0, P0), x_t ~ N(F x_{t-1} + b, Q), y_t ~ Poisson(exp(x_t)) (NaN: not
    observed), by a forward-backward pass on one uniform grid that covers the prior marginals of all steps by `width` standard deviations (the likelihood only
    narrows them): alpha_t(x') = g_t(x') sum_x alpha_{t-1}(x) N(x'; F x + b, Q), beta alike, marginal ~ alpha_t beta_t.  The grid spacing stays far below
    sqrt(Q) and the marginal widths, so the rectangle rule is exact to far more digits than any standard error.  Independent of every sampler and oracle."""
    y = np.asarray(y, np.float64).reshape(-1)
    m0, P0, F, Q, b = (float(np.reshape(a, -1)[0]) for a in (m0, P0, F, Q, b))
    T = y.shape[0]
    mu, var, lo, hi = m0, P0, np.inf, -np.inf
    for t in range(T):
        if t > 0:
            mu, var = F * mu + b, F * F * var + Q
        lo, hi = min(lo, mu - width * np.sqrt(var)), max(hi, mu + width * np.sqrt(var))
    g = np.linspace(lo, hi, n)
    assert g[1] - g[0] < 0.05 * np.sqrt(min(Q, P0))
    lg = np.stack([np.zeros(n) if not np.isfinite(y[t]) else y[t] * g - np.exp(g) for t in range(T)])
    ltr = -0.5 * (g[None, :] - (F * g[:, None] + b)) ** 2 / Q  # [x, x']
    tr = np.exp(ltr)

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
def build(m0, P0, F, b, Q, y):
    """(device objects (M0, G0, Mt, Gt), literal Model) of one model"""
    from aux_ssm_samplers_amd import csmc
    T = y.shape[0]
    M0, Mt = csmc.GaussianInit(m0=m0, P0=P0), csmc.LinearGaussianDynamics(F=F, b=b, Q=Q)
    dev = (M0, csmc.PoissonPotential(y=y[0]), Mt, csmc.PoissonPotential(params=y[1:]))
    return dev, Model(m0, P0, L.LinearGaussianDynamics(F, b, np.linalg.cholesky(Q), T), Q, y)


def case(d, T, rng, nan_steps=()):
    """tests/guided_np.py::sv_case's linear-Gaussian dynamics moved to a stationary mean of about 1 (intensities around e), observed as counts.  nan_steps: up to
    three time steps with missing data -- the first loses component 0, the second its WHOLE row, the third every component but the last (for d >= 2 a row that
    is partly NaN; d = 1: its only component).  Returns (device objects (M0, G0, Mt, Gt), literal Model, a trajectory, delta in [0.1, 0.4] / d: proposals that
    N <= 64 particles can follow at every d, below the Langevin stability limit of the gradient proposals at these intensities)."""
    F = 0.9 * np.eye(d) + 0.02 * rng.standard_normal((d, d)) / np.sqrt(d)
    one = 1.0 + 0.1 * rng.standard_normal(d)
    b = one - F @ one
    Q, P0, m0 = G.spd(d, rng), G.spd(d, rng, 0.5), one + 0.1 * rng.standard_normal(d)
    x = np.zeros((T, d))
    x[0] = m0 + np.linalg.cholesky(P0) @ rng.standard_normal(d)
    for t in range(1, T):
        x[t] = F @ x[t - 1] + b + np.linalg.cholesky(Q) @ rng.standard_normal(d)
    y = rng.poisson(np.exp(x)).astype(np.float64)
    for i, t in enumerate(nan_steps):
        if i % 3 == 0:
            y[t, 0] = np.nan
        elif i % 3 == 1:
            y[t, :] = np.nan
        else:
            y[t, :max(d - 1, 1)] = np.nan
    dev, m = build(m0, P0, F, b, Q, y)
    return dev, m, x, (0.1 + 0.3 * rng.random(T)) / d


def program(dev):
    """the same model with the potential as user source (device_models.BUILTIN_POISSON: value, bound and gradient; no theta)"""
    from aux_ssm_samplers_amd.csmc import DevicePotential, device_models as U
    M0, G0, Mt, Gt = dev
    d = int(np.size(G0.y))
    return M0, DevicePotential(U.BUILTIN_POISSON, y=G0.y, p=d), Mt, DevicePotential(U.BUILTIN_POISSON, params=np.reshape(Gt.params, (-1, d)), p=d)


# ---- the cases of tests/test_gpu_poisson.py, shared with the CPU tests that vouch for them (well-posedness of the ancestor comparison) -----------------------
PROGRAM_SHAPES = [(d, N) for d in (1, 2, 4) for N in (64, 100, 1024)]  # (d, N) at T = 40, 3 chains
PROGRAM_T, PROGRAM_CHAINS = 40, 3
REGISTER = [(d, N, 33) for d in (1, 3) for N in (64, 100)]       # (d, N, T)
WIDE = [(d, N, 25) for d in (5, 13, 32) for N in (25, 64)]
LITERAL_CELLS = ([("independent", g, bw) for g in (False, True, "exact") for bw in (False, True)]
                 + [("guided", g, bw) for g in (False, True) for bw in (False, True)]
                 + [("bootstrap", False, bw) for bw in (False, True)])
GAP_BAR = 1e-8  # tests/test_lingauss_potential.py's bar on the smallest distance of a draw from a cumulative-weight edge
MAX_BUMPS = 32


def _seed(style, gradient, backward, shape, bump):
    si = dict(independent=0, guided=1, bootstrap=2)[style]
    gi = {False: 0, True: 1, "exact": 2}[gradient]
    d, N, T = shape
    return [6000 + 1000 * si + 100 * gi + 50 * int(backward), d, N, T, bump]


def literal_case(shape, seed):
    """(d, N, T, device objects, Model, reference trajectory, delta, noise) of one literal case: NaN entries at t = 0 (one component), mid-series (the whole
    row) and T - 1 (all but the last component)"""
    d, N, T = shape
    rng = np.random.default_rng(seed)
    dev, m, xtrue, delta = case(d, T, rng, nan_steps=(0, T // 2, T - 1))
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
    never modified by a test.  The seed is advanced, here on the CPU and from the literal alone, until no draw lies within GAP_BAR of a cumulative-weight edge
    (at N <= 100 and T <= 33 a first seed fails about once in a hundred cells)."""
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
        rng = np.random.default_rng([17, d, N, T, int(gradient), bump])
        self.dev, self.m, xtrue, self.delta = case(d, T, rng, nan_steps=(0, PC.top_boundary(T), T - 1))
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
