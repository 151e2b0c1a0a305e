"""The literal side of every built-in observation potential of the cSMC family, once: the model record, the row potential, the literal samplers, the draw gap,
the seeded literal sweeps (sequential and parallel in time), the scalar quadrature and the generators the cases share.  Test infrastructure only; CPU only; nothing
of the package is imported here.

What is particular to a potential lives in its own module (tests/mvt_np.py, tests/lingauss_np.py, tests/poisson_np.py, tests/logistic_np.py): log_g, grad_log_g,
the data generator, the device objects, the case tables -- and one `Kind` record that ties them together and carries the seeds of its cases.  The seeds are part
of the tests: every case draws the numbers it drew when its potential was added.

The literal independent sampler with gradient proposals (oracle/csmc_np.py::get_independent_kernel) differentiates the joint log-density by central differences
(its stand-in for jax.grad), whose error -- about 1e-10 -- is far above the 1e-12 the particles are held to.  `independent_kernel` therefore builds the same sampler
from the same oracle classes (AuxiliaryM0 / AuxiliaryG0 / GradientAuxiliaryG0 / AuxiliaryMtDynamics / AuxiliaryGt / GradientAuxiliaryGt on get_generic_kernel) with
the gradient in closed form (`joint_grad`), which each tests/test_<kind>_potential.py holds against those central differences."""
import dataclasses
import functools
import typing

import numpy as np

from oracle import csmc_np as L
from tests import guided_np as G
from tests import pit_cases as PC

GAP_BAR = 1e-8  # the bar on the smallest distance of a resampling or backward draw from a cumulative-weight edge (weights normalised to sum 1)
MAX_BUMPS = 32  # how many seeds a kind whose seeds advance offers per cell
LITERAL_CELLS = ([("independent", g, bw) for g in (False, True, "exact") for bw in (False, True)]
                 + [("guided", g, bw) for g in (False, True) for bw in (False, True)])
BOOTSTRAP_CELLS = [("bootstrap", False, bw) for bw in (False, True)]


def one_row(row):
    return (row,)


@dataclasses.dataclass(frozen=True, eq=False)
class Kind:
    """one potential: its functions, its cases and their seeds.  A literal case is named by a `key` (a name or a shape), a tree cell by a tuple that
    `pit_model` understands."""
    name: str
    code: int                              # AUXSSM_POT_*
    log_g: typing.Callable                 # log_g(x, *split(row), *const)
    grad_log_g: typing.Callable
    split: typing.Callable = one_row       # a parameter row -> the leading arguments of log_g after x (the logistic kind: [y | m] -> (y, m))
    # the fp64 literal comparison: (style, gradient, backward) -> the keys of that cell; key, rng -> (d, N, T, device objects, Model, trajectory, delta);
    # (style, gradient, backward, key) -> the seeds to try, in order (one seed: it is taken as it is)
    cells: typing.Callable = None
    literal_model: typing.Callable = None
    seeds: typing.Callable = None
    label: typing.Callable = str           # key -> how a printed line names it
    # parallel in time: the cells; cell, rng -> (d, N, T, device objects, Model, trajectory, delta); (cell, gradient) -> the seeds to try, in order
    pit_cells: tuple = ()
    pit_model: typing.Callable = None
    pit_seeds: typing.Callable = None
    program: typing.Callable = None        # (device objects, gradient) -> the same model with the potential as user source


class RowPotential:
    """g_t as a `Potential` with params = the rows of steps 1 .. T - 1 and as the `UnivariatePotential` of row 0 (oracle.csmc_np.ObsPotential's two roles)"""

    def __init__(self, kind, rows, const=(), first=False):
        self.kind, self.const, self.first = kind, tuple(const), first
        self.params = None if first else np.asarray(rows)
        self.row0 = np.asarray(rows) if first else None

    def __call__(self, *a):
        return self.kind.log_g(a[0], *self.kind.split(self.row0 if self.first else a[2]), *self.const)


class Model(G.Model):
    """tests/guided_np.py's model record with a potential of `kind`: rows (T, p) its per-step parameter rows (the observations; the logistic kind: [y | m]), const
    its arguments that do not change with the step; y = the observations themselves.  attrs: the names a kind's tests read (nu, prec, H, R, c, size)."""

    def __init__(self, kind, m0, P0, dyn, Q, rows, const=(), **attrs):
        rows = np.asarray(rows)
        super().__init__(m0, P0, dyn, Q, RowPotential(kind, rows[0], const, first=True), RowPotential(kind, rows[1:], const), kind.name, kind.split(rows)[0])
        self.pot, self.rows, self.const = kind, rows, tuple(const)
        self.__dict__.update(attrs)
        self.F, self.b = np.asarray(dyn.params[0][0], float), np.asarray(dyn.params[1][0], float)
        self.tv = False  # time-varying transitions: dyn.params has a row per transition, Q / LQ / F / b above are those of the first

    def args(self, t):
        """the arguments of log_g / grad_log_g after x at step t"""
        return (*self.pot.split(self.rows[t]), *self.const)

    def trans(self, t):
        """(F, b, Q, chol Q) of the transition into step t >= 1"""
        if not self.tv:
            return self.F, self.b, self.Q, self.LQ
        F, b, LQ = (np.asarray(p[t - 1], float) for p in self.dyn.params)
        return F, b, LQ @ LQ.T, LQ

    def literal(self):
        """(M0, G0, Mt, Gt) of the literal sampler"""
        return L.GaussianInit(self.m0, self.LP0), self.G0, self.dyn, self.Gt


# ---- the literal samplers ------------------------------------------------------------------------------------------------------------------------------------
def pot_grad(m, u):
    """grad log g_t(u_t), t < T"""
    return np.stack([m.pot.grad_log_g(u[t], *m.args(t)) for t in range(u.shape[0])])


def joint_grad(m, u):
    """the gradient at u (T, d) of log M0(u_0) + G0(u_0) + sum_t [log Mt(u_{t+1} | u_t) + Gt(u_{t+1})] (csmc/independent.py:121-134), in closed form"""
    g = pot_grad(m, u)
    g[0] -= np.linalg.solve(m.P0, u[0] - m.m0)
    for t in range(1, u.shape[0]):
        F, b, Q, _ = m.trans(t)
        w = np.linalg.solve(Q, u[t] - (F @ u[t - 1] + b))
        g[t] -= w
        g[t - 1] += F.T @ w
    return g


def guided_kernel(m, N, backward=False, gradient=False):
    """the literal guided sampler of tests/guided_np.py (time-invariant transitions); its gradient variant shifts u by s^2 grad log g_t(u_t)"""
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


def run_literal(style, gradient, backward, m, N, nz, x0, delta):
    """(x, ancestors, history) of one literal sweep on the explicit noise nz (eps_aux, eps_prop, u_res, u_bwd; the bootstrap style leaves eps_aux and delta out)"""
    nz = dict(nz)
    if style == "bootstrap":
        nz.pop("eps_aux")
        return bootstrap_kernel(m, N, backward)[1](L.Noise(**nz), x0)
    kernel = guided_kernel if style == "guided" else independent_kernel
    return kernel(m, N, backward, gradient)[1](L.Noise(**nz), x0, delta)


def draw_gap(out, nz, dyn, backward):
    """of a literal sweep out = (x, ancestors, history) on the noise nz: the smallest distance of a resampling or backward draw r = c[-1] (1 - u) from a
    cumulative-weight edge c[j] (weights normalised to sum 1).  The exact ancestor comparisons demand EQUAL indices of the device and the fp64 literal while their
    log-weights agree to 1e-10: fair only if no draw lies within rounding of an edge."""
    x, _, h = out
    T, N = h["log_ws"].shape

    def gap(w, u):
        c = np.cumsum(w)
        r = c[-1] * (1 - np.atleast_1d(u))
        return float(np.min(np.abs(r[:, None] - c[None, :])))
    gaps = [gap(L.normalize(h["log_ws"][t]), nz["u_res"][t][1:]) for t in range(T - 1) if N > 1]
    gaps.append(gap(h["w_T"], nz["u_bwd"][T - 1]))
    if backward:
        for t in range(T - 2, -1, -1):
            lw = dyn.logpdf(x[t + 1], h["xs"][t], L._tree_index(dyn.params, t)) + h["log_ws"][t]
            gaps.append(gap(L.normalize(lw), nz["u_bwd"][t]))
    return min(gaps)


# ---- the seeded literal sweeps -------------------------------------------------------------------------------------------------------------------------------
def literal_case(kind, key, seed):
    """(d, N, T, device objects, Model, reference trajectory, delta, noise) of one literal case"""
    rng = np.random.default_rng(seed)
    d, N, T, dev, m, xtrue, delta = kind.literal_model(key, rng)
    x0 = xtrue + 0.3 * rng.standard_normal((T, d))
    return d, N, T, dev, m, x0, delta, G.noise(T, N, d, rng)


@functools.lru_cache(maxsize=None)
def literal_sweep(kind, style, gradient, backward, key):
    """the literal sampler's sweep of one (cell, case): ((x, ancestors, history), the case, the gap, the seed's bump); computed once per process and shared between
    the CPU and the GPU tests, never modified by a test.  The kind's seeds are tried in order, here on the CPU and from the literal alone, until no draw lies
    within GAP_BAR of a cumulative-weight edge (draw_gap).  A kind that offers one seed has nothing to choose between: its sweep is returned with gap None, and what
    vouches for the seed is the kind's own business (tests/test_lingauss_potential.py computes the gap of every cell; the multivariate-t cases predate the rule)."""
    seeds = list(kind.seeds(style, gradient, backward, key))
    for bump, seed in enumerate(seeds):
        cs = literal_case(kind, key, seed)
        d, N, T, dev, m, x0, delta, nz = cs
        out = run_literal(style, gradient, backward, m, N, nz, x0, delta)
        if len(seeds) == 1:
            return out, cs, None, bump
        g = draw_gap(out, nz, m.dyn, backward)
        if g >= GAP_BAR:
            return out, cs, g, bump
    raise AssertionError(f"no well-posed seed among {len(seeds)} for {kind.name} {(style, gradient, backward, key)}")


def literal_cells(kind):
    """every (style, gradient, backward, key) of the kind's fp64 literal comparison"""
    return [(s, g, bw, key) for s, g, bw in LITERAL_CELLS + BOOTSTRAP_CELLS for key in kind.cells(s, g, bw)]


class PitCase(PC._Sides):
    """tests/pit_cases.py's sides of one tree cell of a kind"""

    def __init__(self, kind, cell, gradient, seed):
        self.kind, self.cell, self.gradient = kind, cell, bool(gradient)
        rng = np.random.default_rng(seed)
        self.d, self.N, self.T, self.dev, self.m, xtrue, self.delta = kind.pit_model(cell, rng)
        self.x0 = xtrue + 0.3 * rng.standard_normal((self.T, self.d))
        self.noise = dict(eps_aux=rng.standard_normal((self.T, self.d)), eps_prop=rng.standard_normal((self.T, self.N, self.d)),
                          u_res=rng.random((self.T, self.N)))

    def literal_objects(self):
        return self.m.literal()

    def joint_grad(self, u):
        return joint_grad(self.m, u)

    def device_objects(self):
        return self.dev


@functools.lru_cache(maxsize=None)
def pit_literal(kind, cell, gradient):
    """(the case, its literal tree sweep (x, origins, history)) of one cell, computed once per process: the kind's seeds are tried in order, on the CPU, until the
    literal's smallest draw margin is at least tests/pit_cases.py::margin_threshold(N)"""
    seeds = list(kind.pit_seeds(cell, gradient))
    for seed in seeds:
        c = PitCase(kind, cell, gradient, seed)
        out = c.literal_sweep()
        if out[2]["min_margin"] >= PC.margin_threshold(c.N):
            return c, out
    raise AssertionError(f"no well-posed seed among {len(seeds)} for the {kind.name} tree cell {cell}, gradient={gradient}")


# ---- the posterior of a scalar model by quadrature --------------------------------------------------------------------------------------------------------------
def posterior_by_quadrature(steps, m0, P0, F, Q, b, n=1601, width=9.0):
    """(T, 2): posterior mean and variance of every x_t of the SCALAR model x_0 ~ N(m0, P0), x_t ~ N(F x_{t-1} + b, Q) with the potentials steps[t](x) = log g_t
    at states x (n, 1) (a step that is not observed: 0), by a forward-backward pass on one uniform grid that covers the prior marginals of all steps by `width`
    standard deviations (the likelihood only narrows them): alpha_t(x') = g_t(x') sum_x alpha_{t-1}(x) N(x'; F x + b, Q), beta alike, marginal ~ alpha_t beta_t.
    The grid spacing stays far below sqrt(Q) and the marginal widths, so the rectangle rule is exact to far more digits than any standard error.  Independent of
    every sampler and oracle."""
    m0, P0, F, Q, b = (float(np.reshape(a, -1)[0]) for a in (m0, P0, F, Q, b))
    T = len(steps)
    mu, var, lo, hi = m0, P0, np.inf, -np.inf
    for t in range(T):
        if t > 0:
            mu, var = F * mu + b, F * F * var + Q
        lo, hi = min(lo, mu - width * np.sqrt(var)), max(hi, mu + width * np.sqrt(var))
    g = np.linspace(lo, hi, n)
    assert g[1] - g[0] < 0.05 * np.sqrt(min(Q, P0))
    lg = np.stack([f(g[:, None]) for f in steps])
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


def independent_moments(steps_of, d, par):
    """(E x_t, E x_t x_t^T) of the posterior of a model with diagonal P0, F and Q (par = (m0, P0, F, Q, b), the diagonals): per component by quadrature on
    steps_of(k), cross moments as products of the means (the components are independent)"""
    m0, P0, F, Q, b = par
    q = np.stack([posterior_by_quadrature(steps_of(k), m0[k], P0[k], F[k], Q[k], b[k]) for k in range(d)], axis=1)  # (T, d, 2)
    mean = q[..., 0]
    second = mean[:, :, None] * mean[:, None, :]
    second[:, np.arange(d), np.arange(d)] += q[..., 1]
    return mean, second


# ---- the generators the cases share ----------------------------------------------------------------------------------------------------------------------------
def dynamics(d, rng, level=None):
    """tests/guided_np.py::sv_case's linear-Gaussian dynamics (F = 0.9 I + small, Q = 0.3 I + small SPD, P0 alike): (m0, P0, F, b, Q) around 0, or (level given)
    moved to a stationary mean of about `level`"""
    F = 0.9 * np.eye(d) + 0.02 * rng.standard_normal((d, d)) / np.sqrt(d)
    if level is None:
        centre, b = 0.0, 0.05 * rng.standard_normal(d)
    else:
        centre = level + 0.1 * rng.standard_normal(d)
        b = centre - F @ centre
    Q, P0 = G.spd(d, rng), G.spd(d, rng, 0.5)
    return centre + 0.1 * rng.standard_normal(d), P0, F, b, Q


def trajectory(m0, P0, F, b, Q, T, rng):
    """x (T, d) of the model; F, b and Q of all transitions or, with a leading axis T - 1, of each"""
    Ft, bt, Qt = (np.broadcast_to(a, (T - 1,) + np.shape(a)[-n:]) for a, n in ((F, 2), (b, 1), (Q, 2)))
    x = np.zeros((T, len(m0)))
    x[0] = m0 + np.linalg.cholesky(P0) @ rng.standard_normal(len(m0))
    for t in range(1, T):
        x[t] = Ft[t - 1] @ x[t - 1] + bt[t - 1] + np.linalg.cholesky(Qt[t - 1]) @ rng.standard_normal(len(m0))
    return x


def knock_out(y, nan_steps):
    """missing data per component, in place: the first step of every three loses component 0, the second its WHOLE row, the third every component but the last
    (for d >= 2 a row that is partly NaN; d = 1: its only component)"""
    d = y.shape[1]
    for i, t in enumerate(nan_steps):
        if i % 3 == 0:
            y[t, 0] = np.nan
        elif i % 3 == 1:
            y[t, :] = np.nan
        else:
            y[t, :max(d - 1, 1)] = np.nan


def seed_index(style, gradient, backward):
    """1000 * style + 100 * gradient + 50 * backward: what the seed bases of the literal cells add to"""
    return 1000 * dict(independent=0, guided=1, bootstrap=2)[style] + 100 * {False: 0, True: 1, "exact": 2}[gradient] + 50 * int(backward)
