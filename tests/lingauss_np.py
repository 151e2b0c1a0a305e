"""The linear-Gaussian observation potential (AUXSSM_POT_LIN_GAUSS) as GENERIC protocol objects for the literal NumPy cSMC (oracle/csmc_np.py), the cases the
tests of this potential share, and the exact posterior of the whole (linear-Gaussian) model.  Test infrastructure only, written independently of the package:

    log g_t(x) = log N(y_t; H x + c, R),   NaN -> 0

with np.linalg.solve on the UNWHITENED residual and slogdet -- neither the kernels' whitened form nor their operation order: agreement is to rounding.

The literal independent sampler with gradient proposals differentiates the joint log-density by central differences (oracle/csmc_np.py), whose error is far
above the 1e-12 the particles are held to; `independent_kernel` builds the same sampler from the same oracle classes with the gradient in closed form
(`joint_grad`), which tests/test_lingauss_potential.py holds against those central differences (the arrangement of tests/mvt_np.py)."""
import functools

import numpy as np

from oracle import csmc_np as L
from tests import guided_np as G


def log_g(x, y, H, R, c):
    x = np.asarray(x, np.float64)
    H, R = np.asarray(H, np.float64), np.asarray(R, np.float64)
    with np.errstate(invalid="ignore"):
        r = np.asarray(y, np.float64) - (np.atleast_2d(x) @ H.T + np.asarray(c, np.float64))
        q = np.sum(r * np.linalg.solve(R, r.T).T, axis=-1)
        v = -0.5 * q - 0.5 * np.linalg.slogdet(R)[1] - 0.5 * H.shape[0] * np.log(2.0 * np.pi)
    v = np.where(np.isnan(v), 0.0, v)
    return v if x.ndim > 1 else v[0]


def grad_log_g(x, y, H, R, c):
    """d log g / dx = H^T R^-1 (y - H x - c); 0 where the value was NaN"""
    x = np.asarray(x, np.float64)
    H, R = np.asarray(H, np.float64), np.asarray(R, np.float64)
    with np.errstate(invalid="ignore"):
        r = np.asarray(y, np.float64) - (np.atleast_2d(x) @ H.T + np.asarray(c, np.float64))
        g = np.linalg.solve(R, r.T).T @ H
    g = np.where(np.isnan(g), 0.0, g)
    return g if x.ndim > 1 else g[0]


class LinGaussPotential:
    """g_t as a `Potential` with params = y[1:] and as the `UnivariatePotential` of y[0] (oracle.csmc_np.ObsPotential's two roles)"""

    def __init__(self, H, R, c, y, first=False):
        self.H, self.R, self.c, self.first = np.asarray(H, np.float64), np.asarray(R, np.float64), np.asarray(c, np.float64), first
        self.params = None if first else np.asarray(y)
        self.y0 = np.asarray(y) if first else None

    def __call__(self, *a):
        return log_g(a[0], self.y0 if self.first else a[2], self.H, self.R, self.c)


class Model(G.Model):
    """tests/guided_np.py's model record with this potential (time-invariant transitions)"""

    def __init__(self, m0, P0, dyn, Q, H, R, c, y):
        super().__init__(m0, P0, dyn, Q, LinGaussPotential(H, R, c, y[0], first=True), LinGaussPotential(H, R, c, y[1:]), "lingauss", y)
        self.H, self.R, self.c = np.asarray(H, np.float64), np.asarray(R, np.float64), np.asarray(c, np.float64)
        self.F, self.b = np.asarray(dyn.params[0][0], float), np.asarray(dyn.params[1][0], float)

    def literal(self):
        """(M0, G0, Mt, Gt) of the literal sampler"""
        return L.GaussianInit(self.m0, self.LP0), self.G0, self.dyn, self.Gt


def joint_grad(m, u):
    """the gradient at u (T, d) of log M0(u_0) + G0(u_0) + sum_t [log Mt(u_{t+1} | u_t) + Gt(u_{t+1})] (csmc/independent.py:121-134), in closed form"""
    T = u.shape[0]
    g = np.stack([grad_log_g(u[t], m.y[t], m.H, m.R, m.c) for t in range(T)])
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
        return u + (scale * scale)[:, None] * np.stack([grad_log_g(u[t], m.y[t], m.H, m.R, m.c) for t in range(u.shape[0])])

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


def exact_posterior(m):
    """mean (T d,) and covariance (T d, T d) of the stacked (x_0 ... x_{T-1}) given the observations: the dense joint precision J and potential vector h
    assembled term by term from P0, F, b, Q, H, R, c, y (steps whose observation has a NaN skipped), then one dense solve.  No filter, nothing of the package."""
    T, d = m.y.shape[0], m.m0.shape[0]
    J, h = np.zeros((T * d, T * d)), np.zeros(T * d)
    P0i, Qi, Ri = np.linalg.inv(m.P0), np.linalg.inv(m.Q), np.linalg.inv(m.R)
    s = lambda t: slice(t * d, (t + 1) * d)
    J[s(0), s(0)] += P0i
    h[s(0)] += P0i @ m.m0
    for t in range(1, T):  # -1/2 (x_t - F x_{t-1} - b)' Q^-1 (x_t - F x_{t-1} - b)
        J[s(t), s(t)] += Qi
        J[s(t - 1), s(t - 1)] += m.F.T @ Qi @ m.F
        J[s(t), s(t - 1)] -= Qi @ m.F
        J[s(t - 1), s(t)] -= m.F.T @ Qi
        h[s(t)] += Qi @ m.b
        h[s(t - 1)] -= m.F.T @ Qi @ m.b
    for t in range(T):  # -1/2 (y_t - c - H x_t)' R^-1 (y_t - c - H x_t)
        if np.isnan(m.y[t]).any():
            continue
        J[s(t), s(t)] += m.H.T @ Ri @ m.H
        h[s(t)] += m.H.T @ Ri @ (m.y[t] - m.c)
    cov = np.linalg.inv(J)
    return cov @ h, 0.5 * (cov + cov.T)


# ---- cases: the model on both sides ---------------------------------------------------------------------------------------------------------------------
def observation(d, dy, rng):
    """a dense H (dy, d) with no zero entry, a non-diagonal R with eigenvalues in [0.4, 1.6] and an offset c != 0"""
    H = rng.standard_normal((dy, d)) / np.sqrt(d)
    H = np.where(np.abs(H) < 0.05 / np.sqrt(d), 0.05 / np.sqrt(d), H)
    U = np.linalg.qr(rng.standard_normal((dy, dy)))[0]
    R = (U * np.linspace(0.4, 1.6, dy)) @ U.T
    return H, 0.5 * (R + R.T), 0.3 * rng.standard_normal(dy) + 0.1


def build(m0, P0, F, b, Q, H, R, c, y):
    """(device objects (M0, G0, Mt, Gt), literal Model) of one model"""
    from aux_ssm_samplers_amd.csmc import GaussianInit, LinearGaussianDynamics, LinearGaussianPotential
    T = y.shape[0]
    M0, Mt = GaussianInit(m0=m0, P0=P0), LinearGaussianDynamics(F=F, b=b, Q=Q)
    dev = (M0, LinearGaussianPotential(H=H, R=R, c=c, y=y[0]), Mt, LinearGaussianPotential(H=H, R=R, c=c, params=y[1:]))
    return dev, Model(m0, P0, L.LinearGaussianDynamics(F, b, np.linalg.cholesky(Q), T), Q, H, R, c, y)


def case(d, dy, T, rng, nan_rows=()):
    """tests/guided_np.py::sv_case's linear-Gaussian dynamics observed through `observation`.  nan_rows: time steps whose observation has a NaN component (the
    step is flat).  Returns (device objects (M0, G0, Mt, Gt), literal Model, a trajectory, delta in [0.2, 0.8] / d: proposals that N <= 64 particles can
    follow at every d)."""
    F = 0.9 * np.eye(d) + 0.02 * rng.standard_normal((d, d)) / np.sqrt(d)
    b = 0.05 * rng.standard_normal(d)
    Q, P0, m0 = G.spd(d, rng), G.spd(d, rng, 0.5), 0.1 * rng.standard_normal(d)
    H, R, c = observation(d, dy, rng)
    x = np.zeros((T, d))
    x[0] = m0 + np.linalg.cholesky(P0) @ rng.standard_normal(d)
    for t in range(1, T):
        x[t] = F @ x[t - 1] + b + np.linalg.cholesky(Q) @ rng.standard_normal(d)
    y = x @ H.T + c + rng.standard_normal((T, dy)) @ np.linalg.cholesky(R).T
    for i, t in enumerate(nan_rows):
        y[t, i % dy] = np.nan
    dev, m = build(m0, P0, F, b, Q, H, R, c, y)
    return dev, m, x, (0.2 + 0.6 * rng.random(T)) / d


def program(dev, grad=False):
    """the same model with the potential as user source (device_models.BUILTIN_LINGAUSS[_GRAD]): theta = [c_lin, Hw row-major], observations = yw"""
    from aux_ssm_samplers_amd.csmc import DevicePotential, device_models as U
    M0, G0, Mt, Gt = dev
    src = U.BUILTIN_LINGAUSS_GRAD if grad else U.BUILTIN_LINGAUSS
    d = G0.dx
    Hw, yw, c_lin = Gt.whitened(np.concatenate([np.reshape(G0.y, (1, -1)), np.reshape(Gt.params, (-1, G0.dy))], axis=0))
    theta = np.concatenate([[c_lin], Hw.reshape(-1)])
    return M0, DevicePotential(src, y=yw[0], theta=theta, p=d), Mt, DevicePotential(src, params=yw[1:], theta=theta, p=d)


# ---- the cases of tests/test_gpu_lingauss.py, shared with the CPU tests that vouch for them (whitening identity, well-posedness of the ancestor comparison) ----
PROGRAM_SHAPES = [(1, 1, 1024, 40, 5), (2, 1, 100, 40, 5), (4, 2, 64, 24, 3), (4, 4, 65, 24, 3)]  # (d, dy, N, T, chains)
LITERAL_CASES = dict(r1=(1, 1, 1024, 40), r3=(3, 2, 100, 33), r4=(4, 1, 64, 24),
                     w5=(5, 3, 33, 20), w9=(9, 9, 25, 20), w25=(25, 12, 25, 25), w32a=(32, 1, 64, 12), w32b=(32, 32, 64, 12))  # (d, dy, N, T)
REGISTER, WIDE = ("r1", "r3", "r4"), ("w5", "w9", "w25", "w32a", "w32b")
LITERAL_CELLS = ([("independent", g, bw) for g in (False, True, "exact") for bw in (False, True)]
                 + [("guided", g, bw) for g in (False, True) for bw in (False, True)])
BOOTSTRAP_CASES = ("r3", "w9")


# (cell, case) -> how often its seed was advanced until no draw of the literal sweep lay within 1e-8 of a cumulative-sum edge (wellposedness below; at N = 1024
# and T = 40 some forty thousand draws meet a thousand edges, so a first seed fails about every other time)
SEED_BUMPS = {("independent", False, False, "r1"): 12, ("independent", False, True, "r1"): 6, ("independent", True, False, "r1"): 6,
              ("independent", True, True, "r1"): 11, ("independent", "exact", True, "r1"): 13, ("guided", False, False, "r1"): 2,
              ("guided", False, True, "r1"): 16, ("guided", True, True, "r1"): 21}


def literal_seed(style, gradient, backward, name):
    """the seed of one (cell, case) of the literal comparison (tests/test_lingauss_potential.py checks that no draw of it lies on a cumulative-sum edge)"""
    si = dict(independent=0, guided=1, bootstrap=2)[style]
    gi = {False: 0, True: 1, "exact": 2}[gradient]
    return 9000 + 1000 * si + 100 * gi + 50 * int(backward) + list(LITERAL_CASES).index(name) + 7919 * SEED_BUMPS.get((style, gradient, backward, name), 0)


def literal_case(name, seed):
    """(d, N, T, device objects, Model, reference trajectory, delta, noise) of one literal case: NaN rows at t = 0, mid-series and T - 1"""
    d, dy, N, T = LITERAL_CASES[name]
    rng = np.random.default_rng(seed)
    dev, m, xtrue, delta = case(d, dy, T, rng, nan_rows=(0, T // 2, T - 1))
    x0 = xtrue + 0.3 * rng.standard_normal((T, d))
    nz = dict(eps_aux=rng.standard_normal((T, d)), eps_prop=rng.standard_normal((T, N, d)), u_res=rng.random((T - 1, N)), u_bwd=rng.random(T))
    return d, N, T, dev, m, x0, delta, nz


@functools.lru_cache(maxsize=None)
def literal_sweep(style, gradient, backward, name):
    """the literal sampler's sweep of one (cell, case): ((x, ancestors, history), the case); computed once per process and shared, never modified by a test"""
    cs = literal_case(name, literal_seed(style, gradient, backward, name))
    d, N, T, dev, m, x0, delta, nz = cs
    nz = dict(nz)
    if style == "bootstrap":
        nz.pop("eps_aux")
        return bootstrap_kernel(m, N, backward)[1](L.Noise(**nz), x0), cs
    if style == "guided":
        return guided_kernel(m, N, backward, gradient)[1](L.Noise(**nz), x0, delta), cs
    return independent_kernel(m, N, backward, gradient)[1](L.Noise(**nz), x0, delta), cs


def wellposedness(style, gradient, backward, name):
    """of the literal sweep of one (cell, case): the smallest distance of a resampling or backward draw r = c[-1] (1 - u) from a cumulative-weight edge c[j]
    (weights normalised to sum 1) -- tests/user_models.py::wellposedness's gap -- and the share of time steps whose new ancestor is not the reference particle"""
    (x, B, h), (d, N, T, dev, m, x0, delta, nz) = literal_sweep(style, gradient, backward, name)

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
    return dict(gap=min(gaps), moved=float(np.mean(B != 0)))


def literal_cells():
    """every (style, gradient, backward, case name) of the fp64 literal comparison"""
    out = [(s, g, bw, n) for s, g, bw in LITERAL_CELLS for n in REGISTER + WIDE]
    return out + [("bootstrap", False, bw, n) for bw in (False, True) for n in BOOTSTRAP_CASES]
