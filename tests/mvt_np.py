"""The multivariate Student-t potential (AUXSSM_POT_MVT) as GENERIC protocol objects for the literal NumPy cSMC (oracle/csmc_np.py), and the cases the
tests of this potential share.  Test infrastructure only.

    log g_t(x) = -(nu + d) / 2 log(1 + (x - y_t)^T prec (x - y_t) / nu),   NaN -> 0          (examples/spatial/t_distribution.py:98-104, model.py:121-124)

written here with NumPy's own matrix product and log1p -- not in the kernels' operation order: agreement is to rounding, not bit for bit.

The literal independent sampler with gradient proposals (oracle/csmc_np.py::get_independent_kernel) differentiates the joint log-density by central
differences (its stand-in for jax.grad), whose error -- about 1e-10 -- is far above the 1e-12 the particles are held to.  `independent_kernel` therefore builds the
same sampler from the same oracle classes (AuxiliaryM0 / AuxiliaryG0 / GradientAuxiliaryG0 / AuxiliaryMtDynamics / AuxiliaryGt / GradientAuxiliaryGt on
get_generic_kernel) with the gradient in closed form (`joint_grad`), which tests/test_mvt_potential.py holds against those central differences."""
import numpy as np

from oracle import csmc_np as L
from tests import guided_np as G


def log_g(x, y, nu, prec):
    x = np.asarray(x)
    r = np.atleast_2d(x) - np.asarray(y, x.dtype)
    with np.errstate(invalid="ignore"):
        q = np.sum((r @ np.asarray(prec, x.dtype).T) * r, axis=-1)
        v = -x.dtype.type(0.5 * (nu + r.shape[-1])) * np.log1p(q / x.dtype.type(nu))
    v = np.where(np.isnan(v), x.dtype.type(0), v)
    return v if x.ndim > 1 else v[0]


def grad_log_g(x, y, nu, prec):
    """d log g / dx = -(nu + d) / (nu + q) prec (x - y); 0 where the value was NaN"""
    x = np.asarray(x, np.float64)
    r = x - np.asarray(y, np.float64)
    z = r @ np.asarray(prec).T
    with np.errstate(invalid="ignore"):
        q = np.sum(z * r, axis=-1, keepdims=True)
        g = -(nu + x.shape[-1]) / (nu + q) * z
    return np.where(np.isnan(g), 0.0, g)


class MvtPotential:
    """g_t as a `Potential` with params = y[1:] and as the `UnivariatePotential` of y[0] (oracle.csmc_np.ObsPotential's two roles)"""

    def __init__(self, nu, prec, y, first=False):
        self.nu, self.prec, self.first = float(nu), np.asarray(prec, np.float64), first
        self.params = None if first else np.asarray(y)
        self.y0 = np.asarray(y) if first else None

    def __call__(self, *a):
        return log_g(a[0], self.y0 if self.first else a[2], self.nu, self.prec)


class Model(G.Model):
    """tests/guided_np.py's model record with this potential; `grad` is what its `shifted` needs for gradient=True"""

    def __init__(self, m0, P0, dyn, Q, nu, prec, y):
        super().__init__(m0, P0, dyn, Q, MvtPotential(nu, prec, y[0], first=True), MvtPotential(nu, prec, y[1:]), "mvt", y)
        self.nu, self.prec = float(nu), np.asarray(prec, np.float64)
        self.F, self.b = np.asarray(dyn.params[0][0], float), np.asarray(dyn.params[1][0], float)
        self.tv = False  # time-varying transitions: dyn.params has a row per transition, Q / LQ / F / b above are those of the first

    def trans(self, t):
        """(F, b, Q, chol Q) of the transition into step t >= 1"""
        if not self.tv:
            return self.F, self.b, self.Q, self.LQ
        F, b, LQ = (np.asarray(p[t - 1], float) for p in self.dyn.params)
        return F, b, LQ @ LQ.T, LQ

    def literal(self):
        """(M0, G0, Mt, Gt) of the literal sampler"""
        return L.GaussianInit(self.m0, self.LP0), self.G0, self.dyn, self.Gt


def joint_grad(m, u):
    """the gradient at u (T, d) of log M0(u_0) + G0(u_0) + sum_t [log Mt(u_{t+1} | u_t) + Gt(u_{t+1})] (csmc/independent.py:121-134), in closed form"""
    T = u.shape[0]
    g = np.stack([grad_log_g(u[t], m.y[t], m.nu, m.prec) for t in range(T)])
    g[0] -= np.linalg.inv(m.P0) @ (u[0] - m.m0)
    for t in range(1, T):
        F, b, Q, _ = m.trans(t)
        w = np.linalg.inv(Q) @ (u[t] - (F @ u[t - 1] + b))
        g[t] -= w
        g[t - 1] += F.T @ w
    return g


def guided_kernel(m, N, backward=False, gradient=False):
    """the literal guided sampler of tests/guided_np.py; its gradient variant shifts u by s^2 grad log g_t(u_t)"""
    def shifted(u, scale):
        if not gradient:
            return u
        return u + (scale * scale)[:, None] * np.stack([grad_log_g(u[t], m.y[t], m.nu, m.prec) for t in range(u.shape[0])])

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


# ---- cases: the model on both sides ---------------------------------------------------------------------------------------------------------------------
def case(d, T, rng, nu=4.0, prec=None, nan_rows=(), walk=False, tv=False):
    """linear-Gaussian dynamics with the multivariate-t potential: tests/guided_np.py::sv_case's dynamics, or (walk) the spatial example's random walk
    x_t = x_{t-1} + eps, or (tv) sv_case's dynamics with an F_t, b_t and Q_t of its own for each of the T - 1 transitions; prec: default a dense random SPD
    matrix.  nan_rows: time steps whose observation has a NaN component (the step is flat).
    Returns (device objects (M0, G0, Mt, Gt), literal Model, a trajectory, delta in [0.2, 0.8] / d: proposals that N <= 64 particles can follow at every d)."""
    from aux_ssm_samplers_amd.csmc import GaussianInit, LinearGaussianDynamics, MultivariateTPotential
    if walk:
        F, b, Q, P0, m0 = np.eye(d), np.zeros(d), np.eye(d), np.eye(d), np.zeros(d)
    else:
        F = 0.9 * np.eye(d) + 0.02 * rng.standard_normal((d, d)) / np.sqrt(d)
        b = 0.05 * rng.standard_normal(d)
        Q, P0, m0 = G.spd(d, rng), G.spd(d, rng, 0.5), 0.1 * rng.standard_normal(d)
    if tv:
        F = F + 0.05 * rng.standard_normal((T - 1, d, d)) / np.sqrt(d)
        b = b + 0.05 * rng.standard_normal((T - 1, d))
        Q = np.stack([G.spd(d, rng) for _ in range(T - 1)])
    Ft, bt, Qt = (np.broadcast_to(a, (T - 1,) + a.shape[-n:]) for a, n in ((F, 2), (b, 1), (Q, 2)))
    if prec is None:
        A = rng.standard_normal((d, d))
        prec = 1.5 * np.eye(d) + 0.8 * (A @ A.T) / d
        prec = 0.5 * (prec + prec.T)
    x = np.zeros((T, d))
    x[0] = m0 + np.linalg.cholesky(P0) @ rng.standard_normal(d)
    for t in range(1, T):
        x[t] = Ft[t - 1] @ x[t - 1] + bt[t - 1] + np.linalg.cholesky(Qt[t - 1]) @ rng.standard_normal(d)
    Lc = np.linalg.cholesky(np.linalg.inv(prec))
    y = x + (rng.standard_normal((T, d)) @ Lc.T) / np.sqrt(rng.chisquare(nu, T) / nu)[:, None]
    for i, t in enumerate(nan_rows):
        y[t, i % d] = np.nan
    M0, Mt = GaussianInit(m0=m0, P0=P0), LinearGaussianDynamics(F=F, b=b, Q=Q)
    dev = (M0, MultivariateTPotential(nu=nu, prec=prec, y=y[0]), Mt, MultivariateTPotential(nu=nu, prec=prec, params=y[1:]))
    m = Model(m0, P0, L.LinearGaussianDynamics(F, b, np.linalg.cholesky(Q), T), Qt[0], nu, prec, y)
    m.tv = tv
    return dev, m, x, (0.2 + 0.6 * rng.random(T)) / d


def program(dev, grad=False):
    """the same model with the potential as user source (device_models.BUILTIN_MVT[_GRAD]), theta = [nu, prec row-major]"""
    from aux_ssm_samplers_amd.csmc import DevicePotential, device_models as U
    M0, G0, Mt, Gt = dev
    src = U.BUILTIN_MVT_GRAD if grad else U.BUILTIN_MVT
    theta = np.concatenate([[G0.nu], np.reshape(G0.prec, -1)])
    d = G0.dx
    return M0, DevicePotential(src, y=G0.y, theta=theta, p=d), Mt, DevicePotential(src, params=Gt.params, theta=theta, p=d)
