"""Guided (locally optimal) auxiliary proposals as GENERIC protocol objects for the literal NumPy cSMC (oracle/csmc_np.py::get_generic_kernel).

Test infrastructure only.  The algorithm, restated (reference: examples/stochastic_volatility/auxiliary_guided_csmc.py with csmc/generic.py:56-72):
with s_t = sqrt(delta_t / 2), u_t = x*_t + s_t eps_aux_t, pred_0 = m0 / P = P0 and pred_t = mean(x_{t-1}^A) / P = Q for t >= 1,

    K_t = solve(P + s_t^2 I, P)^T,   Lambda_t = P - K_t P,   L_t = cholesky((Lambda_t + Lambda_t^T) / 2)   (non-finite entries -> those of s_t I)
    x ~ N(mu_t, Lambda_t),           mu_t = pred + K_t (u~_t - pred),   u~_t = u_t [+ s_t^2 grad_x log g_t(u_t) with gradient]
    log w = log g_t(x) + log N(x; pred, P) + sum_k log N(x_k; u_{t,k}, s_t^2) - log N(x; mu_t, Lambda_t)      (the third term at u, not u~)

`tables="solve"` builds K and L as written; `tables="eig"` builds the same matrices from the eigen-decomposition of P (K and Lambda share P's
eigenvectors; L from a QR factorisation) -- a second, independent route whose distance from the first is the rounding floor of the problem."""
import numpy as np

from oracle import csmc_np as L


def tables(P, s, how="solve"):
    """(K, chol Lambda) of one step"""
    P = np.asarray(P, np.float64)
    d = P.shape[0]
    if how == "solve":
        K = np.linalg.solve(P + s * s * np.eye(d), P).T
        Lam = P - K @ P
        with np.errstate(invalid="ignore"):
            try:
                C = np.linalg.cholesky(0.5 * (Lam + Lam.T))
            except np.linalg.LinAlgError:
                C = np.full((d, d), np.nan)
    else:
        lam, V = np.linalg.eigh(P)
        K = (V * (lam / (lam + s * s))) @ V.T
        R = np.linalg.qr(np.sqrt(lam * s * s / (lam + s * s))[:, None] * V.T, mode="r")  # Lambda = R^T R
        C = (R * np.sign(np.diag(R))[:, None]).T
    return K, np.where(np.isfinite(C), C, s * np.eye(d))


def grad_potential(kind, x, y, sig=1.0):
    """d log g_t / dx of oracle.csmc_np.ObsPotential's kinds (None: flat), in closed form"""
    if kind is None:
        return np.zeros_like(x)
    y = np.asarray(y, x.dtype)
    if kind == "sv":
        with np.errstate(over="ignore", invalid="ignore"):
            v = 0.5 * (y * y * np.exp(-x) - 1.0)
    else:
        v = (y - x) / (sig * sig)
    return np.where(np.isnan(v), 0.0, v) if kind != "gauss" else v


class Model:
    """the model a guided kernel needs: prior N(m0, P0), dynamics `dyn` (an oracle.csmc_np Dynamics with .mean(x, params) and covariance Q), the
    potentials G0 / Gt (oracle.csmc_np protocol objects, e.g. ObsPotential) and, for gradient=True, kind / y / sig of the potential"""

    def __init__(self, m0, P0, dyn, Q, G0, Gt, kind=None, y=None, sig=1.0):
        self.m0, self.P0, self.dyn, self.Q, self.G0, self.Gt = np.asarray(m0, float), np.atleast_2d(np.asarray(P0, float)), dyn, np.atleast_2d(np.asarray(Q, float)), G0, Gt
        self.kind, self.y, self.sig = kind, y, sig
        self.LP0, self.LQ = np.linalg.cholesky(self.P0), np.linalg.cholesky(self.Q)


def _weight(g, x, pred, LP, u, s, mu, C):
    out = g + L._mvn_chol_logpdf(x, pred, LP)
    out = out + np.sum(L.norm_logpdf(x, u, s), axis=-1)
    return out - L._mvn_chol_logpdf(x, mu, C)


class GuidedM0(L.Distribution):
    def __init__(self, m, ut, K, C):
        self.mu, self.C = m.m0 + K @ (ut - m.m0), C

    def sample(self, key, N):
        return self.mu[None, :] + key @ self.C.T


class GuidedG0:
    def __init__(self, m, u, s, ut, K, C):
        self.m, self.u, self.s, self.mu, self.C = m, u, s, m.m0 + K @ (ut - m.m0), C

    def __call__(self, x):
        return _weight(self.m.G0(x), x, self.m.m0, self.m.LP0, self.u, self.s, self.mu, self.C)


class GuidedMt(L.Dynamics):
    def __init__(self, m, params):
        self.m, self.params = m, params  # (u~, K, C, dynamics' params), leading axis T - 1

    def sample(self, key, x_prev, params):
        ut, K, C, dp = params
        pred = self.m.dyn.mean(x_prev, dp)
        return pred + (ut - pred) @ K.T + key @ C.T


class GuidedGt:
    def __init__(self, m, params):
        self.m, self.params = m, params  # (u, s, u~, K, C, dynamics' params, potential's params)

    def __call__(self, x, x_prev, params):
        u, s, ut, K, C, dp, gp = params
        pred = self.m.dyn.mean(x_prev, dp)
        mu = pred + (ut - pred) @ K.T
        return _weight(self.m.Gt(x, x_prev, gp), x, pred, self.m.LQ, u, s, mu, C)


def shifted(m, u, scale, gradient):
    """u~: u, or u + s^2 grad log g_t(u) row by row"""
    if not gradient:
        return u
    g = np.stack([grad_potential(m.kind, u[t], None if m.y is None else m.y[t], m.sig) for t in range(u.shape[0])])
    return u + (scale * scale)[:, None] * g


def factory(m, gradient=False, how="solve"):
    def f(u, scale):
        T = u.shape[0]
        tab = [tables(m.P0 if t == 0 else m.Q, float(scale[t]), how) for t in range(T)]
        Ks, Cs = np.stack([a for a, _ in tab]), np.stack([b for _, b in tab])
        ut = shifted(m, u, scale, gradient)
        return (GuidedM0(m, ut[0], Ks[0], Cs[0]), GuidedG0(m, u[0], scale[0], ut[0], Ks[0], Cs[0]),
                GuidedMt(m, (ut[1:], Ks[1:], Cs[1:], m.dyn.params)),
                GuidedGt(m, (u[1:], scale[1:], ut[1:], Ks[1:], Cs[1:], m.dyn.params, m.Gt.params)))
    return f


def get_kernel(m, N, backward=False, gradient=False, how="solve"):
    """(init, kernel) of the literal guided sampler; kernel(Noise, x, delta) -> (x, ancestors, history)"""
    return L.get_generic_kernel(factory(m, gradient, how), N, backward, m.dyn)


def closed_form(m, t, x, x_prev, u, s):
    """log g_t(x) + log N(u_t; pred, P + s^2 I): what the guided weight without gradient equals, with no K or Lambda in it"""
    d = m.m0.shape[0]
    if t == 0:
        g, pred, P = m.G0(x), np.broadcast_to(m.m0, x.shape), m.P0
    else:
        g, pred, P = m.Gt(x, x_prev, L._tree_index(m.Gt.params, t - 1)), m.dyn.mean(x_prev, L._tree_index(m.dyn.params, t - 1)), m.Q
    return g + L._mvn_chol_logpdf(np.broadcast_to(u, pred.shape), pred, np.linalg.cholesky(P + s * s * np.eye(d)))


# ---- the cases of the test files: the model on both sides (device family objects, literal objects) -------------------------------------------------------
CASES = [(1, 1024, 60), (2, 100, 40), (4, 65, 33), (8, 25, 20), (30, 25, 25), (32, 64, 12),
         (1, 512, 3)]  # eight full waves: the guided kernels have no instantiation of that shape, the generic workgroup runs it (csmc.hip::fwd_kernel)


def spd(d, rng, base=0.3, small=0.05):
    A = rng.standard_normal((d, d))
    return base * np.eye(d) + small * (A @ A.T) / d


def sv_case(d, T, rng, potential="sv", sig=0.7):
    """linear-Gaussian dynamics (F = 0.9 I + small, Q = 0.3 I + small SPD, P0 alike) with the SV or the Gaussian-observation potential;
    returns (device objects (M0, G0, Mt, Gt), literal Model, a trajectory to start from, delta in [0.2, 0.8])"""
    from aux_ssm_samplers_amd.csmc import GaussianInit, LinearGaussianDynamics, SVPotential, GaussianObsPotential
    F = 0.9 * np.eye(d) + 0.02 * rng.standard_normal((d, d)) / np.sqrt(d)
    b = 0.05 * rng.standard_normal(d)
    Q, P0, m0 = spd(d, rng), spd(d, rng, 0.5), 0.1 * rng.standard_normal(d)
    x = np.zeros((T, d))
    x[0] = m0 + np.linalg.cholesky(P0) @ rng.standard_normal(d)
    for t in range(1, T):
        x[t] = F @ x[t - 1] + b + np.linalg.cholesky(Q) @ rng.standard_normal(d)
    M0, Mt = GaussianInit(m0=m0, P0=P0), LinearGaussianDynamics(F=F, b=b, Q=Q)
    dyn = L.LinearGaussianDynamics(F, b, np.linalg.cholesky(Q), T)
    if potential == "sv":
        y = np.exp(0.5 * x) * rng.standard_normal((T, d))
        dev = (M0, SVPotential(y=y[0]), Mt, SVPotential(params=y[1:]))
        m = Model(m0, P0, dyn, Q, L.ObsPotential("sv", y[0], first=True), L.ObsPotential("sv", y[1:]), "sv", y)
    else:
        y = x + sig * rng.standard_normal((T, d))
        dev = (M0, GaussianObsPotential(sig=sig, y=y[0]), Mt, GaussianObsPotential(sig=sig, params=y[1:]))
        m = Model(m0, P0, dyn, Q, L.ObsPotential("gauss", y[0], sig, first=True), L.ObsPotential("gauss", y[1:], sig), "gauss", y, sig)
    return dev, m, x, 0.2 + 0.6 * rng.random(T)


def noise(T, N, d, rng):
    return dict(eps_aux=rng.standard_normal((T, d)), eps_prop=rng.standard_normal((T, N, d)), u_res=rng.random((T - 1, N)), u_bwd=rng.random(T))


def lorenz_case(T, seed=4):
    """config C4's model: Lorenz-63 Euler-Maruyama transition (dx = 3), (x2, x3) observed sparsely -- the transition mean is not linear"""
    from tests.helpers import lorenz_setup
    M0, Mt, G0, Gt, xtrue, y, sig_y = lorenz_setup(T, seed=seed)
    LQ = np.asarray(Mt.chol())
    dyn = L.Lorenz63EM(np.asarray(Mt.theta, float), Mt.dt, LQ, T)
    m = Model(M0.m0, M0.P0, dyn, LQ @ LQ.T, L.ObsPotential("masked", y[0], sig_y, first=True), L.ObsPotential("masked", y[1:], sig_y), "masked", y, sig_y)
    return (M0, G0, Mt, Gt), m, xtrue


def rare_event_case(T, rho=0.9, r=0.5, yv=2.0):
    """the rare-event model in the closed family: AR(1) with unit marginals, one Gaussian observation of x_{T-1} (NaN everywhere else)"""
    from aux_ssm_samplers_amd.csmc import GaussianInit, LinearGaussianDynamics, MaskedGaussianObsPotential
    y = np.full((T, 1), np.nan)
    y[-1] = yv
    q = 1 - rho ** 2
    M0, Mt = GaussianInit(m0=[0.0], P0=[[1.0]]), LinearGaussianDynamics(F=[[rho]], b=[0.0], Q=[[q]])
    dev = (M0, MaskedGaussianObsPotential(sig=r, y=y[0]), Mt, MaskedGaussianObsPotential(sig=r, params=y[1:]))
    dyn = L.LinearGaussianDynamics(np.array([[rho]]), np.zeros(1), np.array([[np.sqrt(q)]]), T)
    m = Model(np.zeros(1), [[1.0]], dyn, [[q]], L.ObsPotential("masked", y[0], r, first=True), L.ObsPotential("masked", y[1:], r), "masked", y, r)
    return dev, m, np.linspace(0.0, yv, T)[:, None]
