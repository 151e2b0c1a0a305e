"""TEST INFRASTRUCTURE ONLY: the cells of the conjugate dynamics step's GPU tests (tests/test_gpu_dynamics_theta.py) and their references, computed once per
process by the literal restatement tests/dynamics_theta_np.py and shared by the tests that need them."""
import copy
import functools

import numpy as np

from tests import dynamics_theta_np as NP

L = NP.SEGMENT_LEN
# T: the smallest, one more, one transition short of a segment (L - 1 steps: L - 2 transitions), a segment and its neighbours (L + 1 steps: exactly one full
# segment; L + 2: one transition into the second), three segments and a ragged tail
T_CASES = (2, 3, L - 1, L + 1, L + 2, 3 * L + 38)
C_CASES = (1, 3, 33, 70)        # one chain, a few, more than half a wave, more than one block of 64 chains
D_CASES = (1, 2, 3, 4)
C_MAX, T_MAX = max(C_CASES), max(T_CASES)
FP64_BAR = 1e-9                 # the project's fp64 bar, relative to the largest entry of each matrix

GAMMA_SHAPES = (0.3, 1.0, 2.5, 500.0, 32768.0)


def moments_within(g, shape, nse=5.0):
    """sample mean and variance of Gamma(shape, 1) draws within nse standard errors (the variance's from the sample fourth moment)"""
    n = g.size
    mean, var = g.mean(), g.var(ddof=1)
    se_mean = np.sqrt(shape / n)
    mu4 = np.mean((g - mean) ** 4)
    se_var = np.sqrt(max(mu4 - var * var, 0.0) / n)
    return abs(mean - shape) <= nse * se_mean and abs(var - shape) <= nse * se_var, (mean, var, se_mean, se_var)


@functools.lru_cache(maxsize=None)
def problem(d, f32=False):
    """C_MAX stable VAR(1) trajectories of T_MAX steps (a cell takes the leading [:C, :T]), a proper prior, and explicit noise for the draw.
    f32: everything the device is handed in float32 is rounded to float32 here and held as float64: the reference sees the inputs the device sees."""
    r = (lambda a: np.asarray(a, np.float32).astype(np.float64)) if f32 else (lambda a: np.asarray(a, np.float64))
    rng = np.random.default_rng(4000 + d)
    n = d + 1
    F = 0.7 * np.eye(d) + 0.1 * rng.standard_normal((d, d))
    b = 0.3 * rng.standard_normal(d)
    Lq = np.tril(0.2 * rng.standard_normal((d, d))) + 0.5 * np.eye(d)
    x = np.zeros((C_MAX, T_MAX, d))
    x[:, 0] = rng.standard_normal((C_MAX, d))
    for t in range(T_MAX - 1):
        x[:, t + 1] = x[:, t] @ F.T + b + rng.standard_normal((C_MAX, d)) @ Lq.T
    M0 = 0.1 * rng.standard_normal((d, n))
    a = rng.standard_normal((n, n))
    K0 = 0.5 * np.eye(n) + 0.1 * a @ a.T
    c = rng.standard_normal((d, d))
    Psi0 = np.eye(d) + 0.2 * c @ c.T
    ew, ea = rng.standard_normal((C_MAX, d, d)), rng.standard_normal((C_MAX, d, n))
    u = rng.random((C_MAX, d))          # (spreads the explicit chi values: chi_for)
    return dict(d=d, x=r(x), M0=M0, K0=0.5 * (K0 + K0.T), nu0=d + 2.5, Psi0=0.5 * (Psi0 + Psi0.T), ew=r(ew), ea=r(ea), u=u,
                F0=r(0.5 * np.eye(d)), b0=r(np.zeros(d)), Q0=r(np.eye(d)))


def chi_for(p, T, f32=False):
    """explicit chi-square values of the right size for T steps: nu_n - i plus a spread, positive"""
    d = p["d"]
    nun = p["nu0"] + T - 1
    chi = (nun - np.arange(d)) * (0.5 + p["u"])
    return np.asarray(chi, np.float32).astype(np.float64) if f32 else chi


@functools.lru_cache(maxsize=None)
def reference(d, T, f32=False):
    """for all C_MAX chains at T steps: (stats flat (C, .), post flat (C, .), Q (C, d, d), A (C, d, d + 1)) by the restatement"""
    p = problem(d, f32)
    x = p["x"][:, :T]
    S = NP.stats(x)
    post = NP.posterior(S, T - 1, p["M0"], p["K0"], p["nu0"], p["Psi0"])
    Q, A = NP.draw(post, chi_for(p, T, f32), p["ew"], p["ea"])
    return NP.stats_flat(x), NP.post_flat(post), Q, A


def rel(got, want, axes):
    """largest error relative to the largest entry of each matrix (per chain)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.max(np.max(np.abs(got - want), axis=axes) / np.max(np.abs(want), axis=axes)))


def blocks(d):
    """slices of the flat statistics [S_zz | S_xz | S_xx] and of post_out [M_n | K_n | nu_n | Psi_n]"""
    n = d + 1
    s = np.cumsum([0, n * n, d * n, d * d])
    q = np.cumsum([0, d * n, n * n, 1, d * d])
    return [slice(s[i], s[i + 1]) for i in range(3)], [slice(q[i], q[i + 1]) for i in range(4)]


def with_dynamics(model, F, Q, b):
    """a FRESH model (no device state) that is `model` with the time-invariant dynamics (F, Q, b)"""
    m = copy.copy(model)
    n = m.T - 1
    F, Q, b = (np.array(a, np.float64) for a in (F, Q, b))
    m.Fs, m.Qs, m.bs = np.broadcast_to(F, (n,) + F.shape), np.broadcast_to(Q, (n,) + Q.shape), np.broadcast_to(b, (n,) + b.shape)
    if hasattr(m, "F"):
        m.F, m.Q, m.b = F, Q, b
    m._dev = {}
    return m


# ---- joint ground truth: the posterior of (F, b, log Q, x_0, x_{T-1}) of a scalar linear-Gaussian model by quadrature -----------------------------------------
def joint_model(T=6):
    """a scalar LGConcatModel's ingredients with data that pins the posterior down moderately, and an informative MNIW prior"""
    rng = np.random.default_rng(2024)
    F, b, Q, R = 0.6, 0.3, 0.25, 0.3
    x = np.zeros(T)
    x[0] = 0.5
    for t in range(T - 1):
        x[t + 1] = F * x[t] + b + np.sqrt(Q) * rng.standard_normal()
    y = x + np.sqrt(R) * rng.standard_normal(T)
    return dict(T=T, y=y, R=R, m0=0.0, P0=1.0, F=F, b=b, Q=Q, M0=np.array([[0.5, 0.2]]), K0=np.array([[4.0, 0.5], [0.5, 6.0]]), nu0=8.0,
                Psi0=np.array([[2.0]]))


def joint_quadrature(j, n):
    """posterior means of (F, b, log Q, x_0, x_{T-1}) on an n^3 midpoint grid over (F, b, log Q): the state integrated out by a Kalman filter (the weight
    is prior x marginal likelihood) and a backward smoother (the conditional means of the states)"""
    T, y, R = j["T"], j["y"], j["R"]
    M0, K0, nu0, Psi0 = j["M0"][0], j["K0"], j["nu0"], j["Psi0"][0, 0]

    def mid(lo, hi):
        h = (hi - lo) / n
        return lo + h * (np.arange(n) + 0.5)

    Fg, bg, sg = np.meshgrid(mid(-2.5, 3.5), mid(-3.0, 3.5), mid(-4.5, 3.5), indexing="ij")
    Q = np.exp(sg)
    dA0, dA1 = Fg - M0[0], bg - M0[1]
    quad = K0[0, 0] * dA0 * dA0 + 2 * K0[0, 1] * dA0 * dA1 + K0[1, 1] * dA1 * dA1
    # log prior in (F, b, s = log Q): IW(nu0, Psi0) in Q (d = 1) x the Jacobian Q, MN(M0, Q, K0^-1) in A
    lp = -0.5 * (nu0 + 2.0) * sg - 0.5 * Psi0 / Q + sg - 1.0 * sg - 0.5 * quad / Q
    m, P = np.full(Fg.shape, j["m0"]), np.full(Fg.shape, j["P0"])
    ms, Ps, mp, Pp = [], [], [], []
    ll = np.zeros(Fg.shape)
    for t in range(T):
        if t > 0:
            m, P = Fg * m + bg, Fg * Fg * P + Q
        mp.append(m), Pp.append(P)
        S = P + R
        ll += -0.5 * np.log(2 * np.pi * S) - 0.5 * (y[t] - m) ** 2 / S
        K = P / S
        m, P = m + K * (y[t] - m), (1.0 - K) * P
        ms.append(m), Ps.append(P)
    sm = ms[-1]
    xT = sm
    for t in range(T - 2, -1, -1):
        G = Ps[t] * Fg / Pp[t + 1]
        sm = ms[t] + G * (sm - mp[t + 1])
    lw = lp + ll
    w = np.exp(lw - lw.max())
    w /= w.sum()
    return np.array([np.sum(w * Fg), np.sum(w * bg), np.sum(w * sg), np.sum(w * sm), np.sum(w * xT)])
