"""Synthetic workloads of the BASELINE configurations (C1/C2 linear-Gaussian, C3 stochastic volatility, C4 Lorenz-63, C5 dense and
batched-scalar spatial models): the model builders shared by `bench.py`, the measurement scripts under `tools/` and the tests.  Plain NumPy recipes with
fixed seeds -- no oracle import here (`bench.py` and `tools/` must not reach the oracle through this module), nothing of the hot path."""
import numpy as np
from scipy.linalg import block_diag


def rot(theta):
    c, s = np.cos(theta), np.sin(theta)
    return np.array([[c, -s], [s, c]])


def lg_model(T, d, seed=0, dtype=np.float64):
    """SURVEY 8(d) C1/C2 linear-Gaussian SSM: F = 0.95*blkdiag(Rot(pi/16)[, Rot(pi/7)]), Q = 0.1 I,
    y_t = x_t + N(0, 0.5 I), m0 = 0, P0 = I.  Data from numpy Generator(PCG64(seed))."""
    assert d in (1, 2, 3, 4)
    if d == 1:
        F = np.array([[0.95]])
    elif d == 2:
        F = 0.95 * rot(np.pi / 16)
    elif d == 3:  # (not a BASELINE shape: the smoother's benchmark leg) a third, unrotated component
        F = 0.95 * block_diag(rot(np.pi / 16), np.eye(1))
    else:
        F = 0.95 * block_diag(rot(np.pi / 16), rot(np.pi / 7))
    Q = 0.1 * np.eye(d)
    Robs = 0.5 * np.eye(d)
    rng = np.random.Generator(np.random.PCG64(seed))
    x = np.zeros((T, d))
    x[0] = rng.standard_normal(d)
    for t in range(1, T):
        x[t] = F @ x[t - 1] + np.sqrt(0.1) * rng.standard_normal(d)
    y = x + np.sqrt(0.5) * rng.standard_normal((T, d))
    return dict(m0=np.zeros(d, dtype), P0=np.eye(d, dtype=dtype), F=F.astype(dtype), Q=Q.astype(dtype),
                b=np.zeros(d, dtype), Hobs=np.eye(d, dtype=dtype), Robs=Robs.astype(dtype),
                cobs=np.zeros(d, dtype), y=y.astype(dtype), x_true=x.astype(dtype))


def sv_setup(T, d, seed=0, phi=0.9, tau=2.0, rho=0.25):
    """model.py:34-53 (nu = 0): F = phi I, Q = P0 = U / (1 - phi^2), U = tau (rho + (1 - rho) I); data as model.py:11-31."""
    rng = np.random.Generator(np.random.PCG64(seed))
    U = tau * rho * np.ones((d, d))
    U[np.diag_indices(d)] = tau
    Q = U / (1 - phi ** 2)
    F, b, m0 = phi * np.eye(d), np.zeros(d), np.zeros(d)
    L = np.linalg.cholesky(Q)
    x = np.zeros((T, d))
    x[0] = L @ rng.standard_normal(d)
    for t in range(1, T):
        x[t] = F @ x[t - 1] + L @ rng.standard_normal(d)
    y = np.exp(0.5 * x) * rng.standard_normal((T, d))
    return y, x, (m0, Q, F, Q, b)


def spatial_precision(grid, tau=-0.25, r_y=1):
    """The spatial example's precision matrix on a grid x grid lattice flattened row by row: entry ((i, j), (k, l)) is tau^(|i - k| + |j - l|) where that
    lattice distance is <= r_y, else 0 (grid 2: the 4 x 4 matrix examples/spatial/model.py:43-46 prints)."""
    ii, jj = np.divmod(np.arange(grid * grid), grid)
    dist = np.abs(ii[:, None] - ii[None, :]) + np.abs(jj[:, None] - jj[None, :])
    return np.where(dist <= r_y, float(tau) ** dist, 0.0)


def spatial_setup(T, grid, seed=0, sigma_x=1.0, nu=1.0, tau=-0.25, r_y=1):
    """The spatial example (examples/spatial/model.py) on a grid x grid lattice, dx = grid^2: x_0 ~ N(0, sigma_x^2 I), a random walk
    x_t = x_{t-1} + sigma_x eps_t, and multivariate Student-t observations y_t = x_t + chol(prec^-1) z_t / sqrt(w_t / nu), w_t ~ chi^2_nu, with the
    precision matrix of spatial_precision.  Returns (M0, Mt, G0, Gt, x, y, prec): the model as the cSMC kernels take it, the simulated states and data."""
    from aux_ssm_samplers_amd.csmc import GaussianInit, LinearGaussianDynamics, MultivariateTPotential
    rng = np.random.Generator(np.random.PCG64(seed))
    d = grid * grid
    prec = spatial_precision(grid, tau, r_y)
    Lc = np.linalg.cholesky(np.linalg.inv(prec))
    x = np.cumsum(sigma_x * rng.standard_normal((T, d)), axis=0)
    w = rng.chisquare(nu, size=T)
    y = x + (rng.standard_normal((T, d)) @ Lc.T) / np.sqrt(w / nu)[:, None]
    M0 = GaussianInit(m0=np.zeros(d), P0=sigma_x ** 2 * np.eye(d))
    Mt = LinearGaussianDynamics(F=np.eye(d), b=np.zeros(d), Q=sigma_x ** 2 * np.eye(d))
    G0 = MultivariateTPotential(nu=nu, prec=prec, y=y[0])
    Gt = MultivariateTPotential(nu=nu, prec=prec, params=y[1:])
    return M0, Mt, G0, Gt, x, y, prec


def spatial_kalman_setup(T, grid, seed=0, sigma_x=1.0, nu=1.0, tau=-0.25, r_y=1, order=1):
    """The spatial example for its auxiliary Kalman sampler (examples/spatial/auxiliary_kalman.py): the data of spatial_setup (same recipe, same seed -> same
    x and y) and the batched dynamics of model.py:103-112 (F = 1, Q = P0 = sigma_x^2, b = m0 = 0 per component).
    Returns (model, x0): a kalman.MVTModel and a start state of the reference's shape (T, d, 1) -- the simulated states."""
    from aux_ssm_samplers_amd.kalman import MVTModel
    *_, x, y, prec = spatial_setup(T, grid, seed, sigma_x, nu, tau, r_y)
    d = grid * grid
    F, Q, b = np.ones((d, 1, 1)), sigma_x ** 2 * np.ones((d, 1, 1)), np.zeros((d, 1))
    return MVTModel(y, b, Q, F, Q, b, nu, prec, order=order), x[..., None]


def lgssm_tracking_setup(T, dx, dy, seed=0):
    """A partially observed linear-Gaussian state-space model, 1 <= dy <= dx: x_0 ~ N(0, I), x_t = F x_{t-1} + eps_t with a stable banded F (0.9 on the
    diagonal, 0.05 / -0.05 beside it) and Q = 0.25 I, observations y_t ~ N(H x_t, R) with a dense H (every entry non-zero: each sensor sees a mixture of all
    components) and a non-diagonal R of condition number <= 50 (an orthogonal basis with eigenvalues between 0.1 and 2).
    Returns (M0, Mt, G0, Gt, x, y, H, R): the model as the cSMC kernels take it (csmc.LinearGaussianPotential), the simulated states and data."""
    from aux_ssm_samplers_amd.csmc import GaussianInit, LinearGaussianDynamics, LinearGaussianPotential
    rng = np.random.Generator(np.random.PCG64(seed))
    F = 0.9 * np.eye(dx) + 0.05 * np.eye(dx, k=1) - 0.05 * np.eye(dx, k=-1)
    Q = 0.25 * np.eye(dx)
    H = rng.standard_normal((dy, dx)) / np.sqrt(dx)
    H = np.where(np.abs(H) < 0.05 / np.sqrt(dx), 0.05 / np.sqrt(dx), H)
    U = np.linalg.qr(rng.standard_normal((dy, dy)))[0]
    R = (U * np.linspace(0.1, 2.0, dy)) @ U.T
    R = 0.5 * (R + R.T)
    x = np.zeros((T, dx))
    x[0] = rng.standard_normal(dx)
    for t in range(1, T):
        x[t] = F @ x[t - 1] + 0.5 * rng.standard_normal(dx)
    y = x @ H.T + rng.standard_normal((T, dy)) @ np.linalg.cholesky(R).T
    M0, Mt = GaussianInit(m0=np.zeros(dx), P0=np.eye(dx)), LinearGaussianDynamics(F=F, b=np.zeros(dx), Q=Q)
    return M0, Mt, LinearGaussianPotential(H=H, R=R, y=y[0]), LinearGaussianPotential(H=H, R=R, params=y[1:]), x, y, H, R


def poisson_setup(T, dx, seed=0):
    """Multivariate counts with a log link: a stable linear-Gaussian log-intensity x_t = F x_{t-1} + b + eps_t with the banded F of lgssm_tracking_setup (0.9 on
    the diagonal, 0.05 / -0.05 beside it), Q = 0.04 I, b = (I - F) 1 so that the stationary mean is 1 in every component, x_0 ~ N(1, P0) with P0 = 0.2 I (about
    the stationary variance), and y_{t,k} ~ Poisson(exp(x_{t,k})): intensities around e, counts mostly 0 .. 30.
    Returns (M0, Mt, G0, Gt, x, y): the model as the cSMC kernels take it (csmc.PoissonPotential), the simulated states and counts (float64)."""
    from aux_ssm_samplers_amd.csmc import GaussianInit, LinearGaussianDynamics, PoissonPotential
    rng = np.random.Generator(np.random.PCG64(seed))
    F = 0.9 * np.eye(dx) + 0.05 * np.eye(dx, k=1) - 0.05 * np.eye(dx, k=-1)
    m0 = np.ones(dx)
    b = m0 - F @ m0
    Q, P0 = 0.04 * np.eye(dx), 0.2 * np.eye(dx)
    x = np.zeros((T, dx))
    x[0] = m0 + np.sqrt(0.2) * rng.standard_normal(dx)
    for t in range(1, T):
        x[t] = F @ x[t - 1] + b + 0.2 * rng.standard_normal(dx)
    y = rng.poisson(np.exp(x)).astype(np.float64)
    M0, Mt = GaussianInit(m0=m0, P0=P0), LinearGaussianDynamics(F=F, b=b, Q=Q)
    return M0, Mt, PoissonPotential(y=y[0]), PoissonPotential(params=y[1:]), x, y


def poisson_kalman_setup(T, dx, seed=0, order=1):
    """The model of poisson_setup for the auxiliary Kalman sampler (same recipe, same seed -> same x and y).
    Returns (model, x0): a kalman.PoissonModel and a start state (T, dx) -- the simulated log-intensities."""
    from aux_ssm_samplers_amd.kalman import PoissonModel
    M0, Mt, _, _, x, y = poisson_setup(T, dx, seed)
    return PoissonModel(y, M0.m0, M0.P0, Mt.F, Mt.Q, Mt.b, order=order), x


def logistic_setup(T, dx, family="binomial", seed=0):
    """Binomial or negative-binomial data with a logit link: AR(1) log-odds x_t = 0.9 x_{t-1} + eps_t per component, Q = 0.04 I, m0 = b = 0, P0 = 0.2 I (about
    the stationary variance).  family "binomial": trials drawn from 1 .. 40 per observation, component 0 binary (trials = 1), y ~ Binomial(trials, sigma(x));
    "negbinomial": r = 3, y ~ NB(3, p = sigma(x)) (mean 3 e^x), drawn as a Gamma-Poisson mixture.
    Returns (M0, Mt, G0, Gt, x, y, par): the model as the cSMC kernels take it (csmc.BinomialPotential / NegBinomialPotential), the simulated log-odds and data
    (float64) and the family's parameter -- the trials (T, dx), or r = 3.0."""
    from aux_ssm_samplers_amd.csmc import GaussianInit, LinearGaussianDynamics, BinomialPotential, NegBinomialPotential
    rng = np.random.Generator(np.random.PCG64(seed))
    F, Q, P0 = 0.9 * np.eye(dx), 0.04 * np.eye(dx), 0.2 * np.eye(dx)
    m0, b = np.zeros(dx), np.zeros(dx)
    x = np.zeros((T, dx))
    x[0] = np.sqrt(0.2) * rng.standard_normal(dx)
    for t in range(1, T):
        x[t] = 0.9 * x[t - 1] + 0.2 * rng.standard_normal(dx)
    if family == "binomial":
        trials = rng.integers(1, 41, size=(T, dx)).astype(np.float64)
        trials[:, 0] = 1.0
        y = rng.binomial(trials.astype(np.int64), 1.0 / (1.0 + np.exp(-x))).astype(np.float64)
        G0, Gt, par = BinomialPotential(trials[0], y=y[0]), BinomialPotential(trials[1:], params=y[1:]), trials
    elif family == "negbinomial":
        y = rng.poisson(rng.gamma(3.0, np.exp(x))).astype(np.float64)
        G0, Gt, par = NegBinomialPotential(3.0, y=y[0]), NegBinomialPotential(3.0, params=y[1:]), 3.0
    else:
        raise ValueError(f"family must be 'binomial' or 'negbinomial', got {family!r}")
    return GaussianInit(m0=m0, P0=P0), LinearGaussianDynamics(F=F, b=b, Q=Q), G0, Gt, x, y, par


def logistic_kalman_setup(T, dx, family="binomial", seed=0, order=1):
    """The model of logistic_setup for the auxiliary Kalman sampler (same recipe, same seed -> same x and y).
    Returns (model, x0): a kalman.BinomialModel or kalman.NegBinomialModel and a start state (T, dx) -- the simulated log-odds."""
    from aux_ssm_samplers_amd.kalman import BinomialModel, NegBinomialModel
    M0, Mt, _, _, x, y, par = logistic_setup(T, dx, family, seed)
    model = BinomialModel if family == "binomial" else NegBinomialModel
    return model(y, par, M0.m0, M0.P0, Mt.F, Mt.Q, Mt.b, order=order), x


def poisson_lin_setup(T, dx, dy, seed=0, order=1):
    """Poisson counts through a loading matrix (a Poisson linear dynamical system): dy count channels on a dx-dimensional linear-Gaussian latent,
    y_{t,j} ~ Poisson(exp(h_j' x_t + c_j)).  F = 0.9 I with 0.05 / -0.05 beside the diagonal (poisson_setup's), m0 = b = 0, Q = 0.04 I, P0 = 0.2 I (about
    the stationary variance); H = N(0, 1) / sqrt(dx) with entries of magnitude below 0.1 set to 0.1, c ~ U(0, 2): rates around e, counts mostly 0 .. 30 with
    occasional counts above 100 at large loadings.
    Returns (model, x0, H, c): a kalman.PoissonLinearModel, a start state (T, dx) -- the simulated latent path --, the loading matrix and the offsets."""
    from aux_ssm_samplers_amd.kalman import PoissonLinearModel
    rng = np.random.Generator(np.random.PCG64(seed))
    F = 0.9 * np.eye(dx) + 0.05 * np.eye(dx, k=1) - 0.05 * np.eye(dx, k=-1)
    m0, b = np.zeros(dx), np.zeros(dx)
    Q, P0 = 0.04 * np.eye(dx), 0.2 * np.eye(dx)
    H = rng.standard_normal((dy, dx)) / np.sqrt(dx)
    H = np.where(np.abs(H) < 0.1, 0.1, H)
    c = 2.0 * rng.random(dy)
    x = np.zeros((T, dx))
    x[0] = np.sqrt(0.2) * rng.standard_normal(dx)
    for t in range(1, T):
        x[t] = F @ x[t - 1] + 0.2 * rng.standard_normal(dx)
    y = rng.poisson(np.exp(x @ H.T + c)).astype(np.float64)
    return PoissonLinearModel(y, H, c, m0, P0, F, Q, b, order=order), x, H, c


def logistic_lin_setup(T, dx, dy, family="binomial", seed=0, order=1):
    """Binomial or negative-binomial channels through a loading matrix: poisson_lin_setup's latent (the same F, m0 = b = 0, Q = 0.04 I, P0 = 0.2 I) and loading
    matrix H = N(0, 1) / sqrt(dx) with entries of magnitude below 0.1 set to 0.1; the offsets are log-odds, c ~ U(-1, 1).  family "binomial": trials per channel
    drawn from 1 .. 40, channel 0 binary (trials = 1), y ~ Binomial(trials, sigma(eta)); "negbinomial": r = 3, y ~ NB(3, p = sigma(eta)) (mean 3 e^eta), drawn
    as a Gamma-Poisson mixture.
    Returns (model, x0, H, c, par): a kalman.BinomialLinearModel or kalman.NegBinomialLinearModel, a start state (T, dx) -- the simulated latent path --, the
    loading matrix, the offsets and the family's parameter -- the trials (dy,), or r = 3.0."""
    from aux_ssm_samplers_amd.kalman import BinomialLinearModel, NegBinomialLinearModel
    if family not in ("binomial", "negbinomial"):
        raise ValueError(f"family must be 'binomial' or 'negbinomial', got {family!r}")
    rng = np.random.Generator(np.random.PCG64(seed))
    F = 0.9 * np.eye(dx) + 0.05 * np.eye(dx, k=1) - 0.05 * np.eye(dx, k=-1)
    m0, b = np.zeros(dx), np.zeros(dx)
    Q, P0 = 0.04 * np.eye(dx), 0.2 * np.eye(dx)
    H = rng.standard_normal((dy, dx)) / np.sqrt(dx)
    H = np.where(np.abs(H) < 0.1, 0.1, H)
    c = 2.0 * rng.random(dy) - 1.0
    x = np.zeros((T, dx))
    x[0] = np.sqrt(0.2) * rng.standard_normal(dx)
    for t in range(1, T):
        x[t] = F @ x[t - 1] + 0.2 * rng.standard_normal(dx)
    eta = x @ H.T + c
    if family == "binomial":
        par = rng.integers(1, 41, size=dy).astype(np.float64)
        par[0] = 1.0
        y = rng.binomial(np.broadcast_to(par, eta.shape).astype(np.int64), 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
        return BinomialLinearModel(y, par, H, c, m0, P0, F, Q, b, order=order), x, H, c, par
    y = rng.poisson(rng.gamma(3.0, np.exp(eta))).astype(np.float64)
    return NegBinomialLinearModel(y, 3.0, H, c, m0, P0, F, Q, b, order=order), x, H, c, 3.0


def lorenz_kalman_setup(T, every=8, dt=0.01, seed=0):
    """examples/lorenz: theta = (10, 28, 8/3), sigma_x = 3, m0 = (1.5, -1.5, 25), P0 = diag(400, 20, 20), (x2, x3) observed every `every`-th
    step with variance 5, NaN rows (ys AND Hs, as model.py:43-56) elsewhere."""
    from aux_ssm_samplers_amd.kalman import LorenzModel
    rng = np.random.default_rng(seed)
    theta, sx = np.array([10.0, 28.0, 8.0 / 3.0]), 3.0
    m0, P0 = np.array([1.5, -1.5, 25.0]), np.diag([400.0, 20.0, 20.0])
    H = np.array([[0, 1.0, 0], [0, 0, 1.0]])
    ys = np.full((T, 2), np.nan)
    Hs = np.full((T, 2, 3), np.nan)
    Hs[::every] = H
    Rs = np.broadcast_to(5.0 * np.eye(2), (T, 2, 2))
    cs = np.zeros((T, 2))
    model = LorenzModel(ys, Hs, Rs, cs, m0, P0, theta, sx, dt)
    x = np.zeros((T, 3))
    x[0] = m0
    for t in range(1, T):
        x[t] = model.mean(x[t - 1]) + sx * np.sqrt(dt) * rng.standard_normal(3)
    ys[::every] = x[::every] @ H.T + np.sqrt(5.0) * rng.standard_normal((len(x[::every]), 2))
    model.yobs = ys
    return model, x


def lorenz_setup(T, seed=0, every=8, dt=0.01, sig_y=np.sqrt(5.0)):
    """examples/lorenz (experiment.py:75-83, model.py:10-56) on a short horizon: theta = (10, 28, 8/3), sigma_x = 3,
    m0 = (1.5, -1.5, 25), P0 = diag(400, 20, 20), x2 and x3 observed every `every`-th step with sd sig_y, NaN elsewhere."""
    from aux_ssm_samplers_amd.csmc import GaussianInit, Lorenz63Dynamics, MaskedGaussianObsPotential
    rng = np.random.default_rng(seed)
    Mt = Lorenz63Dynamics(theta=(10.0, 28.0, 8.0 / 3.0), sigma_x=3.0, dt=dt)
    M0 = GaussianInit(m0=np.array([1.5, -1.5, 25.0]), P0=np.diag([400.0, 20.0, 20.0]))
    x = np.zeros((T, 3))
    x[0] = [1.5, -1.5, 25.0]
    for t in range(1, T):
        x[t] = Mt.mean(x[t - 1]) + 3.0 * np.sqrt(dt) * rng.standard_normal(3)
    y = np.full((T, 3), np.nan)
    y[::every, 1:] = x[::every, 1:] + sig_y * rng.standard_normal((len(x[::every]), 2))
    G0 = MaskedGaussianObsPotential(sig=sig_y, y=y[0])
    Gt = MaskedGaussianObsPotential(sig=sig_y, params=y[1:])
    return M0, Mt, G0, Gt, x, y, sig_y


def c5_model(T, d=64, delta=0.1, seed=0):
    """F = 0.9 I + 0.04 tridiag(1, 0, 1) on the 8 x 8 grid's flattened index, Q = I, first-order
    auxiliary observations H = I, R = delta/2 I (p = d)."""
    F = 0.9 * np.eye(d) + 0.04 * (np.eye(d, k=1) + np.eye(d, k=-1))
    rng = np.random.default_rng(seed)
    x = np.zeros((T, d))
    x[0] = rng.standard_normal(d)
    for t in range(1, T):
        x[t] = F @ x[t - 1] + rng.standard_normal(d)
    u = x + np.sqrt(delta / 2) * rng.standard_normal((T, d))
    bt = np.broadcast_to
    lg = (np.zeros(d), np.eye(d), bt(F, (T - 1, d, d)), bt(np.eye(d), (T - 1, d, d)), bt(np.zeros(d), (T - 1, d)),
          bt(np.eye(d), (T, d, d)), bt(delta / 2 * np.eye(d), (T, d, d)), bt(np.zeros(d), (T, d)))
    return u, lg, x


def c5_batched_model(T, B=64, delta=0.1, seed=0):
    """SURVEY 8(d) config C5 in the form the reference's spatial example actually runs (examples/spatial/model.py:103-112, auxiliary_kalman.py:18-28): the
    d^2 = 64 grid cells as B = 64 INDEPENDENT scalar LGSSMs on the batch axis (dx = dy = 1) -- x_t = 0.9 x_{t-1} + N(0, 1) per cell, first-order auxiliary
    observations H = 1, R = delta/2.  Returns (u (T, B, 1), lgssm with a batch axis, x (T, B, 1))."""
    rng = np.random.default_rng(seed)
    x = np.zeros((T, B, 1))
    x[0] = rng.standard_normal((B, 1))
    for t in range(1, T):
        x[t] = 0.9 * x[t - 1] + rng.standard_normal((B, 1))
    u = x + np.sqrt(delta / 2) * rng.standard_normal((T, B, 1))
    bt = np.broadcast_to
    lg = (np.zeros((B, 1)), bt(np.eye(1), (B, 1, 1)), bt(0.9 * np.eye(1), (T - 1, B, 1, 1)), bt(np.eye(1), (T - 1, B, 1, 1)), bt(np.zeros(1), (T - 1, B, 1)),
          bt(np.eye(1), (T, B, 1, 1)), bt(delta / 2 * np.eye(1), (T, B, 1, 1)), bt(np.zeros(1), (T, B, 1)))
    return u, lg, x
