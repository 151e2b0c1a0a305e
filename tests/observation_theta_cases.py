"""TEST INFRASTRUCTURE ONLY: the problems the tests of the conjugate observation step share (tests/test_observation_theta_host.py on the CPU,
tests/test_gpu_observation_theta.py on the device)."""
import numpy as np


def problem(dx, dy, T, seed, missing=(), C=None):
    """states around a stable VAR(1), data y = H x + c + noise with the rows `missing` wholly NaN, and a proper prior.  C: that many chains (C, T, dx) scattered
    around the one trajectory the data came from"""
    rng = np.random.default_rng(seed)
    n = dx + 1
    F = 0.6 * np.eye(dx) + 0.1 * rng.standard_normal((dx, dx))
    x = np.zeros((T, dx))
    x[0] = rng.standard_normal(dx)
    for t in range(T - 1):
        x[t + 1] = F @ x[t] + 0.3 + 0.6 * rng.standard_normal(dx)
    H = rng.standard_normal((dy, dx))
    c = 0.5 * rng.standard_normal(dy)
    Lr = np.tril(0.2 * rng.standard_normal((dy, dy))) + 0.5 * np.eye(dy)
    y = x @ H.T + c + rng.standard_normal((T, dy)) @ Lr.T
    for t in missing:
        y[t] = np.nan
    M0 = np.concatenate([H, c[:, None]], axis=1) + 0.1 * rng.standard_normal((dy, n))
    a = rng.standard_normal((n, n))
    K0 = 0.5 * np.eye(n) + 0.1 * a @ a.T
    g = rng.standard_normal((dy, dy))
    Psi0 = np.eye(dy) + 0.2 * g @ g.T
    nu0 = dy + 2.5
    xs = x if C is None else x[None] + 0.3 * rng.standard_normal((C, T, dx))
    return dict(x=xs, y=y, H=H, c=c, R=Lr @ Lr.T, M0=M0, K0=K0, nu0=nu0, Psi0=Psi0)


def noise(dx, dy, seed, nu, lead=()):
    """chi (.., dy) chi-square draws of nu - i degrees, ew (.., dy, dy), ea (.., dy, dx + 1)"""
    rng = np.random.default_rng(seed)
    chi = np.stack([rng.chisquare(nu - i, lead) for i in range(dy)], axis=-1)
    return chi, rng.standard_normal(lead + (dy, dy)), rng.standard_normal(lead + (dy, dx + 1))


def exact_fit(dx, dy, T):
    """data that an affine map of the state reproduces EXACTLY in floating point (small integers), a prior mean equal to that map and a vanishing Psi0: Psi_n is
    rounding noise of the sums it is the difference of (flag 2 in both modes).  For dy <= dx: the data then lies in c + span(H), all of R^dy, and a chain
    with ANOTHER state keeps a full-rank residual scatter (with dy > dx every chain's Psi_n would be singular: the intercept absorbs c and the residuals stay in
    span(H)).  -> x (T, dx), y (T, dy), A = [H c], Psi0"""
    rng = np.random.default_rng(5)
    x = rng.integers(-8, 9, (T, dx)).astype(np.float64)
    H = rng.integers(-3, 4, (dy, dx)).astype(np.float64)
    c = np.arange(1, dy + 1, dtype=np.float64)
    y = x @ H.T + c
    return x, y, np.concatenate([H, c[:, None]], axis=1), 1e-200 * np.eye(dy)


def rel(got, want):
    """largest difference relative to the reference's largest entry"""
    want = np.asarray(want, np.float64)
    return float(np.max(np.abs(np.asarray(got, np.float64) - want)) / np.max(np.abs(want)))


def split_post(post, dx, dy):
    """post_out row(s) (..., dy n + n n + 1 + dy dy) -> M_n, K_n, nu_n, Psi_n"""
    n = dx + 1
    post = np.asarray(post)
    lead = post.shape[:-1]
    o = [0, dy * n, dy * n + n * n, dy * n + n * n + 1, dy * n + n * n + 1 + dy * dy]
    return (post[..., o[0]:o[1]].reshape(lead + (dy, n)), post[..., o[1]:o[2]].reshape(lead + (n, n)), post[..., o[2]], post[..., o[3]:o[4]].reshape(lead + (dy, dy)))
