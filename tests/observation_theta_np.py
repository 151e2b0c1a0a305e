"""TEST INFRASTRUCTURE ONLY: a literal NumPy restatement of the conjugate step on the linear-Gaussian observation model y_t = H x_t + c + N(0, R)
(csrc/observation_theta.h / .hip, include/auxssm.h): the sufficient statistics, both posteriors and the draw from explicit noise.  Written from the formulas,
not from the kernels: library linear algebra (solve, inv, cholesky) where the kernels run their own substitutions.

    z_t = [x_t; 1],  A = [H c] (dy, dx + 1);   R ~ IW(nu0, Psi0),  A | R ~ MN(M0, R, K0^-1);   sums over the steps whose row of y is entirely finite
    So_zz = sum z_t z_t^T,  S_yz = sum y_t z_t^T,  S_yy = sum y_t y_t^T,  n_obs
    joint    K_n = K0 + So_zz,  M_n = (M0 K0 + S_yz) K_n^-1,  nu_n = nu0 + n_obs,  Psi_n = sym(Psi0 + S_yy + M0 K0 M0^T - M_n K_n M_n^T)
    R alone  nu_n = nu0 + n_obs,  Psi_n = sym(Psi0 + S_yy - A S_yz^T - S_yz A^T + A So_zz A^T)
    L = chol(Psi_n), U = chol(K_n), B lower, B_ii = sqrt(chi_i), chi_i ~ chi^2(nu_n - i), B_ij ~ N(0, 1) (i > j)
    R = sym(L B^-T B^-1 L^T),  A = M_n + chol(R) E U^-1
"""
import numpy as np

from tests.dynamics_theta_np import PIVOT_TOL, SEGMENT_LEN, chol_checked  # noqa: F401  (the device's factorisation rule and segment length are the dynamics step's)

JOINT, R_ALONE = 1, 2


def observed(y):
    """y (T, dy) -> (T,) bool: the rows that are entirely finite"""
    return np.all(np.isfinite(np.asarray(y, np.float64)), axis=-1)


def stats(x, y):
    """x (..., T, dx), y (T, dy) -> So_zz (..., n, n), S_yz (..., dy, n) in float64, over the observed rows of y"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    m = observed(y)
    z = np.concatenate([x[..., m, :], np.ones(x.shape[:-2] + (int(m.sum()), 1))], axis=-1)
    return np.einsum("...ti,...tj->...ij", z, z), np.einsum("ti,...tj->...ij", y[m], z)


def stats_flat(x, y):
    """the layout of auxssm_observation_stats: (..., n n + dy n)"""
    zz, yz = stats(x, y)
    lead = zz.shape[:-2]
    return np.concatenate([zz.reshape(lead + (-1,)), yz.reshape(lead + (-1,))], axis=-1)


def data_terms(y):
    """y (T, dy) -> (S_yy (dy, dy), n_obs); syy_nobs of the C ABI is their concatenation"""
    y = np.asarray(y, np.float64)
    yo = y[observed(y)]
    return yo.T @ yo, yo.shape[0]


def syy_nobs(y):
    syy, n = data_terms(y)
    return np.concatenate([syy.ravel(), [float(n)]])


def posterior_joint(S, syy, nobs, M0, K0, nu0, Psi0):
    """S = (So_zz, S_yz) [leading axes allowed] -> M_n, K_n, nu_n, Psi_n"""
    zz, yz = S
    M0, K0, Psi0 = (np.asarray(a, np.float64) for a in (M0, K0, Psi0))
    Kn = K0 + zz
    G = M0 @ K0 + yz
    Mn = np.swapaxes(np.linalg.solve(Kn, np.swapaxes(G, -1, -2)), -1, -2)      # G K_n^-1 (K_n symmetric)
    Psi = Psi0 + syy + M0 @ K0 @ M0.T - Mn @ Kn @ np.swapaxes(Mn, -1, -2)
    return Mn, Kn, nu0 + nobs, 0.5 * (Psi + np.swapaxes(Psi, -1, -2))


def posterior_r(S, syy, nobs, nu0, Psi0, A):
    """R alone, A = [H c] (..., dy, n) fixed -> A, So_zz, nu_n, Psi_n (the layout of post_out in that mode)"""
    zz, yz = S
    A = np.asarray(A, np.float64)
    At = np.swapaxes(A, -1, -2)
    Psi = np.asarray(Psi0, np.float64) + syy - A @ np.swapaxes(yz, -1, -2) - yz @ At + A @ zz @ At
    return A, zz, nu0 + nobs, 0.5 * (Psi + np.swapaxes(Psi, -1, -2))


def post_flat(post):
    """the layout of post_out: (..., dy n + n n + 1 + dy dy)"""
    Mn, Kn, nun, Psi = post
    lead = Mn.shape[:-2]
    return np.concatenate([Mn.reshape(lead + (-1,)), Kn.reshape(lead + (-1,)), np.broadcast_to(np.float64(nun), lead + (1,)), Psi.reshape(lead + (-1,))], axis=-1)


def draw_r(Psi, chi, ew):
    """Psi (..., dy, dy), chi (..., dy) chi-square values, ew (..., dy, dy) (strict lower triangle read) -> R"""
    chi, ew = np.asarray(chi, np.float64), np.asarray(ew, np.float64)
    dy = chi.shape[-1]
    L = np.linalg.cholesky(Psi)
    B = np.tril(ew, -1)
    i = np.arange(dy)
    B[..., i, i] = np.sqrt(chi)
    W = L @ np.swapaxes(np.linalg.inv(B), -1, -2)
    R = W @ np.swapaxes(W, -1, -2)
    return 0.5 * (R + np.swapaxes(R, -1, -2))


def draw(post, chi, ew, ea):
    """joint mode: post = (M_n, K_n, nu_n, Psi_n); ea (..., dy, n) -> R, A (batched over leading axes)"""
    Mn, Kn, _, Psi = post
    R = draw_r(Psi, chi, ew)
    U = np.linalg.cholesky(Kn)
    A = Mn + np.linalg.cholesky(R) @ np.asarray(ea, np.float64) @ np.linalg.inv(U)
    return R, A


def step(x, y, M0, K0, nu0, Psi0, chi, ew, ea, mode=JOINT, A0=None):
    """one chain: x (T, dx), y (T, dy) -> (flag, post, R or None, A or None); flag as the device's (0 ok, 1 K_n or no observed row, 2 Psi_n, 3 chi, 4 R).
    mode R_ALONE: A0 = the chain's present [H c]; A is returned as None (H, c keep their bits)"""
    x = np.asarray(x, np.float64)
    S = stats(x, y)
    syy, nobs = data_terms(y)
    Psi0 = np.asarray(Psi0, np.float64)
    if mode == JOINT:
        M0, K0 = np.asarray(M0, np.float64), np.asarray(K0, np.float64)
        Kn = K0 + S[0]
        if nobs == 0 or chol_checked(Kn) is None:     # (the posterior stops at K_n and nu_n, as the device's does)
            return 1, (None, Kn, nu0 + nobs, None), None, None
        post = posterior_joint(S, syy, nobs, M0, K0, nu0, Psi0)
        plus = np.diag(Psi0 + syy + M0 @ K0 @ M0.T)
    else:
        A0 = np.asarray(A0, np.float64)
        if nobs == 0:
            return 1, (A0, S[0], nu0 + nobs, None), None, None
        post = posterior_r(S, syy, nobs, nu0, Psi0, A0)
        plus = np.diag(Psi0 + syy + A0 @ S[0] @ A0.T)
    if not np.all(np.diag(post[3]) > PIVOT_TOL * plus) or chol_checked(post[3]) is None:
        return 2, post, None, None
    if not np.all((np.asarray(chi) > 0) & np.isfinite(chi)):
        return 3, post, None, None
    if mode == JOINT:
        R, A = draw(post, chi, ew, ea)
    else:
        R, A = draw_r(post[3], chi, ew), None
    if chol_checked(R) is None or not np.all(np.isfinite(R)) or (A is not None and not np.all(np.isfinite(A))):
        return 4, post, None, None
    return 0, post, R, A
