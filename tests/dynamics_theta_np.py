"""TEST INFRASTRUCTURE ONLY: a literal NumPy restatement of the conjugate step on linear-Gaussian dynamics (csrc/dynamics_theta.h / .hip, include/auxssm.h):
the sufficient statistics, the matrix-normal inverse-Wishart posterior, the draw, and the Marsaglia-Tsang gamma generator on the package's Threefry streams
(oracle/rng_np.py, imported read-only).  Written from the formulas, not from the kernels: library linear algebra (solve, inv, cholesky) where the kernels run
their own substitutions, libm log / exp where they run det_math.h's.

    z_t = [x_t; 1],  A = [F b] (d, d + 1);   Q ~ IW(nu0, Psi0),  A | Q ~ MN(M0, Q, K0^-1)
    S_zz = sum z_t z_t^T,  S_xz = sum x_{t+1} z_t^T,  S_xx = sum x_{t+1} x_{t+1}^T            (t = 0 .. T - 2)
    K_n = K0 + S_zz,  M_n = (M0 K0 + S_xz) K_n^-1,  nu_n = nu0 + T - 1,  Psi_n = sym(Psi0 + S_xx + M0 K0 M0^T - M_n K_n M_n^T)
    L = chol(Psi_n), U = chol(K_n), B lower, B_ii = sqrt(chi_i), chi_i ~ chi^2(nu_n - i), B_ij ~ N(0, 1) (i > j)
    Q = sym(L B^-T B^-1 L^T),  A = M_n + chol(Q) E U^-1
"""
import numpy as np

from oracle import rng_np

SEGMENT_LEN = 512          # csrc/dynamics_theta.h::dt_segment_len: transitions per segment of the device's statistics pass (a function of T alone)
GAMMA_ATTEMPTS = 16        # DT_GAMMA_ATTEMPTS
PIVOT_TOL = 2.0 ** -46     # DT_PIVOT_TOL


def stats(x):
    """x (..., T, d) -> S_zz (..., n, n), S_xz (..., d, n), S_xx (..., d, d) in float64"""
    x = np.asarray(x, np.float64)
    z = np.concatenate([x[..., :-1, :], np.ones(x.shape[:-2] + (x.shape[-2] - 1, 1))], axis=-1)
    xn = x[..., 1:, :]
    return np.einsum("...ti,...tj->...ij", z, z), np.einsum("...ti,...tj->...ij", xn, z), np.einsum("...ti,...tj->...ij", xn, xn)


def stats_flat(x):
    """the layout of auxssm_dynamics_stats: (..., n n + d n + d d)"""
    zz, xz, xx = stats(x)
    lead = zz.shape[:-2]
    return np.concatenate([a.reshape(lead + (-1,)) for a in (zz, xz, xx)], axis=-1)


def posterior(S, ntrans, M0, K0, nu0, Psi0):
    """S = (S_zz, S_xz, S_xx) [leading axes allowed] -> M_n, K_n, nu_n, Psi_n"""
    zz, xz, xx = S
    M0, K0, Psi0 = (np.asarray(a, np.float64) for a in (M0, K0, Psi0))
    Kn = K0 + zz
    G = M0 @ K0 + xz
    Mn = np.swapaxes(np.linalg.solve(Kn, np.swapaxes(G, -1, -2)), -1, -2)      # G K_n^-1 (K_n symmetric)
    Psi = Psi0 + xx + M0 @ K0 @ M0.T - Mn @ Kn @ np.swapaxes(Mn, -1, -2)
    return Mn, Kn, nu0 + ntrans, 0.5 * (Psi + np.swapaxes(Psi, -1, -2))


def post_flat(post):
    """the layout of post_out: (..., d n + n n + 1 + d d)"""
    Mn, Kn, nun, Psi = post
    lead = Mn.shape[:-2]
    return np.concatenate([Mn.reshape(lead + (-1,)), Kn.reshape(lead + (-1,)), np.broadcast_to(np.float64(nun), lead + (1,)), Psi.reshape(lead + (-1,))], axis=-1)


def chol_checked(a):
    """lower Cholesky factor of ONE matrix, or None where the device calls the factorisation failed: a pivot that is not finite, not positive, or below
    2^-46 of its diagonal entry"""
    a = np.asarray(a, np.float64)
    n = a.shape[0]
    l = np.zeros((n, n))
    for j in range(n):
        d = a[j, j] - np.dot(l[j, :j], l[j, :j])
        if not np.isfinite(d) or not d > PIVOT_TOL * a[j, j]:
            return None
        l[j, j] = np.sqrt(d)
        for i in range(j + 1, n):
            l[i, j] = (a[i, j] - np.dot(l[i, :j], l[j, :j])) / l[j, j]
    return l


def draw(post, chi, ew, ea):
    """post = (M_n, K_n, nu_n, Psi_n); chi (..., d) chi-square values, ew (..., d, d) (strict lower triangle read), ea (..., d, n) -> Q, A (batched over leading axes)"""
    Mn, Kn, _, Psi = post
    chi, ew, ea = (np.asarray(a, np.float64) for a in (chi, ew, ea))
    d = chi.shape[-1]
    L = np.linalg.cholesky(Psi)
    U = np.linalg.cholesky(Kn)
    B = np.tril(ew, -1)
    i = np.arange(d)
    B[..., i, i] = np.sqrt(chi)
    W = L @ np.swapaxes(np.linalg.inv(B), -1, -2)
    Q = W @ np.swapaxes(W, -1, -2)
    Q = 0.5 * (Q + np.swapaxes(Q, -1, -2))
    A = Mn + np.linalg.cholesky(Q) @ ea @ np.linalg.inv(U)
    return Q, A


def step(x, M0, K0, nu0, Psi0, chi, ew, ea):
    """one chain: x (T, d) -> (flag, post, Q or None, A or None); flag as the device's (0 ok, 1 K_n, 2 Psi_n, 3 chi, 4 Q)"""
    x = np.asarray(x, np.float64)
    S = stats(x)
    Kn = np.asarray(K0, np.float64) + S[0]
    if chol_checked(Kn) is None:     # (K_n cannot be solved with: the posterior stops at K_n and nu_n, as the device's does)
        return 1, (None, Kn, nu0 + x.shape[0] - 1, None), None, None
    post = posterior(S, x.shape[0] - 1, M0, K0, nu0, Psi0)
    plus = np.diag(np.asarray(Psi0) + S[2] + np.asarray(M0) @ np.asarray(K0) @ np.asarray(M0).T)
    if not np.all(np.diag(post[3]) > PIVOT_TOL * plus) or chol_checked(post[3]) is None:
        return 2, post, None, None
    if not np.all((np.asarray(chi) > 0) & np.isfinite(chi)):
        return 3, post, None, None
    Q, A = draw(post, chi, ew, ea)
    if chol_checked(Q) is None or not (np.all(np.isfinite(Q)) and np.all(np.isfinite(A))):
        return 4, post, None, None
    return 0, post, Q, A


# ---- Gamma(shape, 1): Marsaglia & Tsang (2000) on the Threefry streams ------------------------------------------------------------------
def _blocks(key, stream, blk):
    blk = np.asarray(blk, np.uint64)
    x0 = (blk & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    x1 = (np.uint64(stream) ^ ((blk >> np.uint64(32)) << np.uint64(16))).astype(np.uint32)
    return rng_np.threefry2x32(key[0], key[1], x0, x1)


def gamma_variates(key, stream, g, k):
    """attempt k of draws g (flat indices): x ~ N(0, 1) = the cos branch of the fp64 Box-Muller transform of block 2 (16 g + k) (as rng_np.normal forms it),
    u, u' = (word + 1/2) 2^-32 of the two words of the next block"""
    blk = np.uint64(2) * (np.asarray(g, np.uint64) * np.uint64(GAMMA_ATTEMPTS) + np.uint64(k))
    a0, a1 = _blocks(key, stream, blk)
    u1 = (a0.astype(np.float64) + 0.5) * 2.3283064365386963e-10
    u2 = (a1.astype(np.float64) + 0.5) * 2.3283064365386963e-10
    c, _ = rng_np.sincos_2pi(u2)
    x = np.sqrt(-2.0 * np.log(u1)) * c
    b0, b1 = _blocks(key, stream, blk + np.uint64(1))
    return x, (b0.astype(np.float64) + 0.5) * 2.3283064365386963e-10, (b1.astype(np.float64) + 0.5) * 2.3283064365386963e-10


def gamma(key, stream, n, shapes, with_margin=False):
    """out (n, m), out[j, i] ~ Gamma(shapes[i], 1); draw g = j m + i takes the first accepted of GAMMA_ATTEMPTS attempts, NaN if none.
    with_margin: also the smallest |threshold - log u| over the decisions taken (how far the restatement is from deciding otherwise)."""
    shapes = np.asarray(shapes, np.float64)
    m = shapes.size
    g = np.arange(n * m, dtype=np.uint64)
    a = np.tile(shapes, n)
    boost = a < 1.0
    a1 = np.where(boost, a + 1.0, a)
    d = a1 - 1.0 / 3.0
    c = 1.0 / np.sqrt(9.0 * d)
    out = np.full(n * m, np.nan)
    todo = np.ones(n * m, bool)
    margin = np.inf
    for k in range(GAMMA_ATTEMPTS):
        idx = np.nonzero(todo)[0]
        if idx.size == 0:
            break
        x, u, ub = gamma_variates(key, stream, g[idx], k)
        t = 1.0 + c[idx] * x
        v = t * t * t
        pos = v > 0.0
        with np.errstate(all="ignore"):
            thr = ((0.5 * x * x + d[idx]) - d[idx] * v) + d[idx] * np.log(np.where(pos, v, 1.0))
            diff = thr - np.log(u)
        if np.any(pos):
            margin = min(margin, float(np.min(np.abs(diff[pos]))))
        acc = pos & (diff > 0.0)
        val = d[idx] * v
        bi = boost[idx]
        val = np.where(bi, val * np.exp(np.log(ub) / np.where(bi, a[idx], 1.0)), val)
        out[idx[acc]] = val[acc]
        todo[idx[acc]] = False
    out = out.reshape(n, m)
    return (out, margin) if with_margin else out
