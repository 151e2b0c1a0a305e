"""TEST INFRASTRUCTURE ONLY: a literal NumPy restatement of EM for a time-invariant linear-Gaussian state-space model
    x_0 ~ N(m0, P0),  x_{t+1} = F x_t + b + N(0, Q),  y_t = H x_t + c + N(0, R)
as csrc/lgssm_em.h / lgssm_em.hip run it: Kalman filter, Rauch-Tung-Striebel smoother, lag-one smoothing covariances, expected sufficient statistics, the three
M-step blocks with their failure rule, and the EM loop.  Formulas as written in include/auxssm.h, one time step after the other, solves by np.linalg.solve.
A parameter set is a dict with the keys m0, P0, F, b, Q, H, c, R.  Rows of y that are entirely NaN are missing steps."""
import numpy as np

PIVOT_TOL = 2.0 ** -46
SEGMENT_LEN = 512   # dynamics_theta.h::dt_segment_len
NAMES = ("F", "b", "Q", "H", "c", "R", "m0", "P0")
BLOCKS = {"dynamics": ("F", "b", "Q"), "observations": ("H", "c", "R"), "initial": ("m0", "P0")}


def sym(a):
    return 0.5 * (a + a.T)


def chol_ok(a):
    """the failure rule: a pivot that is not finite, not positive, or below 2^-46 of its diagonal entry"""
    a = np.asarray(a, np.float64)
    N = a.shape[0]
    l = np.zeros((N, N))
    for j in range(N):
        d = a[j, j] - np.dot(l[j, :j], l[j, :j])
        if not (d > PIVOT_TOL * a[j, j]) or not np.isfinite(d):
            return False
        l[j, j] = np.sqrt(d)
        for i in range(j + 1, N):
            l[i, j] = (a[i, j] - np.dot(l[i, :j], l[j, :j])) / l[j, j]
    return True


# ---- E-step ------------------------------------------------------------------------------------------------------------------------------------------------------

def kalman_filter(ys, p):
    """-> ms (T, dx), Ps (T, dx, dx), ell; a NaN entry of y_t is a missing component (a row of NaNs: no update)"""
    T, dx = ys.shape[0], p["m0"].shape[0]
    ms, Ps, ell = np.zeros((T, dx)), np.zeros((T, dx, dx)), 0.0
    m, P = p["m0"], p["P0"]
    for t in range(T):
        if t > 0:
            m, P = p["F"] @ m + p["b"], sym(p["F"] @ P @ p["F"].T + p["Q"])
        o = np.isfinite(ys[t])
        if o.any():
            H, c, R = p["H"][o], p["c"][o], p["R"][np.ix_(o, o)]
            r = ys[t][o] - (H @ m + c)
            S = sym(H @ P @ H.T + R)
            K = np.linalg.solve(S, H @ P).T
            ell += -0.5 * (r @ np.linalg.solve(S, r) + np.linalg.slogdet(S)[1] + o.sum() * np.log(2.0 * np.pi))
            m, P = m + K @ r, sym(P - K @ S @ K.T)
        ms[t], Ps[t] = m, P
    return ms, Ps, ell


def rts(ms, Ps, p):
    """-> sms, sPs: sms[t] = m_t + G_t (sms[t+1] - F m_t - b), sPs[t] = G_t sPs[t+1] G_t^T + sym(P_t - G_t S_t G_t^T)"""
    T = ms.shape[0]
    sms, sPs = ms.copy(), Ps.copy()
    for t in range(T - 2, -1, -1):
        S = sym(p["F"] @ Ps[t] @ p["F"].T + p["Q"])
        G = np.linalg.solve(S, p["F"] @ Ps[t]).T
        sms[t] = ms[t] + G @ (sms[t + 1] - p["F"] @ ms[t] - p["b"])
        sPs[t] = sym(G @ sPs[t + 1] @ G.T + sym(Ps[t] - G @ S @ G.T))
    return sms, sPs


def lag_one(Ps, sPs, p):
    """X_t = Cov[x_{t+1}, x_t | y] = sPs[t+1] G_t^T, t = 0 .. T-2"""
    T, dx = Ps.shape[0], Ps.shape[1]
    X = np.zeros((T - 1, dx, dx))
    for t in range(T - 1):
        S = sym(p["F"] @ Ps[t] @ p["F"].T + p["Q"])
        G = np.linalg.solve(S, p["F"] @ Ps[t]).T
        X[t] = sPs[t + 1] @ G.T
    return X


def observed_rows(ys):
    return np.all(np.isfinite(ys), axis=-1)


def statistics(ys, sms, sPs, X, reverse=False):
    """the expected sufficient statistics of one sequence, summed step by step (reverse: in descending time) -> dict of blocks"""
    T, dx = sms.shape
    dy, n = ys.shape[1], dx + 1
    st = dict(S_zz=np.zeros((n, n)), S_xz=np.zeros((dx, n)), S_xx=np.zeros((dx, dx)), So_zz=np.zeros((n, n)), S_yz=np.zeros((dy, n)))

    def Ezz(t):
        e = np.zeros((n, n))
        e[:dx, :dx] = sPs[t] + np.outer(sms[t], sms[t])
        e[:dx, dx] = e[dx, :dx] = sms[t]
        e[dx, dx] = 1.0
        return e

    steps = range(T - 2, -1, -1) if reverse else range(T - 1)
    for t in steps:
        st["S_zz"] += Ezz(t)
        st["S_xz"][:, :dx] += X[t] + np.outer(sms[t + 1], sms[t])
        st["S_xz"][:, dx] += sms[t + 1]
        st["S_xx"] += sPs[t + 1] + np.outer(sms[t + 1], sms[t + 1])
    seen = observed_rows(ys)
    for t in (range(T - 1, -1, -1) if reverse else range(T)):
        if seen[t]:
            st["So_zz"] += Ezz(t)
            st["S_yz"] += np.outer(ys[t], np.append(sms[t], 1.0))
    st["sm0"], st["sP0"] = sms[0].copy(), sPs[0].copy()
    return st


STAT_BLOCKS = ("S_zz", "S_xz", "S_xx", "So_zz", "S_yz", "sm0", "sP0")   # the order of stats_out's FULL layout


def flat(st):
    return np.concatenate([np.ravel(st[k]) for k in STAT_BLOCKS])


def split(vec, dx, dy):
    """a FULL statistics vector -> dict of blocks"""
    n = dx + 1
    shapes = dict(S_zz=(n, n), S_xz=(dx, n), S_xx=(dx, dx), So_zz=(n, n), S_yz=(dy, n), sm0=(dx,), sP0=(dx, dx))
    out, o = {}, 0
    for k in STAT_BLOCKS:
        m = int(np.prod(shapes[k]))
        out[k] = np.asarray(vec[o:o + m]).reshape(shapes[k])
        o += m
    assert o == len(vec)
    return out


def e_step(ys, p, reverse=False):
    ms, Ps, ell = kalman_filter(ys, p)
    sms, sPs = rts(ms, Ps, p)
    X = lag_one(Ps, sPs, p)
    return statistics(ys, sms, sPs, X, reverse), ell, (ms, Ps, sms, sPs, X)


def syy_nobs(ys_list):
    """S_yy = sum y_t y_t^T over the observed steps of all sequences, and their number"""
    dy = ys_list[0].shape[1]
    Syy, nobs = np.zeros((dy, dy)), 0
    for ys in ys_list:
        for t in np.nonzero(observed_rows(ys))[0]:
            Syy += np.outer(ys[t], ys[t])
            nobs += 1
    return Syy, nobs


# ---- M-step: each block -> (flag, new values or None) ----------------------------------------------------------------------------------------------------------

def _regress(Saa, Sab, Sbb, cnt):
    if not cnt >= 1 or not chol_ok(Saa):
        return 1, None
    coef = np.linalg.solve(Saa, Sab.T).T
    res = sym(Sbb - coef @ Sab.T) / cnt
    if not chol_ok(res):
        return 2, None
    if not (np.all(np.isfinite(coef)) and np.all(np.isfinite(res))):
        return 3, None
    return 0, (coef, res)


def mstep_dynamics(S_zz, S_xz, S_xx, prior=None):
    """maximum likelihood: [F b] = S_xz S_zz^-1, Q = sym(S_xx - [F b] S_xz^T) / N_tr;  prior (M0, K0, nu0, Psi0): the joint mode of the MNIW posterior"""
    dx = S_xx.shape[0]
    n, ntr = dx + 1, S_zz[-1, -1]
    if prior is None:
        flag, out = _regress(S_zz, S_xz, S_xx, ntr)
        return (flag, None) if flag else (0, (out[0][:, :dx], out[0][:, dx], out[1]))
    M0, K0, nu0, Psi0 = prior
    Kn = K0 + S_zz
    if not chol_ok(Kn):
        return 1, None
    Mn = np.linalg.solve(Kn, (M0 @ K0 + S_xz).T).T
    Psi = sym(Psi0 + S_xx + M0 @ K0 @ M0.T - Mn @ Kn @ Mn.T)
    if not chol_ok(Psi):
        return 2, None
    Q = Psi / (nu0 + ntr + dx + n + 1)
    return 0, (Mn[:, :dx], Mn[:, dx], Q)


def mstep_observations(So_zz, S_yz, Syy, nobs):
    dx = So_zz.shape[0] - 1
    flag, out = _regress(So_zz, S_yz, Syy, nobs)
    return (flag, None) if flag else (0, (out[0][:, :dx], out[0][:, dx], out[1]))


def mstep_initial(sm0s, sP0s):
    m0 = np.mean(sm0s, axis=0)
    P0 = sym(np.mean([sP + np.outer(sm - m0, sm - m0) for sm, sP in zip(sm0s, sP0s)], axis=0))
    return (0, (m0, P0)) if chol_ok(P0) else (2, None)


def em(ys_list, p, n_iter, update=NAMES, prior=None, reverse=False):
    """-> (iterates [n_iter + 1 parameter dicts, the start first], ells (n_iter + 1,), flags (n_iter, 4)); ells[k]: at the parameters before M-step k"""
    p = {k: np.array(v, np.float64) for k, v in p.items()}
    Syy, nobs = syy_nobs(ys_list)
    iterates, ells, flags = [dict(p)], [], np.zeros((n_iter, 4), np.int32)
    for it in range(n_iter):
        sts, ell = [], 0.0
        for ys in ys_list:
            st, e, _ = e_step(ys, p, reverse)
            sts.append(st)
            ell += e
        ells.append(ell)
        tot = {k: sum(st[k] for st in sts) for k in ("S_zz", "S_xz", "S_xx", "So_zz", "S_yz")}
        new = dict(p)
        if "F" in update:
            flags[it, 0], out = mstep_dynamics(tot["S_zz"], tot["S_xz"], tot["S_xx"], prior)
            if out is not None:
                new["F"], new["b"], new["Q"] = out
        if "H" in update:
            flags[it, 1], out = mstep_observations(tot["So_zz"], tot["S_yz"], Syy, nobs)
            if out is not None:
                new["H"], new["c"], new["R"] = out
        if "m0" in update:
            flags[it, 2], out = mstep_initial([st["sm0"] for st in sts], [st["sP0"] for st in sts])
            if out is not None:
                new["m0"], new["P0"] = out
        p = new
        iterates.append(dict(p))
    ells.append(sum(kalman_filter(ys, p)[2] for ys in ys_list))
    return iterates, np.array(ells), flags


# ---- problems the CPU and GPU tests share -----------------------------------------------------------------------------------------------------------------------

def random_model(rng, dx, dy):
    """a stable, well-conditioned parameter set"""
    F = 0.7 * np.eye(dx) + 0.15 * rng.standard_normal((dx, dx)) / np.sqrt(dx)
    F *= min(1.0, 0.85 / np.max(np.abs(np.linalg.eigvals(F))))   # spectral radius <= 0.85: the states stay O(1) and no statistic cancels
    A = rng.standard_normal((dx, dx))
    Q = 0.3 * np.eye(dx) + 0.05 * A @ A.T
    B = rng.standard_normal((dy, dy))
    R = 0.4 * np.eye(dy) + 0.05 * B @ B.T
    return dict(m0=0.3 * rng.standard_normal(dx), P0=np.eye(dx) * 0.8, F=F, b=0.1 * rng.standard_normal(dx), Q=Q,
                H=rng.standard_normal((dy, dx)) / np.sqrt(dx), c=0.2 * rng.standard_normal(dy), R=R)


def simulate(rng, p, T, missing=()):
    dx, dy = p["m0"].shape[0], p["c"].shape[0]
    x = np.zeros((T, dx))
    x[0] = p["m0"] + np.linalg.cholesky(p["P0"]) @ rng.standard_normal(dx)
    LQ, LR = np.linalg.cholesky(p["Q"]), np.linalg.cholesky(p["R"])
    for t in range(1, T):
        x[t] = p["F"] @ x[t - 1] + p["b"] + LQ @ rng.standard_normal(dx)
    ys = x @ p["H"].T + p["c"] + rng.standard_normal((T, dy)) @ LR.T
    for t in missing:
        ys[t] = np.nan
    return x, ys


def perturbed(rng, p, scale=0.2):
    """a start for EM: the parameters moved, covariances kept positive definite"""
    q = {k: np.array(v, np.float64) for k, v in p.items()}
    for k in ("F", "b", "H", "c", "m0"):
        q[k] = q[k] + scale * rng.standard_normal(q[k].shape) * 0.5
    for k in ("Q", "R", "P0"):
        q[k] = q[k] * (1.0 + scale)
    return q


EM_SEED = 7   # the seed of em_problem(): chosen so that the restatement alone passes its monotonicity and summation-order checks (test_lgssm_em_host.py)


def em_problem(seed=EM_SEED, T=300, dx=2, dy=3, missing=(40, 171)):
    """the EM test's problem (CPU and GPU): data from a random model, two missing rows, a perturbed start"""
    rng = np.random.default_rng(seed)
    truth = random_model(rng, dx, dy)
    _, ys = simulate(rng, truth, T, missing)
    return ys, perturbed(rng, truth), truth
