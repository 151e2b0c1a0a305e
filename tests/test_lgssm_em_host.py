"""EM for linear-Gaussian state-space models, the CPU half:
  1. the restatement (tests/lgssm_em_np.py) against a dense conditioning of the joint Gaussian of (x_0 .. x_3, y): sm, sP and every lag-one covariance at 1e-10
  2. csrc/lgssm_em.h under g++ (tests/hostsim_lgssm_em) against the restatement at 1e-12 for d = 1..4, dy in {1, 3, 8}: lag-one terms, the statistics of a short
     sequence, the three M-step blocks (maximum likelihood and with a prior), and a singular S_zz, which must raise the flag
  3. the restatement's EM: a log-likelihood that does not decrease, and the same iterates with the sums taken in reversed time order (the conditioning check of
     the GPU comparison)
  4. every refusal of the Python layer raises before a handle is taken; the new symbols are in the built library."""
import numpy as np
import pytest

from aux_ssm_samplers_amd import _lib
from aux_ssm_samplers_amd._primitives import kalman as K
from aux_ssm_samplers_amd.loop import MNIWPrior
from tests import hostsim_lgssm_em as hs
from tests import lgssm_em_np as E

DIMS = [(dx, dy) for dx in (1, 2, 3, 4) for dy in (1, 3, 8)]


def _close(a, b, tol, what=""):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    err = float(np.max(np.abs(a - b))) / max(1.0, float(np.max(np.abs(b))))
    assert err <= tol, f"{what}: {err:.3e} > {tol:.1e}"


def test_restatement_against_dense_conditioning():
    T, dx, dy = 4, 2, 2
    rng = np.random.default_rng(11)
    p = E.random_model(rng, dx, dy)
    _, ys = E.simulate(rng, p, T, missing=(2,))
    # the joint Gaussian of (x_0 .. x_3): mean and covariance by the recursion of the model, block by block
    mu, cov = np.zeros((T, dx)), np.zeros((T, T, dx, dx))
    mu[0], cov[0, 0] = p["m0"], p["P0"]
    for t in range(1, T):
        mu[t] = p["F"] @ mu[t - 1] + p["b"]
        cov[t, t] = p["F"] @ cov[t - 1, t - 1] @ p["F"].T + p["Q"]
    for s in range(T):
        for t in range(s + 1, T):
            cov[t, s] = p["F"] @ cov[t - 1, s]
            cov[s, t] = cov[t, s].T
    Sx = cov.transpose(0, 2, 1, 3).reshape(T * dx, T * dx)
    obs = [t for t in range(T) if np.all(np.isfinite(ys[t]))]
    Hbig = np.zeros((len(obs) * dy, T * dx))
    for k, t in enumerate(obs):
        Hbig[k * dy:(k + 1) * dy, t * dx:(t + 1) * dx] = p["H"]
    Rbig = np.kron(np.eye(len(obs)), p["R"])
    yv = np.concatenate([ys[t] - p["c"] for t in obs])
    Sy = Hbig @ Sx @ Hbig.T + Rbig
    gain = np.linalg.solve(Sy, Hbig @ Sx).T
    post_m = (mu.ravel() + gain @ (yv - Hbig @ mu.ravel())).reshape(T, dx)
    post_S = Sx - gain @ Sy @ gain.T
    _, _, (ms, Ps, sms, sPs, X) = E.e_step(ys, p)
    _close(sms, post_m, 1e-10, "sm")
    for t in range(T):
        _close(sPs[t], post_S[t * dx:(t + 1) * dx, t * dx:(t + 1) * dx], 1e-10, f"sP[{t}]")
    for t in range(T - 1):
        _close(X[t], post_S[(t + 1) * dx:(t + 2) * dx, t * dx:(t + 1) * dx], 1e-10, f"X[{t}]")


@pytest.mark.parametrize("dx,dy", DIMS)
def test_harness_against_restatement(dx, dy):
    rng = np.random.default_rng(100 * dx + dy)
    p = E.random_model(rng, dx, dy)
    T = 40   # enough observed rows for a positive definite R at dy = 8
    _, ys = E.simulate(rng, p, T, missing=(0, 17, T - 1))
    st, _, (ms, Ps, sms, sPs, X) = E.e_step(ys, p)
    assert hs.ns(dx, dy) == E.flat(st).size
    for t in (0, 5, T - 2):
        failed, Xt = hs.lag_one(p["F"], p["Q"], Ps[t], sPs[t + 1])
        assert failed == 0
        _close(Xt, X[t], 1e-12, f"lag one t={t}")
    cross, full = hs.stats(p["F"], p["Q"], ys, Ps, sms, sPs)
    _close(cross, X, 1e-12, "cross")
    got = E.split(full, dx, dy)
    for k in E.STAT_BLOCKS:
        _close(got[k], st[k], 1e-12, k)
    assert np.array_equal(got["S_zz"], got["S_zz"].T) and np.array_equal(got["So_zz"], got["So_zz"].T)
    assert got["S_zz"][-1, -1] == T - 1 and got["So_zz"][-1, -1] == T - 3

    n = dx + 1
    dyn = np.concatenate([got[k].ravel() for k in ("S_zz", "S_xz", "S_xx")])
    prior = (0.5 * rng.standard_normal((dx, n)), np.eye(n) * 2.0, dx + 3.0, np.eye(dx) * 0.7)
    for pr in (None, prior):
        flag, A, Q = hs.mstep_dyn(dx, dyn, pr)
        rflag, (F_, b_, Q_) = E.mstep_dynamics(st["S_zz"], st["S_xz"], st["S_xx"], pr)
        assert flag == 0 and rflag == 0
        _close(A[:, :dx], F_, 1e-12, "F")
        _close(A[:, dx], b_, 1e-12, "b")
        _close(Q, Q_, 1e-12, "Q")
        assert np.array_equal(Q, Q.T)
    Syy, nobs = E.syy_nobs([ys])
    flag, HC, R = hs.mstep_obs(dx, dy, np.concatenate([got["So_zz"].ravel(), got["S_yz"].ravel()]), Syy, nobs)
    rflag, (H_, c_, R_) = E.mstep_observations(st["So_zz"], st["S_yz"], Syy, nobs)
    assert flag == 0 and rflag == 0
    _close(HC[:, :dx], H_, 1e-12, "H")
    _close(HC[:, dx], c_, 1e-12, "c")
    _close(R, R_, 1e-12, "R")
    assert np.array_equal(R, R.T)
    # three sequences' initial moments
    sm0 = st["sm0"] + 0.3 * rng.standard_normal((3, dx))
    sP0 = np.stack([st["sP0"] * (1.0 + 0.1 * k) for k in range(3)])
    flag, m0, P0 = hs.mstep_init(sm0, sP0)
    rflag, (m0_, P0_) = E.mstep_initial(sm0, sP0)
    assert flag == 0 and rflag == 0
    _close(m0, m0_, 1e-12, "m0")
    _close(P0, P0_, 1e-12, "P0")
    assert np.array_equal(P0, P0.T)


def test_singular_gram_raises_the_flag():
    """T = 2 at dx = 4: one transition.  With exact smoothed moments S_zz = E[z_0 z_0^T] has the Schur complement sP_0, so it is singular exactly when x_0 is
    known -- from a path (sP = 0), or from a prior that pins x_0 (P0 = 1e-20 I: every pivot after the first is below 2^-46 of its diagonal)."""
    dx, dy = 4, 3
    rng = np.random.default_rng(5)
    p = E.random_model(rng, dx, dy)
    x, ys = E.simulate(rng, p, 2)
    z = np.append(x[0], 1.0)
    S_zz, S_xz, S_xx = np.outer(z, z), np.outer(x[1], z), np.outer(x[1], x[1])
    flag, A, Q = hs.mstep_dyn(dx, np.concatenate([S_zz.ravel(), S_xz.ravel(), S_xx.ravel()]))
    assert flag == 1 and np.all(np.isnan(A)) and np.all(np.isnan(Q))   # nothing was written
    assert E.mstep_dynamics(S_zz, S_xz, S_xx) == (1, None)
    p["P0"] = 1e-20 * np.eye(dx)
    st, _, (ms, Ps, sms, sPs, X) = E.e_step(ys, p)
    _, full = hs.stats(p["F"], p["Q"], ys, Ps, sms, sPs)
    n = dx + 1
    flag, A, Q = hs.mstep_dyn(dx, full[:n * n + dx * n + dx * dx])
    assert flag == 1 and np.all(np.isnan(A)) and np.all(np.isnan(Q))
    assert E.mstep_dynamics(st["S_zz"], st["S_xz"], st["S_xx"])[0] == 1
    # the other blocks of the same statistics do update
    Syy, nobs = E.syy_nobs([ys])
    got = E.split(full, dx, dy)
    assert hs.mstep_obs(dx, dy, np.concatenate([got["So_zz"].ravel(), got["S_yz"].ravel()]), Syy, nobs)[0] in (0, 2)   # (two rows cannot give a dy = 3 R)
    assert hs.mstep_init(got["sm0"][None], got["sP0"][None])[0] == 0


def test_restatement_em_monotone_and_order_independent():
    ys, start, _ = E.em_problem()
    its, ells, flags = E.em([ys], start, 15)
    assert not flags.any()
    assert np.all(np.diff(ells) >= -1e-9 * np.abs(ells[:-1])), np.diff(ells)
    assert ells[-1] > ells[0] + 1.0   # the fit moved
    its_r, ells_r, flags_r = E.em([ys], start, 15, reverse=True)
    assert not flags_r.any()
    for a, b in zip(its, its_r):
        for k in E.NAMES:
            assert np.max(np.abs(a[k] - b[k])) <= 1e-10, (k, np.max(np.abs(a[k] - b[k])))


def _lg(T, dx, dy, rng=None):
    p = E.random_model(rng or np.random.default_rng(0), dx, dy)
    bt = np.broadcast_to
    return K.LGSSM(p["m0"], p["P0"], bt(p["F"], (T - 1, dx, dx)), bt(p["Q"], (T - 1, dx, dx)), bt(p["b"], (T - 1, dx)), bt(p["H"], (T, dy, dx)),
                   bt(p["R"], (T, dy, dy)), bt(p["c"], (T, dy)))


def test_refusals_come_before_a_handle(monkeypatch):
    def no_handle(*a, **k):
        raise AssertionError("a handle was taken")

    monkeypatch.setattr(_lib, "default_handle", no_handle)
    T, dx, dy = 6, 2, 3
    ys = np.random.default_rng(1).standard_normal((T, dy))
    lg = _lg(T, dx, dy)
    with pytest.raises(ValueError, match="unknown parameter"):
        K.fit_em(ys, lg, 2, update=("F", "b", "Q", "G"))
    for bad in (("F",), ("F", "b"), ("H", "R"), ("m0",), ("F", "b", "Q", "c")):
        with pytest.raises(ValueError, match="one block"):
            K.fit_em(ys, lg, 2, update=bad)
    with pytest.raises(ValueError, match="dx <= 4"):
        K.fit_em(np.zeros((T, dy)), _lg(T, 5, dy), 2)
    with pytest.raises(ValueError, match="dy <= 8"):
        K.fit_em(np.zeros((T, 9)), _lg(T, dx, 9), 2)
    with pytest.raises(ValueError, match="T >= 2"):
        K.fit_em(np.zeros((1, dy)), _lg(1, dx, dy), 2)
    for k in (2, 3, 4, 5, 6, 7):
        arrs = [np.array(a) for a in lg]
        arrs[k][1] = arrs[k][1] * 1.5 + 0.1
        with pytest.raises(ValueError, match="varies in time"):
            K.fit_em(ys, K.LGSSM(*arrs), 2)
    with pytest.raises(ValueError, match="prior is for d = 3"):
        K.fit_em(ys, lg, 2, prior=MNIWPrior(np.zeros((3, 4)), np.eye(4), 5.0, np.eye(3)))
    with pytest.raises(ValueError, match="MNIWPrior"):
        K.fit_em(ys, lg, 2, prior=(1, 2, 3, 4))
    with pytest.raises(ValueError, match="needs the dynamics block"):
        K.fit_em(ys, lg, 2, update=("H", "c", "R"), prior=MNIWPrior(np.zeros((2, 3)), np.eye(3), 4.0, np.eye(2)))
    part = ys.copy()
    part[2, 1] = np.nan
    with pytest.raises(ValueError, match="partly NaN"):
        K.fit_em(part, lg, 2)
    with pytest.raises(ValueError, match="shape"):
        K.fit_em(ys[None, None], lg, 2)
    with pytest.raises(ValueError, match="expected shape"):
        K.fit_em(np.zeros((T + 1, dy)), lg, 2)
    # the dynamics-only fit takes partly observed rows (as `filtering` does): it gets as far as asking for a handle
    with pytest.raises(AssertionError, match="a handle was taken"):
        K.fit_em(part, lg, 2, update=("F", "b", "Q"))
    # smoothing_lag_one
    with pytest.raises(ValueError, match="dx <= 4"):
        K.smoothing_lag_one(np.zeros((T, dy)), _lg(T, 5, dy), True)
    with pytest.raises(ValueError, match="T >= 2"):
        K.smoothing_lag_one(np.zeros((1, dy)), _lg(1, dx, dy), True)
    arrs = [np.array(a) for a in lg]
    arrs[2][1] *= 0.5
    with pytest.raises(ValueError, match="varies in time"):
        K.smoothing_lag_one(ys, K.LGSSM(*arrs), True)


def test_symbols_in_the_built_library():
    lib = _lib.load()
    for name in ("auxssm_kalman_smooth_stats", "auxssm_lgssm_em_mstep"):
        assert name in _lib.exported_symbols() and hasattr(lib, name)
    assert lib.auxssm_version() == 108
