"""CPU: the conjugate step on linear-Gaussian dynamics (loop.DynamicsThetaStep / csrc/dynamics_theta.h) without a device.
  * self-checks of the literal NumPy restatement tests/dynamics_theta_np.py: a vanishing K0 gives the least-squares fit; 2e5 explicit draws have the matrix-normal
    inverse-Wishart means; the gamma sampler has the gamma mean and variance;
  * the AX_HD header the kernels compile, run under g++ (tests/hostsim_dynamics_theta), against the restatement: statistics, posterior and draw at 1e-12 relative
    for d = 1 .. 4 (relative to the largest entry of each matrix: Psi_n is a difference of sums), the failure flags, and the gamma generator (its normals come from
    the table-driven Box-Muller transform, pinned to the restatement's libm form at 1e-12: the draws are compared at 1e-10);
  * validation and refusals of loop.MNIWPrior / loop.DynamicsThetaStep."""
import numpy as np
import numpy.testing as npt
import pytest

from tests import dynamics_theta_cases as DC, dynamics_theta_np as NP, hostsim_dynamics_theta as HS

SHAPES = DC.GAMMA_SHAPES
moments_within = DC.moments_within


def _problem(d, T, seed, scale=1.0):
    """a stable VAR(1) trajectory and a proper prior"""
    rng = np.random.default_rng(seed)
    n = d + 1
    F = 0.6 * np.eye(d) + 0.1 * rng.standard_normal((d, d))
    b = 0.3 * rng.standard_normal(d)
    Lq = np.tril(0.2 * rng.standard_normal((d, d))) + 0.5 * np.eye(d)
    x = np.zeros((T, d))
    x[0] = rng.standard_normal(d)
    for t in range(T - 1):
        x[t + 1] = F @ x[t] + b + Lq @ rng.standard_normal(d)
    x *= scale
    M0 = 0.1 * rng.standard_normal((d, n))
    a = rng.standard_normal((n, n))
    K0 = 0.5 * np.eye(n) + 0.1 * a @ a.T
    c = rng.standard_normal((d, d))
    Psi0 = np.eye(d) + 0.2 * c @ c.T
    nu0 = d + 2.5
    return dict(x=x, M0=M0, K0=K0, nu0=nu0, Psi0=Psi0, F=F, b=b, Q=Lq @ Lq.T)


def _noise(d, seed, nu, lead=()):
    rng = np.random.default_rng(seed)
    chi = np.stack([rng.chisquare(nu - i, lead) for i in range(d)], axis=-1)
    return chi, rng.standard_normal(lead + (d, d)), rng.standard_normal(lead + (d, d + 1))


# ---- the restatement itself ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_vanishing_prior_precision_gives_least_squares(d):
    p = _problem(d, 400, d)
    x = p["x"]
    S = NP.stats(x)
    Mn, Kn, nun, Psi = NP.posterior(S, x.shape[0] - 1, p["M0"], 1e-12 * np.eye(d + 1), p["nu0"], p["Psi0"])
    Z = np.concatenate([x[:-1], np.ones((x.shape[0] - 1, 1))], axis=1)
    ls = np.linalg.lstsq(Z, x[1:], rcond=None)[0].T
    npt.assert_allclose(Mn, ls, rtol=1e-8, atol=1e-10)
    res = x[1:] - Z @ ls.T
    npt.assert_allclose(Psi, p["Psi0"] + res.T @ res, rtol=1e-8, atol=1e-9)
    assert nun == p["nu0"] + x.shape[0] - 1


@pytest.mark.parametrize("d", [1, 3])
def test_explicit_draws_have_the_posterior_means(d):
    N = 200_000
    p = _problem(d, 60, 10 + d)
    post = NP.posterior(NP.stats(p["x"]), 59, p["M0"], p["K0"], p["nu0"], p["Psi0"])
    Mn, Kn, nun, Psi = post
    chi, ew, ea = _noise(d, 77, nun, (N,))
    Q, A = NP.draw(post, chi, ew, ea)
    for got, want in ((A, Mn), (Q, Psi / (nun - d - 1))):
        se = got.std(axis=0, ddof=1) / np.sqrt(N)
        assert np.all(np.abs(got.mean(axis=0) - want) <= 5 * se), (np.abs(got.mean(axis=0) - want) / se).max()
    npt.assert_array_equal(Q, np.swapaxes(Q, 1, 2))


def test_gamma_restatement_moments():
    g = NP.gamma((2024, 7), 3, 60_000, SHAPES)
    assert np.all(np.isfinite(g)) and np.all(g > 0)
    for i, a in enumerate(SHAPES):
        ok, info = moments_within(g[:, i], a)
        assert ok, (a, info)


# ---- the header under g++ against the restatement -------------------------------------------------------------------------------------
def _rel(got, want):
    return float(np.max(np.abs(np.asarray(got) - np.asarray(want))) / np.max(np.abs(want)))


@pytest.mark.parametrize("T", [2, 3, 57])
@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_header_statistics_posterior_and_draw(d, T):
    p = _problem(d, T, 100 * d + T)
    x, n = p["x"], d + 1
    full = HS.stats(x)
    want = NP.stats_flat(x)
    o = 0
    for size in (n * n, d * n, d * d):
        assert _rel(full[o:o + size], want[o:o + size]) <= 1e-12
        o += size
    zz = full[:n * n].reshape(n, n)
    npt.assert_array_equal(zz, zz.T)
    chi, ew, ea = _noise(d, 5 * d + T, p["nu0"] + T - 1)
    flag, post, Q, A = HS.update(full, T - 1, p["M0"], p["K0"], p["nu0"], p["Psi0"], chi, ew, ea)
    rflag, rpost, rQ, rA = NP.step(x, p["M0"], p["K0"], p["nu0"], p["Psi0"], chi, ew, ea)
    assert flag == 0 and rflag == 0
    got = (post[:d * n], post[d * n:d * n + n * n], post[d * n + n * n:d * n + n * n + 1], post[d * n + n * n + 1:])
    for g, w in zip(got, rpost):
        assert _rel(g, np.ravel(w)) <= 1e-12
    assert _rel(Q, rQ) <= 1e-12 and _rel(A, rA) <= 1e-12
    npt.assert_array_equal(Q, Q.T)
    # chi_scale: Gamma(shape / 2, 1) draws doubled are the chi-squares
    flag2, _, Q2, A2 = HS.update(full, T - 1, p["M0"], p["K0"], p["nu0"], p["Psi0"], 0.5 * chi, ew, ea, chi_scale=2.0)
    assert flag2 == 0
    npt.assert_array_equal(Q2, Q)
    npt.assert_array_equal(A2, A)


@pytest.mark.parametrize("d", [1, 4])
def test_header_flags_a_degenerate_chain(d):
    """all steps equal, a tiny Psi0 and a prior mean that reproduces the constant: Psi_n is rounding noise of the sums it is the difference of -> flag 2;
    with a vanishing K0 as well, K_n = S_zz has rank one -> flag 1.  As the restatement says, and nothing non-finite comes back."""
    p = _problem(d, 40, 3)
    const = 1.7 + np.arange(d)
    x = np.tile(const, (40, 1))
    M0 = np.concatenate([np.zeros((d, d)), const[:, None]], axis=1)
    Psi0 = 1e-200 * np.eye(d)
    chi, ew, ea = _noise(d, 1, p["nu0"] + 39)
    for K0, want in ((np.eye(d + 1), 2), (1e-200 * np.eye(d + 1), 1)):
        flag, post, Q, A = HS.update(HS.stats(x), 39, M0, K0, p["nu0"], Psi0, chi, ew, ea)
        assert flag == want and NP.step(x, M0, K0, p["nu0"], Psi0, chi, ew, ea)[0] == want
        assert np.all(np.isfinite(post))
    chi[0] = 0.0
    assert HS.update(HS.stats(p["x"]), 39, p["M0"], p["K0"], p["nu0"], p["Psi0"], chi, ew, ea)[0] == 3


def test_header_gamma_generator():
    key = (123456789, 42)
    x, u, ub = NP.gamma_variates(key, 5, np.array([0, 1, 99, 2 ** 33 + 5], np.uint64), 3)
    for j, g in enumerate([0, 1, 99, 2 ** 33 + 5]):
        got = HS.gamma_variates(key, 5, g, 3)
        npt.assert_allclose(got[0], x[j], rtol=1e-12, atol=1e-13)
        assert got[1] == u[j] and got[2] == ub[j]
    want, margin = NP.gamma(key, 5, 4096, SHAPES, with_margin=True)
    got, gm = HS.gamma(key, 5, 4096, SHAPES)
    assert margin > 1e-9, margin   # (no decision of the restatement is within rounding of its threshold: the two take the same ones)
    assert np.all(np.isfinite(got)) and np.all(gm > 0)
    npt.assert_allclose(got, want, rtol=1e-10)


# ---- validation and refusals (no device) ---------------------------------------------------------------------------------------------
def _lg_model(d=2, T=6, time_varying=False):
    from aux_ssm_samplers_amd.kalman import LGConcatModel
    bt = np.broadcast_to
    F = np.stack([0.5 * np.eye(d)] * (T - 1))
    if time_varying:
        F[2] *= 1.1
    else:
        F = bt(0.5 * np.eye(d), (T - 1, d, d))
    return LGConcatModel(np.zeros(d), np.eye(d), F, bt(np.eye(d), (T - 1, d, d)), bt(np.zeros(d), (T - 1, d)), bt(np.eye(d), (T, d, d)),
                         bt(np.eye(d), (T, d, d)), bt(np.zeros(d), (T, d)), np.zeros((T, d)))


def _prior(d=2):
    from aux_ssm_samplers_amd.loop import MNIWPrior
    return MNIWPrior(np.zeros((d, d + 1)), np.eye(d + 1), d + 1.0, np.eye(d))


def test_prior_validation():
    from aux_ssm_samplers_amd.loop import MNIWPrior
    d = 2
    good = dict(M0=np.zeros((d, d + 1)), K0=np.eye(d + 1), nu0=3.0, Psi0=np.eye(d))
    p = MNIWPrior(**good)
    assert p.d == 2 and p.struct().chi_scale == 2.0
    bad = {
        "shape": dict(good, M0=np.zeros((d, d))),
        "finite": dict(good, Psi0=np.array([[1.0, 0.0], [0.0, np.nan]])),
        "nu0": dict(good, nu0=1.0),
        "symmetric": dict(good, K0=np.eye(3) + np.triu(np.ones((3, 3)), 1) * 0.1),
        "positive definite": dict(good, Psi0=np.array([[1.0, 2.0], [2.0, 1.0]])),
    }
    for why, kw in bad.items():
        with pytest.raises(ValueError, match="MNIWPrior"):
            MNIWPrior(**kw)
    with pytest.raises(ValueError, match="dx <= 4"):
        MNIWPrior(np.zeros((5, 6)), np.eye(6), 6.0, np.eye(5)).struct()


def test_step_refusals():
    from aux_ssm_samplers_amd.loop import DynamicsThetaStep
    from aux_ssm_samplers_amd.kalman import models as M
    step = DynamicsThetaStep(_lg_model(), _prior())
    assert step._shapes == [0.5 * (3.0 + 5), 0.5 * (3.0 + 5 - 1)]
    with pytest.raises(ValueError, match="varies in time"):
        DynamicsThetaStep(_lg_model(time_varying=True), _prior())
    with pytest.raises(ValueError, match="the prior is for d = 3"):
        DynamicsThetaStep(_lg_model(), _prior(3))
    with pytest.raises(ValueError, match="MNIWPrior"):
        DynamicsThetaStep(_lg_model(), None)
    T = 6
    lor = M.LorenzModel(np.zeros((T, 1)), np.zeros((T, 1, 3)), np.broadcast_to(np.eye(1), (T, 1, 1)), np.zeros((T, 1)), np.zeros(3), np.eye(3),
                        np.array([10.0, 28.0, 2.6]), 1.0, 0.01)
    with pytest.raises(ValueError, match="LorenzThetaStep"):
        DynamicsThetaStep(lor, _prior(3))
    mvt = M.MVTModel(np.zeros((T, 2)), np.zeros(2), np.ones(2), 0.5 * np.ones(2), np.ones(2), np.zeros(2), 4.0, np.eye(2))
    with pytest.raises(ValueError, match="MVTModel"):
        DynamicsThetaStep(mvt, _prior(2))
    with pytest.raises(ValueError, match="not a model"):
        DynamicsThetaStep(object(), _prior())
    with pytest.raises(ValueError, match="cSMC"):
        step(np.array([1, 2], np.uint32), object())
    sv = M.SVModel(np.zeros((T, 2)), np.zeros(2), np.eye(2), 0.9 * np.eye(2), 0.1 * np.eye(2), np.zeros(2))
    assert DynamicsThetaStep(sv, _prior()).model is sv
    wide = _lg_model(d=5)
    with pytest.raises(ValueError, match="dx <= 4"):
        DynamicsThetaStep(wide, _prior(5))


def test_a_sweep_refuses_a_chain_count_the_per_chain_dynamics_do_not_have():
    """the guard kalman.get_kernel's device sweep runs before every launch (generic._check_per_chain_dynamics): a model whose dynamics a DynamicsThetaStep made
    per-chain for C chains is swept with C chains only -- more would read past the end of its (C, d, d) / (C, d) buffers"""
    from types import SimpleNamespace as NS
    from aux_ssm_samplers_amd.kalman.generic import _check_per_chain_dynamics as check
    rows = lambda c: (NS(shape=(c, 2, 2)), NS(shape=(c, 2)), NS(shape=(c, 2, 2)))
    check(NS(bufs={}), 7)                                   # a model no step has touched
    check(NS(bufs={"dynamics_theta": rows(3)}), 3)
    check(NS(bufs={"dynamics_theta": rows(1)}), 9)          # one row, chain stride 0: shared by every chain
    for C in (1, 2, 4, 34):
        with pytest.raises(ValueError, match="per-chain dynamics .* of 3 chains"):
            check(NS(bufs={"dynamics_theta": rows(3)}), C)
