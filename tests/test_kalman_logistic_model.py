"""kalman.BinomialModel and kalman.NegBinomialModel on the CPU: construction and validation, the NumPy factories against finite differences of the potential,
the two densities written out (Bernoulli; the negative-binomial pmf through lgamma), saturation, and the cells of tests/kalman_logistic_cases.py under the margin
rule.  The device sweep is tests/test_gpu_kalman_logistic.py's."""
import math

import numpy as np
import numpy.testing as npt
import pytest

from tests import kalman_logistic_cases as LC


def _model(family, T=7, d=3, order=1, seed=2):
    y, par, path, _, (m0, P0, F, Q, b) = LC.make_data(family, d, T, seed)
    return LC.make_model(family, y, par, m0, P0, F, Q, b, order), path


def test_construction_and_kinds():
    from aux_ssm_samplers_amd import _lib
    from aux_ssm_samplers_amd import kalman
    from aux_ssm_samplers_amd.kalman import generic
    from aux_ssm_samplers_amd.workloads import logistic_kalman_setup
    assert (_lib.KMODEL_LOGISTIC_FIRST, _lib.KMODEL_LOGISTIC_SECOND) == (13, 14)
    assert "BinomialModel" in kalman.__all__ and "NegBinomialModel" in kalman.__all__
    for family, cls in (("binomial", kalman.BinomialModel), ("negbinomial", kalman.NegBinomialModel)):
        for order, kind in ((1, 13), (2, 14)):
            m, _ = _model(family, T=5, d=2, order=order)
            assert isinstance(m, cls) and (m.kmodel, m.dense_only, m.T, m.dx, m.p_obs) == (kind, False, 5, 2, 2) and m.size.shape == (5, 2)
            assert generic._same_device_model(m.dynamics_factory, m.observations_factory, m.log_likelihood_fn) is m
        model, x0 = logistic_kalman_setup(12, 3, family, 1)
        assert isinstance(model, cls) and model.order == 1 and x0.shape == (12, 3) and model.yobs.shape == (12, 3)
    model, _ = logistic_kalman_setup(50, 3, "binomial", 0)
    assert np.all(model.trials[:, 0] == 1) and model.trials.min() >= 1 and model.trials.max() <= 40 and np.all(model.yobs <= model.trials)
    model, _ = logistic_kalman_setup(50, 3, "negbinomial", 0)
    npt.assert_array_equal(model.size, model.yobs + 3.0)
    with pytest.raises(ValueError):
        logistic_kalman_setup(5, 1, "poisson")


def test_validation_errors():
    from aux_ssm_samplers_amd.kalman import BinomialModel, NegBinomialModel
    T, d = 4, 2
    m0, P0, F, Q, b = np.zeros(d), np.eye(d), 0.9 * np.eye(d), 0.1 * np.eye(d), np.zeros(d)
    y = np.array([[0.0, 3.0], [1.0, np.nan], [2.0, 2.5], [np.nan, 0.0]])
    dyn = (m0, P0, F, Q, b)
    # accepted: scalar, (dx,) and (T, dx) sizes; non-integer values; anything under a missing y
    for trials in (3.0, np.array([2.0, 3.0]), np.full((T, d), 3.0)):
        assert BinomialModel(y, trials, *dyn).size.shape == (T, d)
    tr = np.full((T, d), 3.0)
    tr[1, 1], tr[3, 0] = np.nan, np.inf
    BinomialModel(y, tr, *dyn)
    for r in (0.5, np.array([0.5, 4.0]), np.full((T, d), 2.0)):
        assert NegBinomialModel(y, r, *dyn, order=2).size.shape == (T, d)
    rr = np.full((T, d), 2.0)
    rr[1, 1] = np.nan
    NegBinomialModel(y, rr, *dyn)
    for cls, par in ((BinomialModel, 3.0), (NegBinomialModel, 3.0)):
        with pytest.raises(ValueError):
            cls(y, par, *dyn, order=3)
        with pytest.raises(ValueError):
            cls(y[:, 0], par, *dyn)                     # ys must be (T, dx)
        with pytest.raises(ValueError):
            cls(y, np.full((T, d + 1), 3.0), *dyn)      # a size of another shape
        with pytest.raises(ValueError):
            cls(y, np.full(T, 3.0), *dyn)               # (T,) is not (dx,)
        with pytest.raises(ValueError):
            cls(y, 0.0, *dyn)                           # size must be > 0
        with pytest.raises(ValueError):
            cls(y, np.array([3.0, -1.0]), *dyn)
        bad = y.copy()
        bad[0, 0] = -1.0
        with pytest.raises(ValueError):
            cls(bad, par, *dyn)                         # a finite negative y
        nf = np.full((T, d), 3.0)
        nf[0, 1] = np.nan
        with pytest.raises(ValueError):
            cls(y, nf, *dyn)                            # a non-finite size under a finite y
    with pytest.raises(ValueError):
        BinomialModel(y, 2.9, *dyn)                     # y = 3 of 2.9 trials
    NegBinomialModel(y, 0.1, *dyn)                      # counts above r are what the negative binomial is for


@pytest.mark.parametrize("family", LC.FAMILIES)
def test_grad_and_lam_against_central_differences_of_log_potential(family):
    model, path = _model(family, order=2)
    rng = np.random.default_rng(0)
    x = path + 0.1 * rng.standard_normal(path.shape)
    grad, lam = model.grad_lam(x)
    h = 1e-4
    f0 = model.log_potential(x)
    for t, k in np.ndindex(*x.shape):
        e = np.zeros_like(x)
        e[t, k] = h
        fp, fm = model.log_potential(x + e), model.log_potential(x - e)
        # central differences of y x - m softplus(x): truncation m |sigma'''| h^2 / 6 <= m h^2 / 48 and m h^2 / 96 (|softplus'''| <= 1/(6 sqrt 3), |softplus''''| <= 1/8),
        # plus rounding of sums of size |f| <= 2e4 (2e-12) over 2 h and h^2
        m = np.nan_to_num(model.size[t, k])
        npt.assert_allclose((fp - fm) / (2 * h), grad[t, k], atol=1e-7 + 1e-8 * m)
        npt.assert_allclose(-(fp - 2 * f0 + fm) / h ** 2, lam[t, k], atol=2e-3 + 1e-8 * m)
    miss = ~np.isfinite(model.yobs)
    assert miss.any() and np.all(grad[miss] == 0) and np.all(lam[miss] == 0) and np.all(lam[~miss] > 0)
    assert np.isnan(model.size[miss]).any()    # a missing entry's size is not looked at


def test_binomial_at_one_trial_is_the_bernoulli_log_likelihood():
    from aux_ssm_samplers_amd.kalman import BinomialModel
    rng = np.random.default_rng(1)
    T, d = 11, 3
    x = 3.0 * rng.standard_normal((T, d))
    y = (rng.random((T, d)) < 0.5).astype(np.float64)
    y[4, 1] = np.nan
    model = BinomialModel(y, 1.0, np.zeros(d), np.eye(d), 0.9 * np.eye(d), 0.1 * np.eye(d), np.zeros(d))
    p = 1.0 / (1.0 + np.exp(-x))
    seen = np.isfinite(y)
    want = np.sum(np.where(seen, np.where(y == 1, np.log(p), np.log1p(-p)), 0.0))
    npt.assert_allclose(model.log_potential(x), want, rtol=1e-13)
    grad, lam = model.grad_lam(x)
    npt.assert_allclose(grad, np.where(seen, np.nan_to_num(y) - p, 0.0), rtol=1e-13, atol=1e-15)
    npt.assert_allclose(lam, np.where(seen, p * (1 - p), 0.0), rtol=1e-12)


def test_negative_binomial_against_lgamma_pmf_differences_in_x():
    """log pmf(y; r, p) = lgamma(y + r) - lgamma(r) - lgamma(y + 1) + y log p + r log(1 - p) at p = sigma(x): the potential leaves the three lgamma terms out, so
    differences of the potential between two states are differences of the log pmf"""
    from aux_ssm_samplers_amd.kalman import NegBinomialModel
    rng = np.random.default_rng(2)
    T, d = 9, 2
    y = rng.poisson(4.0, (T, d)).astype(np.float64)
    y[0, 0], y[3, 1] = 0.0, np.nan
    r = np.array([0.7, 3.0])
    model = NegBinomialModel(y, r, np.zeros(d), np.eye(d), 0.9 * np.eye(d), 0.1 * np.eye(d), np.zeros(d))

    def log_pmf(x):
        tot = 0.0
        for t, k in np.ndindex(T, d):
            if np.isfinite(y[t, k]):
                p = 1.0 / (1.0 + math.exp(-x[t, k]))
                tot += math.lgamma(y[t, k] + r[k]) - math.lgamma(r[k]) - math.lgamma(y[t, k] + 1.0) + y[t, k] * math.log(p) + r[k] * math.log1p(-p)
        return tot

    xa, xb = 2.0 * rng.standard_normal((T, d)), 2.0 * rng.standard_normal((T, d))
    npt.assert_allclose(model.log_potential(xa) - model.log_potential(xb), log_pmf(xa) - log_pmf(xb), rtol=1e-12)
    # the mean is r e^x: the gradient of the log pmf in x vanishes at x = log(y / r)
    xs = np.log(np.where(np.isfinite(y) & (y > 0), y, 1.0) / r)
    grad, _ = model.grad_lam(xs)
    npt.assert_allclose(grad[np.isfinite(y) & (y > 0)], 0.0, atol=1e-12)


@pytest.mark.parametrize("family", LC.FAMILIES)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_saturation_is_finite(family, dtype):
    """|x| = 40 and 800: value, grad, lam and both orders' pseudo-observations are finite in either precision (no exp overflows: the one exponential is exp(-|x|))"""
    T, d = 4, 2
    x = np.array([[40.0, -40.0], [800.0, -800.0], [0.0, 40.0], [-800.0, 800.0]], dtype)
    y = np.array([[3.0, 0.0], [5.0, 2.0], [np.nan, 1500.0], [0.0, 7.0]])
    par = np.array([[5.0, 1.0], [5.0, 2.0], [1.0, 1500.0], [40.0, 7.0]])
    dyn = (np.zeros(d), np.eye(d), 0.9 * np.eye(d), 0.1 * np.eye(d), np.zeros(d))
    for order in (1, 2):
        model = LC.make_model(family, y, par, *dyn, order)
        with np.errstate(all="raise"):
            try:
                val = model.log_potential(x)
                grad, lam = model.grad_lam(x)
            except FloatingPointError as e:   # (an underflow of exp(-800) to 0 is the intended result, not an error)
                if "underflow" not in str(e):
                    raise
                with np.errstate(under="ignore"):
                    val = model.log_potential(x)
                    grad, lam = model.grad_lam(x)
        assert grad.dtype == dtype and lam.dtype == dtype
        assert np.isfinite(val) and np.all(np.isfinite(grad)) and np.all(np.isfinite(lam)) and np.all(lam >= 0)
        m = model.size
        seen = np.isfinite(y)
        # saturated: grad -> y - m (x >> 0) or y (x << 0), lam -> 0
        big = seen & (np.abs(x) >= 40)
        npt.assert_allclose(grad[big], np.where(x > 0, y - m, y)[big], atol=1e-12 * 1500)
        assert np.all(lam[big] < 1e-13)
        ys, Hs, Rs, cs = model.observations_factory(x, x + dtype(0.1), 0.5)
        assert np.all(np.isfinite(ys)) and np.all(np.isfinite(Rs))


@pytest.mark.parametrize("family", LC.FAMILIES)
def test_factories_follow_the_specification(family):
    rng = np.random.default_rng(3)
    for order in (1, 2):
        model, path = _model(family, order=order)
        T, d = path.shape
        x, u, delta = path + 0.1 * rng.standard_normal((T, d)), path + 0.2 * rng.standard_normal((T, d)), 0.37
        mask = np.isfinite(model.yobs)
        sig = 1.0 / (1.0 + np.exp(-x))
        yy, mm = np.nan_to_num(model.yobs), np.nan_to_num(model.size)
        grad, lam = np.where(mask, yy - mm * sig, 0.0), np.where(mask, mm * sig * (1 - sig), 0.0)
        ys, Hs, Rs, cs = model.observations_factory(x, u, delta)
        npt.assert_array_equal(Hs, np.broadcast_to(np.eye(d), (T, d, d)))
        npt.assert_array_equal(cs, np.zeros((T, d)))
        if order == 1:
            npt.assert_allclose(ys, u + 0.5 * delta * grad, rtol=1e-13)
            npt.assert_allclose(Rs, np.broadcast_to(0.5 * delta * np.eye(d), (T, d, d)), rtol=1e-15)
        else:
            om = 1.0 / (lam + 2.0 / delta)
            npt.assert_allclose(ys, om * (2 * u / delta + grad + lam * x), rtol=1e-12)
            npt.assert_allclose(Rs, om[..., None] * np.eye(d), rtol=1e-13)
        assert np.all(np.isfinite(ys)) and np.all(np.isfinite(Rs))     # a missing entry never makes a pseudo-observation NaN
        npt.assert_allclose(ys[~mask], u[~mask], rtol=1e-15)
        npt.assert_allclose(np.einsum("tkk->tk", Rs)[~mask], 0.5 * delta, rtol=1e-15)


@pytest.mark.parametrize("family", LC.FAMILIES)
def test_cells_hold_what_they_promise(family):
    for d, T in [(1, 400), (4, 150), (30, 24), (2, 129)]:
        y, par, path, sat, _ = LC.make_data(family, d, T, 7 * d + T)
        cell = LC._build(family, d, T, 4, 1, 0)
        m = cell["model"].size
        seen = np.isfinite(y)
        assert np.isnan(y[0]).sum() == 1 and np.isnan(y[T // 2]).all() and np.isnan(y[T - 1]).sum() == 1 and np.isnan(y).sum() == d + 2
        assert (y[seen] == 0).any() and np.nanmax(m) >= 1000
        assert np.abs(cell["x"][0, sat[0], sat[1]]) > 20 and np.abs(cell["x"][1]).max() < 12 and abs(sat[2]) == 30
        if family == "binomial":
            assert (y[seen] == par[seen]).any() and np.sum(par[:, 0] == 1) >= T - 4 and np.nanmax(par) >= 1000
            assert np.isnan(par[T // 2]).all()
        else:
            assert np.isnan(m[~seen]).all()


@pytest.mark.parametrize("family", LC.FAMILIES)
@pytest.mark.parametrize("order", [1, 2])
def test_cells_are_well_posed_under_the_margin_rule(family, order):
    """every multi-chain cell of the GPU tests holds an accepted and a rejected chain at a margin of at least 0.05; every log alpha is finite and above -80"""
    cells = [(d, T, C, 7) for d, T, C in LC.CM_SHAPES] + ([(d, T, C, 1) for d, T, C in LC.WIDE_SHAPES] if order == 1 else []) + [(4, 150, 1, 1), (1, 2, 1, 1)]
    for d, T, C, every in cells:
        ref = LC.reference(family, d, T, C, order, True, every)
        la = ref["logs"][:, 0]
        assert np.all(np.isfinite(ref["logs"])) and np.all(la > LC.LOG_ALPHA_MIN) and np.all(np.isfinite(ref["x_prop"]))
        assert np.abs(ref["x_prop"] - ref["cell"]["x"][ref["chains"]]).max() > 1e-3
        for u, acc in zip(ref["us"], ref["accepted"]):
            margin = np.abs(np.log(u[ref["chains"]]) - np.minimum(la, 0.0))
            assert np.all(margin >= LC.MARGIN_MIN - 1e-12)
        flags = np.concatenate(ref["accepted"])
        if C > 1:
            assert flags.any() and not flags.all()
        else:
            assert bool(ref["accepted"][0][0]) and (not ref["accepted"][1][0] or la[0] >= -LC.MARGIN_MIN)
    # both scan forms of the oracle agree
    a, b_ = LC.reference(family, 4, 150, 1, order, True), LC.reference(family, 4, 150, 1, order, False)
    npt.assert_allclose(a["x_prop"], b_["x_prop"], rtol=1e-9, atol=1e-10)
    npt.assert_allclose(a["logs"], b_["logs"], rtol=1e-6, atol=1e-7)
