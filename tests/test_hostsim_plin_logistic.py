"""The per-step arithmetic of the logistic-linear Kalman factory (csrc/kalman_plin.h::plin_step_logistic -- the text k_plin_obs_logistic of kalman_plin.hip
compiles) run on the CPU (tests/hostsim_plin_logistic: a plain g++ build behind ctypes) against the NumPy factories of kalman.BinomialLinearModel and
kalman.NegBinomialLinearModel, at every (dx, dy) of tests/kalman_logistic_lin_cases.py, both families and both orders: value = log g_t, ys and Om.  float64 at
1e-12 relative; float32 against float64 at a bar measured here (see the test).  The cells' chains start at eta = -+30 in one channel."""
import numpy as np
import numpy.testing as npt
import pytest

from tests import hostsim_plin_logistic as HS, kalman_logistic_lin_cases as LC

SHAPES = sorted({s[:3] for s in LC.ONE_CHAIN_SHAPES + LC.CHAIN_SHAPES})


def _inputs(family, dx, dy, T, order, f32=False):
    cell = LC._build(family, dx, dy, T, 1, order, 0, f32)
    model, x, delta = cell["model"], cell["x"][0], cell["delta"]
    u = x + np.sqrt(0.5 * delta) * cell["eps_aux"][0]
    if f32:
        u = u.astype(np.float32).astype(np.float64)
    ts, ks = cell["sat"]
    assert abs(x[ts] @ model.H[ks] + model.c[ks]) > 29.9
    return model, x, u, delta


def _steps(model, x, u, delta, order, dtype=np.float64):
    return HS.steps(x, u, model.yobs, model.H, model.c, model.size_s, model.size_w, delta, order, dtype)


def _per_step_value(model, x):
    _, eta, yy, m, e, _ = model._terms(x)
    return np.sum(yy * eta - m * (np.maximum(eta, 0.0) + np.log1p(e)), axis=1)


@pytest.mark.parametrize("family", LC.FAMILIES)
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("dx,dy,T", SHAPES)
def test_fp64_step_is_the_numpy_factory(family, dx, dy, T, order):
    model, x, u, delta = _inputs(family, dx, dy, T, order)
    value, ys, Om = _steps(model, x, u, delta, order)
    want_ys, _, want_R, _ = model.observations_factory(x, u, delta)
    want_v = _per_step_value(model, x)
    npt.assert_allclose(value, want_v, rtol=1e-12, atol=1e-12 * np.abs(want_v).max())
    npt.assert_allclose(ys, want_ys, rtol=1e-12, atol=1e-12 * np.abs(want_ys).max())
    if order == 2:
        npt.assert_allclose(Om, want_R, rtol=1e-12, atol=1e-12 * np.abs(want_R).max())
        npt.assert_array_equal(Om, np.swapaxes(Om, 1, 2))


def test_a_missing_channels_size_is_never_looked_at():
    """NaN sizes under NaN data: the step's sums are those of the model without the channel"""
    model, x, u, delta = _inputs("binomial", 2, 7, 129, 2)
    s = model.size_s.copy()
    y = model.yobs.copy()
    y[:, 3] = np.nan
    s_nan = s.copy()
    s_nan[3] = np.nan
    a = HS.steps(x, u, y, model.H, model.c, s, model.size_w, delta, 2)
    b = HS.steps(x, u, y, model.H, model.c, s_nan, model.size_w, delta, 2)
    for p, q in zip(a, b):
        npt.assert_array_equal(p, q)
    assert np.isfinite(b[0]).all() and np.isfinite(b[1]).all()


# float32 against float64 on float32-rounded inputs: max |error| / max |value| per output.  Measured on this harness over SHAPES, both families and both orders
# (g++ -O1, -ffp-contract=off), at worst: value 5.05e-5 (negbinomial, dx = 1, dy = 1, T = 2; 1.6e-5 at negbinomial (2, 7, 257); every binomial cell below 1e-6),
# ys 2.06e-7 (negbinomial, dx = 4, dy = 65, T = 70, second order) and Om 3.33e-7 (negbinomial, dx = 3, dy = 5, T = 70); the bars are twice that, rounded up to
# one digit.  ys and Om are a few ulp of the largest value.  The value is not: with a count of 1200 at eta = log 400 its two terms y eta = 7.2e3 and m softplus =
# 7.2e3 cancel to about -20, so one float32 rounding of either (4e-4) is 2e-5 of it, and the two-step cell has no larger value to be measured against.  That
# cancellation is the formula's (_LogisticModel's, and the pointwise device kinds'), not the loading matrix's.
F32_BARS = dict(value=2e-4, ys=5e-7, Om=7e-7)


@pytest.mark.parametrize("family", LC.FAMILIES)
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("dx,dy,T", SHAPES)
def test_fp32_step_against_fp64(family, dx, dy, T, order):
    model, x, u, delta = _inputs(family, dx, dy, T, order, f32=True)
    v64, ys64, Om64 = _steps(model, x, u, delta, order)
    v32, ys32, Om32 = _steps(model, x, u, delta, order, np.float32)
    err = dict(value=np.abs(v32 - v64).max() / np.abs(v64).max(), ys=np.abs(ys32 - ys64).max() / np.abs(ys64).max())
    if order == 2:
        err["Om"] = np.abs(Om32 - Om64).max() / np.abs(Om64).max()
    print(f"hostsim_plin_logistic fp32 {family} dx={dx} dy={dy} T={T} order={order}: " + "  ".join(f"{k} {v:.2e}" for k, v in err.items()))
    assert np.isfinite(v32).all() and np.isfinite(ys32).all()
    for k, v in err.items():
        assert v < F32_BARS[k], (k, v)
