"""The per-step arithmetic of the Poisson-linear Kalman factory (csrc/kalman_plin.h::plin_step -- the text the kernels of kalman_plin.hip compile) run on the CPU
(tests/hostsim_plin: a plain g++ build behind ctypes) against kalman.PoissonLinearModel's NumPy factories, at every (dx, dy) of tests/kalman_poisson_lin_cases.py
and both orders: value = log g_t, ys and Om.  float64 at 1e-12 relative; float32 against float64 at a bar measured here (see the test)."""
import numpy as np
import numpy.testing as npt
import pytest

from tests import hostsim_plin as HS, kalman_poisson_lin_cases as LC

SHAPES = sorted({s[:3] for s in LC.ONE_CHAIN_SHAPES + LC.CHAIN_SHAPES})


def _inputs(dx, dy, T, order, f32=False):
    cell = LC._build(dx, dy, T, 1, order, 0, f32)
    model, x, delta = cell["model"], cell["x"][0], cell["delta"]
    u = x + np.sqrt(0.5 * delta) * cell["eps_aux"][0]
    if f32:
        u = u.astype(np.float32).astype(np.float64)
    return model, x, u, delta


def _per_step_value(model, x):
    mask, eta, e, yy = model._terms(x)
    return np.sum(yy * eta - e, axis=1)


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("dx,dy,T", SHAPES)
def test_fp64_step_is_the_numpy_factory(dx, dy, T, order):
    model, x, u, delta = _inputs(dx, dy, T, order)
    value, ys, Om = HS.steps(x, u, model.yobs, model.H, model.c, delta, order)
    want_ys, _, want_R, _ = model.observations_factory(x, u, delta)
    want_v = _per_step_value(model, x)
    npt.assert_allclose(value, want_v, rtol=1e-12, atol=1e-12 * np.abs(want_v).max())
    npt.assert_allclose(ys, want_ys, rtol=1e-12, atol=1e-12 * np.abs(want_ys).max())
    if order == 2:
        npt.assert_allclose(Om, want_R, rtol=1e-12, atol=1e-12 * np.abs(want_R).max())
        npt.assert_array_equal(Om, np.swapaxes(Om, 1, 2))
        # the dense Gaussian term k_plin_terms adds up, against the oracle's own density
        got = HS.norm_logpdf(ys, x, Om)
        r = ys - x
        want = np.array([-0.5 * r[t] @ np.linalg.solve(want_R[t], r[t]) - 0.5 * np.linalg.slogdet(want_R[t])[1] - 0.5 * dx * np.log(2 * np.pi) for t in range(T)])
        npt.assert_allclose(got, want, rtol=1e-12, atol=1e-12 * np.abs(want).max())


# float32 against float64 on float32-rounded inputs: max |error| / max |value| per output.  Measured on this harness over SHAPES and both orders (g++ -O1,
# -ffp-contract=off): value 2.17e-7 (dx = 4, dy = 65, T = 70), ys 2.69e-7 and Om 2.60e-7 (second order) at worst; the bars are twice that, rounded up.  A few
# ulp of the largest value is what these sums can give: the value adds 64 terms y eta - e per block in float32, H' (y - e) cancels.
F32_BARS = dict(value=5e-7, ys=6e-7, Om=6e-7)


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("dx,dy,T", SHAPES)
def test_fp32_step_against_fp64(dx, dy, T, order):
    model, x, u, delta = _inputs(dx, dy, T, order, f32=True)
    v64, ys64, Om64 = HS.steps(x, u, model.yobs, model.H, model.c, delta, order)
    v32, ys32, Om32 = HS.steps(x, u, model.yobs, model.H, model.c, delta, order, np.float32)
    err = dict(value=np.abs(v32 - v64).max() / np.abs(v64).max(), ys=np.abs(ys32 - ys64).max() / np.abs(ys64).max())
    if order == 2:
        err["Om"] = np.abs(Om32 - Om64).max() / np.abs(Om64).max()
    print(f"hostsim_plin fp32 dx={dx} dy={dy} T={T} order={order}: " + "  ".join(f"{k} {v:.2e}" for k, v in err.items()))
    for k, v in err.items():
        assert v < F32_BARS[k], (k, v)
