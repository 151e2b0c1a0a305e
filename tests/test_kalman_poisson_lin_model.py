"""kalman.PoissonLinearModel on the CPU: gradient and Lam against central differences of log_potential, both factories against their defining formulas, the
reduction to PoissonModel at H = I, c = 0, the oracle sweep on the factories in both scan forms, every refusal of the constructor, which kernel
kalman.get_kernel picks, and the conditions tests/kalman_poisson_lin_cases.py promises (with the oracle alone)."""
import numpy as np
import numpy.testing as npt
import pytest

from oracle import kalman_np as K
from tests import kalman_poisson_lin_cases as LC


def small(dx=3, dy=7, T=9, order=1, seed=3):
    model, path = LC.make_model(dx, dy, T, seed, order)
    rng = np.random.default_rng(seed)
    return model, path + 0.1 * rng.standard_normal(path.shape), rng


@pytest.mark.parametrize("dx,dy", [(1, 1), (2, 7), (4, 65)])
def test_grad_and_lam_are_the_derivatives_of_log_potential(dx, dy):
    model, x, _ = small(dx, dy)
    assert np.isnan(model.yobs).any()
    grad, lam = model.grad_lam(x)
    h = 1e-5
    for t in (0, 4, 8):
        for k in range(dx):
            xp, xm = x.copy(), x.copy()
            xp[t, k] += h
            xm[t, k] -= h
            fd = (model.log_potential(xp) - model.log_potential(xm)) / (2 * h)
            npt.assert_allclose(grad[t, k], fd, rtol=1e-6, atol=1e-6)
            gd = (model.grad_lam(xp)[0][t] - model.grad_lam(xm)[0][t]) / (2 * h)    # d grad / d x_k = column k of the Hessian = -Lam
            npt.assert_allclose(-lam[t, :, k], gd, rtol=1e-6, atol=1e-6)
    npt.assert_array_equal(lam, np.swapaxes(lam, 1, 2))
    assert np.all(np.linalg.eigvalsh(lam) > -1e-12)
    npt.assert_array_equal(grad[4], 0.0)   # the wholly missing row T // 2: no term at all
    npt.assert_array_equal(lam[4], 0.0)


@pytest.mark.parametrize("order", [1, 2])
def test_factories_are_their_formulas(order):
    model, x, rng = small(3, 7, 9, order)
    T, d = x.shape
    delta = 0.07
    u = x + np.sqrt(0.5 * delta) * rng.standard_normal(x.shape)
    ys, Hs, Rs, cs = model.observations_factory(x, u, delta)
    m0, P0, Fs, Qs, bs = model.dynamics_factory(x)
    assert Fs.shape == (T - 1, d, d) and Qs.shape == (T - 1, d, d) and bs.shape == (T - 1, d)
    npt.assert_array_equal(Fs[3], model.F)
    npt.assert_array_equal(Hs, np.broadcast_to(np.eye(d), (T, d, d)))
    npt.assert_array_equal(cs, 0.0)
    y, H, c = model.yobs, model.H, model.c
    for t in range(T):
        eta = H @ x[t] + c
        on = np.isfinite(y[t])
        e = np.where(on, np.exp(eta), 0.0)
        yy = np.where(on, y[t], 0.0)
        grad = H.T @ (yy - e)
        lam = H.T @ np.diag(e) @ H
        if order == 1:
            npt.assert_allclose(ys[t], u[t] + 0.5 * delta * grad, rtol=1e-13, atol=1e-14)
            npt.assert_allclose(Rs[t], 0.5 * delta * np.eye(d), rtol=1e-15)
        else:
            om = np.linalg.inv(lam + 2.0 / delta * np.eye(d))
            npt.assert_allclose(Rs[t], om, rtol=1e-12, atol=1e-15)
            npt.assert_array_equal(Rs[t], Rs[t].T)
            npt.assert_allclose(ys[t], om @ (2 * u[t] / delta + grad + lam @ x[t]), rtol=1e-12, atol=1e-14)
    want = K.prior_logpdf(x, (m0, P0, Fs, Qs, bs, None, None, None)) + sum(
        float(np.sum(np.where(np.isfinite(y[t]), np.nan_to_num(y[t]) * (H @ x[t] + c) - np.exp(H @ x[t] + c), 0.0))) for t in range(T))
    npt.assert_allclose(LC.oracle_target(model)(x), want, rtol=1e-13)


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("d", [1, 4])
def test_identity_loadings_give_poisson_model(order, d):
    """H = I, c = 0, dy = dx: the factories and the potential are PoissonModel's on the same data, missing counts included"""
    from aux_ssm_samplers_amd.kalman import PoissonLinearModel, PoissonModel
    from tests.kalman_poisson_cases import make_data
    T = 40
    y, path, (m0, P0, F, Q, b) = make_data(d, T, 11)
    assert np.isnan(y).any()
    lin = PoissonLinearModel(y, np.eye(d), 0.0, m0, P0, F, Q, b, order=order)
    pw = PoissonModel(y, m0, P0, F, Q, b, order=order)
    rng = np.random.default_rng(2)
    x = path + 0.1 * rng.standard_normal(path.shape)
    u = x + 0.1 * rng.standard_normal(path.shape)
    for a, bb in zip(lin.observations_factory(x, u, 0.05), pw.observations_factory(x, u, 0.05)):
        npt.assert_allclose(a, bb, rtol=1e-13, atol=1e-15)
    for a, bb in zip(lin.dynamics_factory(x), pw.dynamics_factory(x)):
        npt.assert_array_equal(a, bb)
    npt.assert_allclose(lin.log_potential(x), pw.log_potential(x), rtol=1e-13)
    npt.assert_allclose(LC.oracle_target(lin)(x), LC.oracle_target(pw)(x), rtol=1e-13)


@pytest.mark.parametrize("order", [1, 2])
def test_oracle_sweep_is_the_same_in_both_scan_forms(order):
    cell = LC._build(2, 7, 33, 1, order, 0)
    a, b = LC.oracle_chain(cell, 0, True), LC.oracle_chain(cell, 0, False)
    npt.assert_allclose(a["x_prop"], b["x_prop"], rtol=1e-9, atol=1e-10)
    for k in ("log_alpha", "lp_prop", "lp_rev", "lt_prop", "lt_rev"):
        npt.assert_allclose(a[k], b[k], rtol=1e-9, atol=1e-9)
    assert np.isfinite(a["log_alpha"])


def test_constructor_refusals():
    from aux_ssm_samplers_amd.kalman import PoissonLinearModel as M
    d, dy, T = 2, 3, 4
    y, H, c = np.ones((T, dy)), np.ones((dy, d)), np.zeros(dy)
    dyn = (np.zeros(d), np.eye(d), 0.9 * np.eye(d), np.eye(d), np.zeros(d))
    M(y, H, c, *dyn)
    assert M(y, H, 0.5, *dyn).c.shape == (dy,)                   # a scalar c is broadcast
    with pytest.raises(ValueError, match="order"):
        M(y, H, c, *dyn, order=3)
    with pytest.raises(ValueError, match=r"ys must be \(T, dy\)"):
        M(np.ones(T), H, c, *dyn)
    with pytest.raises(ValueError, match=r"H must be \(dy, dx\)"):
        M(y, np.ones((dy + 1, d)), c, *dyn)
    with pytest.raises(ValueError, match="finite"):
        M(y, np.where(np.eye(dy, d) > 0, np.nan, 1.0), c, *dyn)
    with pytest.raises(ValueError, match="c must be"):
        M(y, H, np.zeros(dy + 1), *dyn)
    with pytest.raises(ValueError, match="c must be"):
        M(y, H, np.full(dy, np.inf), *dyn)
    with pytest.raises(ValueError):
        M(np.where(np.eye(T, dy) > 0, -1.0, 1.0), H, c, *dyn)    # a negative count (PoissonPotential.check_counts)
    with pytest.raises(ValueError, match="m0, b must be"):
        M(y, H, c, np.zeros(d + 1), *dyn[1:])
    d5 = (np.zeros(5), np.eye(5), 0.9 * np.eye(5), np.eye(5), np.zeros(5))
    with pytest.raises((ValueError, NotImplementedError), match="<= 4"):
        M(y, np.ones((dy, 5)), c, *d5)
    with pytest.raises((ValueError, NotImplementedError), match="<= 1024"):
        M(np.ones((T, 1025)), np.ones((1025, d)), 0.0, *dyn)
    with pytest.raises((ValueError, NotImplementedError), match="1 <= dy"):
        M(np.ones((T, 0)), np.ones((0, d)), 0.0, *dyn)
    assert M.MAX_DY == 1024 and M.MAX_DX == 4 and M.dense_only


def test_get_kernel_recognises_the_model():
    from aux_ssm_samplers_amd import _lib
    from aux_ssm_samplers_amd.kalman import generic
    model, _, _ = small(order=2)
    assert (_lib.KMODEL_POISSON_LIN_FIRST, _lib.KMODEL_POISSON_LIN_SECOND) == (11, 12)
    assert model.kmodel == 12 and model.p_obs == 7
    assert generic._same_device_model(model.dynamics_factory, model.observations_factory, model.log_likelihood_fn) is model
    assert generic._same_device_model(model.dynamics_factory, lambda *a: model.observations_factory(*a), model.log_likelihood_fn) is None


def test_workload_recipe():
    from aux_ssm_samplers_amd.workloads import poisson_lin_setup
    model, x, H, c = poisson_lin_setup(400, 3, 40, seed=1, order=2)
    assert model.order == 2 and x.shape == (400, 3) and H.shape == (40, 3) and c.shape == (40,)
    assert np.abs(H).min() >= 0.1 and c.min() >= 0 and c.max() <= 2
    npt.assert_array_equal(np.diag(model.F), 0.9)
    assert model.F[0, 1] == 0.05 and model.F[1, 0] == -0.05 and not model.m0.any() and not model.b.any()
    npt.assert_array_equal(model.Q, 0.04 * np.eye(3))
    npt.assert_array_equal(model.P0, 0.2 * np.eye(3))
    y = model.yobs
    assert np.isfinite(y).all() and (y >= 0).all() and np.median(y) < 30


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("shape", LC.ONE_CHAIN_SHAPES + LC.CHAIN_SHAPES, ids=str)
def test_every_cell_builds_and_its_margins_hold(shape, order):
    dx, dy, T = shape[:3]
    Cn, every = (shape[3], shape[4]) if len(shape) == 5 else (1, 1)
    ref = LC.reference(dx, dy, T, Cn, order, True, every)
    cell, y = ref["cell"], ref["cell"]["model"].yobs
    assert (y == 0).any() and (T <= 3 or np.isnan(y).sum() == dy + 2)
    assert cell["delta"] <= (0.3 if T <= 3 else 0.05) and cell["delta"] * LC.lambda_max(cell["model"], LC.make_model(dx, dy, T, 100 * ref["attempt"] + 7 * dx + 3 * dy + T,
                                                                                                                    order)[1]) <= 1 + 1e-12
    la = ref["logs"][:, 0]
    assert np.all(la > LC.LOG_ALPHA_MIN) and np.all(np.isfinite(ref["logs"])) and ref["attempt"] < 3
    assert -13 < la.min() and la.max() < 16, (la.min(), la.max())
    for u, acc in zip(ref["us"], ref["accepted"]):
        margin = np.abs(np.minimum(la, 0.0) - np.log(u[ref["chains"]]))
        assert np.all(margin >= 0.05 - 1e-12)
        npt.assert_array_equal(acc, np.log(u[ref["chains"]]) < np.minimum(la, 0.0))
    if Cn > 1:
        assert ref["accepted"][0].any() and not ref["accepted"][0].all()
    else:
        assert len(ref["us"]) == 2 and ref["accepted"][0][0]     # one uniform on each side where the chain can be rejected at a margin
