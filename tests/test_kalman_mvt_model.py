"""kalman.MVTModel without a GPU: the NumPy factories against a literal restatement of examples/spatial/auxiliary_kalman.py:24-54 written here, the closed-form
gradient against central differences of tests/mvt_np.py::log_g, every validation error, which kernel kalman.get_kernel picks, and the conditions the case list of
tests/kalman_mvt_cases.py promises (with the oracle alone)."""
import numpy as np
import numpy.testing as npt
import pytest

from aux_ssm_samplers_amd.kalman import MVTModel, get_kernel
from aux_ssm_samplers_amd.kalman import generic
from aux_ssm_samplers_amd.workloads import spatial_precision, spatial_kalman_setup, spatial_setup
from oracle import kalman_np as K
from tests import kalman_mvt_cases as CS
from tests.mvt_np import log_g


def small(order, nu=3.0, nan=False, seed=0, T=5, grid=2):
    rng = np.random.default_rng(seed)
    d = grid * grid
    prec = spatial_precision(grid)
    y = rng.standard_normal((T, d))
    if nan:
        y[2, 1] = np.nan
    m0, b = 0.1 * rng.standard_normal((d, 1)), 0.05 * rng.standard_normal((d, 1))
    P0, F, Q = 0.5 + rng.random((d, 1, 1)), 0.9 + 0.1 * rng.random((d, 1, 1)), 0.5 + rng.random((d, 1, 1))
    return MVTModel(y, m0, P0, F, Q, b, nu, prec, order=order), dict(y=y, m0=m0, P0=P0, F=F, Q=Q, b=b, nu=nu, prec=prec, T=T, d=d), rng


def numeric_grad(x, y, nu, prec, h=1e-5):
    """central differences of sum_t log_g (the stand-in for jax.grad), (T, d)"""
    g = np.zeros_like(x)
    for t in range(x.shape[0]):
        for k in range(x.shape[1]):
            e = np.zeros(x.shape[1])
            e[k] = h
            g[t, k] = (log_g(x[t] + e, y[t], nu, prec) - log_g(x[t] - e, y[t], nu, prec)) / (2 * h)
    return g


def literal_factories(p, order):
    """auxiliary_kalman.py:16-54 line by line, with numeric_grad for jax.grad"""
    T, d, nu, prec, ys = p["T"], p["d"], p["nu"], p["prec"], p["y"]
    m0, P0, F, Q, b = p["m0"], p["P0"], p["F"], p["Q"], p["b"]
    prec_diag = prec[np.diag_indices(d)]
    eyes = np.ones((T, d, 1, 1))
    zeros = np.zeros((T, d, 1))

    def log_potential(xs):
        return np.sum(np.nan_to_num(log_g(xs, ys, nu, prec)))

    def dynamics_factory(_x):
        return m0, P0, np.tile(F[None, ...], (T - 1, 1, 1, 1)), np.tile(Q[None, ...], (T - 1, 1, 1, 1)), np.tile(b[None, ...], (T - 1, 1, 1))

    def grad(x):
        g = numeric_grad(x.reshape(-1, d), ys, nu, prec)
        g[np.isnan(ys).any(-1)] = np.nan   # jax.grad through the NaN: the whole row
        return g.reshape(T, d, 1)

    def first(x, u, delta):
        return u + 0.5 * delta * np.nan_to_num(grad(x)), eyes, 0.5 * delta * eyes, zeros

    def second(x, u, delta):
        hess = -nu * prec_diag / (nu - 2)
        Om = 1.0 / (-hess[None, ..., None, None] + 2 * eyes / delta)
        return Om[..., 0] * (2 * u / delta + grad(x) - hess[None, ..., None] * x), eyes, Om, zeros

    def log_likelihood_fn(x):
        lg = dynamics_factory(x)
        return K.prior_logpdf(x, lg + (None, None, None)) + log_potential(x.reshape(-1, d))

    return dynamics_factory, first if order == 1 else second, log_likelihood_fn


@pytest.mark.parametrize("nan", [False, True])
@pytest.mark.parametrize("order", [1, 2])
def test_factories_are_the_literal_restatement(order, nan):
    model, p, rng = small(order, nan=nan)
    T, d = p["T"], p["d"]
    x, u, delta = rng.standard_normal((T, d, 1)), rng.standard_normal((T, d, 1)), 0.3
    dyn, obs, llf = literal_factories(p, order)
    for got, want in zip(model.dynamics_factory(x), dyn(x)):
        assert got.shape == want.shape
        npt.assert_array_equal(got, want)
    got, want = model.observations_factory(x, u, delta), obs(x, u, delta)
    for g_, w_ in zip(got, want):
        assert g_.shape == w_.shape
    assert np.array_equal(np.isnan(got[0]), np.isnan(want[0]))
    if nan:
        assert np.isnan(got[0][2]).all() == (order == 2) and not np.isnan(np.delete(got[0], 2, axis=0)).any()   # order 2 keeps the gradient's NaN: the whole row
    npt.assert_allclose(got[0], want[0], rtol=1e-6, atol=1e-9, equal_nan=True)   # (the central differences' error)
    for g_, w_ in zip(got[1:], want[1:]):
        npt.assert_allclose(g_, w_, rtol=1e-15)
    npt.assert_allclose(model.log_likelihood_fn(x), llf(x), rtol=1e-13)
    npt.assert_allclose(model.log_likelihood_fn(x[..., 0]), llf(x), rtol=1e-13)


@pytest.mark.parametrize("nu", [1.0, 3.0])
def test_gradient_against_central_differences(nu):
    model, p, rng = small(1, nu=nu, nan=True, seed=3)
    x = rng.standard_normal((p["T"], p["d"]))
    g = model.grad_log_potential(x)
    assert np.isnan(g[2]).all()
    fin = np.arange(p["T"]) != 2
    want = numeric_grad(x, p["y"], nu, p["prec"])
    npt.assert_allclose(g[fin], want[fin], rtol=1e-6, atol=1e-6 * np.abs(want[fin]).max())


def test_log_likelihood_is_prior_plus_potential():
    model, p, rng = small(1, nan=True, seed=4)
    x = rng.standard_normal((p["T"], p["d"], 1))
    lg = model.dynamics_factory(x) + (None, None, None)
    pot = float(np.sum(np.nan_to_num(log_g(x[..., 0], p["y"], p["nu"], p["prec"]))))
    npt.assert_allclose(model.log_likelihood_fn(x), K.prior_logpdf(x, lg) + pot, rtol=1e-13)
    npt.assert_allclose(model.log_potential(x), pot, rtol=1e-13)


def test_validation_errors():
    _, p, _ = small(1)
    d, T = p["d"], p["T"]
    args = lambda **kw: {**dict(ys=p["y"], m0=p["m0"], P0=p["P0"], F=p["F"], Q=p["Q"], b=p["b"], nu=3.0, prec=p["prec"]), **kw}
    MVTModel(**args())
    MVTModel(**args(m0=p["m0"][:, 0], P0=p["P0"][:, 0, 0]))   # (d,) forms
    bad = p["prec"].copy()
    bad[0, 1] += 0.1
    with pytest.raises(ValueError, match="symmetric"):
        MVTModel(**args(prec=bad))
    with pytest.raises(ValueError, match="positive definite"):
        MVTModel(**args(prec=p["prec"] - 2 * np.eye(d)))
    with pytest.raises(ValueError, match="dense"):
        MVTModel(**args(prec=np.eye(d + 1)))
    for nu in (0.0, -1.0, np.inf):
        with pytest.raises(ValueError, match="nu"):
            MVTModel(**args(nu=nu))
    with pytest.raises(ValueError, match="nu == 2"):
        MVTModel(**args(nu=2.0), order=2)
    MVTModel(**args(nu=2.0), order=1)
    with pytest.raises(ValueError, match="order"):
        MVTModel(**args(), order=3)
    with pytest.raises(ValueError, match="64"):
        MVTModel(np.zeros((3, 65)), np.zeros(65), np.ones(65), np.ones(65), np.ones(65), np.zeros(65), 3.0, np.eye(65))
    MVTModel(np.zeros((3, 64)), np.zeros(64), np.ones(64), np.ones(64), np.ones(64), np.zeros(64), 3.0, np.eye(64))
    for name, val in (("m0", np.zeros(d + 1)), ("b", np.zeros((d, 2))), ("P0", np.ones((d, d))), ("F", np.ones((d, 1))), ("Q", np.ones(d - 1))):
        with pytest.raises(ValueError, match=name):
            MVTModel(**args(**{name: val}))
    with pytest.raises(ValueError, match=r"\(T, d\)"):
        MVTModel(**args(ys=p["y"][0]))
    # the order-2 step-size check: nu = 1 gives h_k = +prec_kk, so Omega_k^-1 = 2/delta - prec_kk
    m2 = MVTModel(**args(nu=1.0), order=2)
    m2.check_delta(1.9)
    with pytest.raises(ValueError, match="delta"):
        m2.check_delta(2.0)
    MVTModel(**args(nu=1.0), order=1).check_delta(100.0)
    MVTModel(**args(nu=3.0), order=2).check_delta(100.0)


def test_order2_delta_is_checked_before_the_device_is_touched(monkeypatch):
    model, p, rng = small(2, nu=1.0)
    monkeypatch.setattr(generic._lib, "default_handle", lambda *a: pytest.fail("the step size is checked first"))
    init, kernel = get_kernel(model.dynamics_factory, model.observations_factory, model.log_likelihood_fn, True)
    with pytest.raises(ValueError, match="delta"):
        kernel(None, init(np.zeros((p["T"], p["d"], 1))), 2.5)
    with pytest.raises(ValueError, match="state of shape"):
        kernel(None, init(np.zeros((p["T"] + 1, p["d"], 1))), 0.5)


def test_get_kernel_picks_the_device_kernel_for_the_bound_methods_only():
    model, *_ = small(1)
    assert generic._same_device_model(model.dynamics_factory, model.observations_factory, model.log_likelihood_fn) is model
    _, kernel = get_kernel(model.dynamics_factory, model.observations_factory, model.log_likelihood_fn, True)
    assert hasattr(kernel, "sweep") and hasattr(kernel, "draw")
    wrapped = (lambda x: model.dynamics_factory(x), lambda x, u, d: model.observations_factory(x, u, d), lambda x: model.log_likelihood_fn(x))
    assert generic._same_device_model(*wrapped) is None
    _, host = get_kernel(*wrapped, True)
    assert not hasattr(host, "sweep")
    other, *_ = small(1, seed=1)
    assert generic._same_device_model(model.dynamics_factory, other.observations_factory, model.log_likelihood_fn) is None
    assert model.dense_only and model.kmodel == generic._lib.KMODEL_MVT_FIRST and small(2)[0].kmodel == generic._lib.KMODEL_MVT_SECOND


def test_spatial_kalman_setup_is_the_recipe_of_spatial_setup():
    model, x0 = spatial_kalman_setup(6, 3, seed=5, nu=1.0, order=2)
    *_, x, y, prec = spatial_setup(6, 3, seed=5, nu=1.0)
    assert x0.shape == (6, 9, 1) and model.order == 2 and (model.T, model.dx) == (6, 9)
    npt.assert_array_equal(x0[..., 0], x)
    npt.assert_array_equal(model.yobs, y)
    npt.assert_array_equal(model.prec, prec)
    npt.assert_array_equal(model.Fv, np.ones(9))


def test_case_list_covers_every_value_and_keeps_its_margins():
    """every axis value of the issue occurs; and -- with the oracle alone -- every chain's margin |log alpha - log u_accept| is >= 1e-2 and each cell has accepted and
    rejected chains"""
    cols = list(zip(*CS.CELLS))
    assert set(cols[0]) == {1, 4, 9, 25, 33, 64} and set(cols[1]) == {2, 3, 70} and set(cols[2]) == {1, 3, 70}
    assert set(cols[3]) == {1, 2} and set(cols[4]) == {1.0, 3.0} and set(cols[5]) == {"grid", "dense"} and set(cols[6]) == {0.05, 0.5}
    assert {"t0_row", "mid_row", "last_row", "t0_comp", "mid_comp", "last_comp", None} <= set(cols[7]) and set(cols[8]) == {True, False}
    assert len(CS.CELLS) <= 26
    for i in range(len(CS.CELLS)):
        c, ref = CS.build(i), CS.reference(i)
        la = ref["logs"][:, 0]
        assert np.all(np.isfinite(ref["logs"])) and np.all(np.isfinite(ref["x_prop"])), CS.IDS[i]
        flags = np.concatenate(ref["accepted"])
        assert flags.any() and not flags.all(), (CS.IDS[i], la)
        for u, acc in zip(ref["us"], ref["accepted"]):
            assert np.all((u > 0) & (u < 1)), (CS.IDS[i], u)
            assert np.all(np.abs(np.minimum(la, 0.0) - np.log(u)) >= 1e-2), CS.IDS[i]
            npt.assert_array_equal(acc, np.log(u) < np.minimum(la, 0.0))
        if c["order"] == 2:
            c["model"].check_delta(c["delta"])
