"""kalman.PoissonModel on the CPU: construction, the NumPy factories against finite differences of the potential, the agreement with csmc.PoissonPotential, and
the oracle's sweep driven by the factories on data with missing counts.  The device sweep is tests/test_gpu_kalman_poisson.py's."""
import numpy as np
import numpy.testing as npt
import pytest

from oracle import kalman_np as K
from tests import kalman_poisson_cases as PC


def _model(T=7, d=3, order=1, seed=2, nan=True):
    from aux_ssm_samplers_amd.kalman import PoissonModel
    y, path, (m0, P0, F, Q, b) = PC.make_data(d, T, seed)
    if not nan:
        y = np.nan_to_num(y, nan=3.0)
    return PoissonModel(y, m0, P0, F, Q, b, order=order), path


def test_construction_and_validation():
    from aux_ssm_samplers_amd import _lib
    from aux_ssm_samplers_amd.kalman import PoissonModel
    from aux_ssm_samplers_amd.workloads import poisson_kalman_setup
    y, path, (m0, P0, F, Q, b) = PC.make_data(2, 5, 0)
    for order, kind in ((1, _lib.KMODEL_POISSON_FIRST), (2, _lib.KMODEL_POISSON_SECOND)):
        m = PoissonModel(y, m0, P0, F, Q, b, order=order)
        assert (m.kmodel, m.dense_only, m.T, m.dx, m.p_obs) == (kind, False, 5, 2, 2)
    assert (_lib.KMODEL_POISSON_FIRST, _lib.KMODEL_POISSON_SECOND) == (7, 8)
    with pytest.raises(ValueError):
        PoissonModel(y, m0, P0, F, Q, b, order=3)
    bad = y.copy()
    bad[1, 1] = -1.0
    with pytest.raises(ValueError):
        PoissonModel(bad, m0, P0, F, Q, b)
    with pytest.raises(ValueError):
        PoissonModel(y[:, 0], m0, P0, F, Q, b)          # ys must be (T, dx)
    PoissonModel(np.where(np.isnan(y), np.nan, y + 0.5), m0, P0, F, Q, b)   # non-integer counts >= 0 and NaN are accepted
    model, x0 = poisson_kalman_setup(12, 3, seed=1, order=2)
    assert isinstance(model, PoissonModel) and model.order == 2 and x0.shape == (12, 3) and model.yobs.shape == (12, 3)
    from aux_ssm_samplers_amd.workloads import poisson_setup
    M0, Mt, _, _, xs, ys = poisson_setup(12, 3, seed=1)
    npt.assert_array_equal(model.yobs, ys)
    npt.assert_array_equal(x0, xs)
    npt.assert_array_equal(model.Q, Mt.Q)


def test_get_kernel_recognises_the_device_model():
    from aux_ssm_samplers_amd.kalman import generic
    model, _ = _model()
    assert generic._same_device_model(model.dynamics_factory, model.observations_factory, model.log_likelihood_fn) is model
    assert generic._same_device_model(lambda z: model.dynamics_factory(z), model.observations_factory, model.log_likelihood_fn) is None


def test_grad_and_lam_against_finite_differences_of_log_potential():
    model, path = _model(order=2)
    rng = np.random.default_rng(0)
    x = path + 0.1 * rng.standard_normal(path.shape)
    grad, lam = model.grad_lam(x)
    h = 1e-4
    for t, k in np.ndindex(*x.shape):
        e = np.zeros_like(x)
        e[t, k] = h
        fp, f0, fm = model.log_potential(x + e), model.log_potential(x), model.log_potential(x - e)
        # central differences of y x - e^x: errors e^x h^2 / 6 and e^x h^2 / 12, plus rounding of sums of size ~|f| (<= 1e3) over h and h^2
        npt.assert_allclose((fp - fm) / (2 * h), grad[t, k], atol=1e-6 + 1e-6 * np.exp(x[t, k]))
        npt.assert_allclose(-(fp - 2 * f0 + fm) / h ** 2, lam[t, k], atol=1e-3 + 1e-6 * np.exp(x[t, k]))
    miss = ~np.isfinite(model.yobs)
    assert miss.any() and np.all(grad[miss] == 0) and np.all(lam[miss] == 0) and np.all(lam[~miss] > 0)


def test_factories_follow_the_specification():
    rng = np.random.default_rng(3)
    for order in (1, 2):
        model, path = _model(order=order)
        T, d = path.shape
        x, u, delta = path + 0.1 * rng.standard_normal((T, d)), path + 0.2 * rng.standard_normal((T, d)), 0.37
        mask, e = np.isfinite(model.yobs), np.exp(x)
        grad, lam = np.where(mask, np.nan_to_num(model.yobs) - e, 0.0), np.where(mask, e, 0.0)
        ys, Hs, Rs, cs = model.observations_factory(x, u, delta)
        npt.assert_array_equal(Hs, np.broadcast_to(np.eye(d), (T, d, d)))
        npt.assert_array_equal(cs, np.zeros((T, d)))
        if order == 1:
            npt.assert_allclose(ys, u + 0.5 * delta * grad, rtol=1e-15)
            npt.assert_allclose(Rs, np.broadcast_to(0.5 * delta * np.eye(d), (T, d, d)), rtol=1e-15)
        else:
            om = 1.0 / (lam + 2.0 / delta)
            npt.assert_allclose(ys, om * (2 * u / delta + grad + lam * x), rtol=1e-14)
            npt.assert_allclose(Rs, om[..., None] * np.eye(d), rtol=1e-15)
        assert np.all(np.isfinite(ys)) and np.all(np.isfinite(Rs))     # a missing count never makes a pseudo-observation NaN
        # a missing component is observed through u alone, with variance delta / 2, in both orders
        npt.assert_allclose(ys[~mask], u[~mask], rtol=1e-15)
        npt.assert_allclose(np.einsum("tkk->tk", Rs)[~mask], 0.5 * delta, rtol=1e-15)
        m0, P0, Fs, Qs, bs = model.dynamics_factory(x)
        assert Fs.shape == (T - 1, d, d) and Qs.shape == (T - 1, d, d) and bs.shape == (T - 1, d)
        npt.assert_array_equal(Fs[3], model.F)
        npt.assert_array_equal(Qs[0], model.Q)


def test_second_order_with_zero_curvature_equals_first_order():
    from aux_ssm_samplers_amd.kalman import PoissonModel
    y, path, (m0, P0, F, Q, b) = PC.make_data(3, 6, 1)
    y = np.full_like(y, np.nan)     # lam = 0 everywhere
    rng = np.random.default_rng(4)
    x, u = path + 0.1 * rng.standard_normal(path.shape), path + 0.3 * rng.standard_normal(path.shape)
    o1 = PoissonModel(y, m0, P0, F, Q, b, order=1).observations_factory(x, u, 0.21)
    o2 = PoissonModel(y, m0, P0, F, Q, b, order=2).observations_factory(x, u, 0.21)
    for a, bb in zip(o1, o2):
        npt.assert_allclose(a, bb, rtol=1e-15, atol=0)


def test_log_potential_equals_the_csmc_potential_summed_over_time():
    from aux_ssm_samplers_amd.csmc import PoissonPotential
    model, path = _model(T=9, d=4)
    x = path + 0.2 * np.random.default_rng(5).standard_normal(path.shape)
    assert np.isnan(model.yobs).any()
    want = float(np.sum(PoissonPotential()(x, model.yobs)))
    npt.assert_allclose(model.log_potential(x), want, rtol=1e-14)
    # log_likelihood_fn = prior + potential, on the oracle's own prior density
    lg = (model.m0, model.P0, model.Fs, model.Qs, model.bs, None, None, None)
    npt.assert_allclose(PC.oracle_target(model)(x), K.prior_logpdf(x, lg) + want, rtol=1e-14)


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("parallel", [True, False])
def test_oracle_sweep_runs_on_missing_counts(order, parallel):
    ref = PC.reference(4, 150, 1, order, parallel)
    cell = ref["cell"]
    assert np.isnan(cell["model"].yobs).sum() == 4 + 2 and (cell["model"].yobs == 0).any() and np.nanmax(cell["model"].yobs) > 100
    assert np.all(np.isfinite(ref["logs"])) and np.all(np.isfinite(ref["x_prop"]))
    assert np.abs(ref["x_prop"] - cell["x"]).max() > 1e-3
    # both scan forms of the oracle agree
    other = PC.reference(4, 150, 1, order, not parallel)
    npt.assert_allclose(ref["x_prop"], other["x_prop"], rtol=1e-9, atol=1e-10)
    npt.assert_allclose(ref["logs"], other["logs"], rtol=1e-6, atol=1e-7)
    # one chain: one sweep with each outcome, unless log alpha leaves no room for a rejection
    acc = [bool(a[0]) for a in ref["accepted"]]
    assert acc[0] is True and (acc[1] is False or ref["logs"][0, 0] >= -PC.MARGIN_MIN)


def test_placed_uniforms_keep_their_margins():
    la = np.array([-30.0, -0.6, -0.2, -0.01, 0.0, 3.0, -5.0])
    us, acc = PC.place_uniforms(la)
    margin = np.abs(np.log(us[0]) - np.minimum(la, 0.0))
    assert np.all(margin >= PC.MARGIN_MIN - 1e-12)
    npt.assert_array_equal(acc[0], [False, True, False, True, True, True, True])
