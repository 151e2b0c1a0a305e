"""kalman.BinomialLinearModel and kalman.NegBinomialLinearModel on the CPU: gradient and Lam against central differences of log_potential, both factories
against their defining formulas, the reduction to BinomialModel / NegBinomialModel at H = I, c = 0, every refusal of the constructors, finiteness at |eta| = 200
in float32, the a-priori curvature bound Lam <= H' diag(m / 4) H, which kernel kalman.get_kernel picks, the workload recipe, and the conditions
tests/kalman_logistic_lin_cases.py promises (with the oracle alone), the range of the oracle's log alpha among them."""
import numpy as np
import numpy.testing as npt
import pytest

from oracle import kalman_np as K
from tests import kalman_logistic_lin_cases as LC


def small(family, dx=3, dy=7, T=9, order=1, seed=3):
    model, path, _ = LC.make_model(family, dx, dy, T, seed, order)
    rng = np.random.default_rng(seed)
    return model, path + 0.1 * rng.standard_normal(path.shape), rng


def formulas(model, x_t, t):
    """(value, grad, Lam) of step t straight from the issue's formulas, channel by channel"""
    y, H, c = model.yobs[t], model.H, model.c
    val, grad, lam = 0.0, np.zeros(H.shape[1]), np.zeros((H.shape[1],) * 2)
    for j in range(H.shape[0]):
        if not np.isfinite(y[j]):
            continue
        eta = H[j] @ x_t + c[j]
        m = model.size_s[j] + model.size_w[j] * y[j]
        e = np.exp(-abs(eta))
        r = 1.0 / (1.0 + e)
        sig = r if eta >= 0 else e * r
        val += y[j] * eta - m * (max(eta, 0.0) + np.log1p(e))
        grad += H[j] * (y[j] - m * sig)
        lam += m * (e * r) * r * np.outer(H[j], H[j])
    return val, grad, lam


@pytest.mark.parametrize("family", LC.FAMILIES)
@pytest.mark.parametrize("dx,dy", [(1, 3), (2, 7), (4, 65)])
def test_grad_and_lam_are_the_derivatives_of_log_potential(family, dx, dy):
    model, x, _ = small(family, dx, dy)
    assert np.isnan(model.yobs).any()
    grad, lam = model.grad_lam(x)
    h = 1e-5
    for t in (0, 3, 8):
        for k in range(dx):
            xp, xm = x.copy(), x.copy()
            xp[t, k] += h
            xm[t, k] -= h
            fd = (model.log_potential(xp) - model.log_potential(xm)) / (2 * h)
            npt.assert_allclose(grad[t, k], fd, rtol=1e-6, atol=1e-6 * max(1.0, np.abs(grad[t]).max()))
            gd = (model.grad_lam(xp)[0][t] - model.grad_lam(xm)[0][t]) / (2 * h)    # d grad / d x_k = column k of the Hessian = -Lam
            npt.assert_allclose(-lam[t, :, k], gd, rtol=1e-6, atol=1e-6 * max(1.0, np.abs(lam[t]).max()))
    npt.assert_array_equal(lam, np.swapaxes(lam, 1, 2))
    assert np.all(np.linalg.eigvalsh(lam) > -1e-12 * np.abs(lam).max())
    npt.assert_array_equal(grad[4], 0.0)   # the wholly missing row T // 2: no term at all
    npt.assert_array_equal(lam[4], 0.0)


@pytest.mark.parametrize("family", LC.FAMILIES)
@pytest.mark.parametrize("order", [1, 2])
def test_factories_are_their_formulas(family, order):
    model, x, rng = small(family, 3, 7, 9, order)
    T, d = x.shape
    delta = 0.07
    u = x + np.sqrt(0.5 * delta) * rng.standard_normal(x.shape)
    ys, Hs, Rs, cs = model.observations_factory(x, u, delta)
    m0, P0, Fs, Qs, bs = model.dynamics_factory(x)
    assert Fs.shape == (T - 1, d, d) and Qs.shape == (T - 1, d, d) and bs.shape == (T - 1, d)
    npt.assert_array_equal(Fs[3], model.F)
    npt.assert_array_equal(Hs, np.broadcast_to(np.eye(d), (T, d, d)))
    npt.assert_array_equal(cs, 0.0)
    total = 0.0
    for t in range(T):
        val, grad, lam = formulas(model, x[t], t)
        total += val
        if order == 1:
            npt.assert_allclose(ys[t], u[t] + 0.5 * delta * grad, rtol=1e-13, atol=1e-13)
            npt.assert_allclose(Rs[t], 0.5 * delta * np.eye(d), rtol=1e-15)
        else:
            om = np.linalg.inv(lam + 2.0 / delta * np.eye(d))
            npt.assert_allclose(Rs[t], om, rtol=1e-12, atol=1e-15)
            npt.assert_array_equal(Rs[t], Rs[t].T)
            npt.assert_allclose(ys[t], om @ (2 * u[t] / delta + grad + lam @ x[t]), rtol=1e-12, atol=1e-13)
    npt.assert_allclose(model.log_potential(x), total, rtol=1e-13)
    want = K.prior_logpdf(x, (m0, P0, Fs, Qs, bs, None, None, None)) + total
    npt.assert_allclose(LC.oracle_target(model)(x), want, rtol=1e-13)
    # the size: s + w y, the binomial's trials whatever y is, the negative binomial's y + r
    yy = np.where(np.isfinite(model.yobs), model.yobs, 0.0)
    npt.assert_array_equal(model.size, model.trials + 0.0 * yy if family == "binomial" else model.r + yy)


@pytest.mark.parametrize("family", LC.FAMILIES)
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("d", [1, 4])
def test_identity_loadings_give_the_pointwise_models(family, order, d):
    """H = I, c = 0, dy = dx: the factories and the potential are BinomialModel's / NegBinomialModel's on the same data (sizes per component, as the linear
    models take them), missing entries included"""
    from aux_ssm_samplers_amd import kalman
    from tests import kalman_logistic_cases as PC
    T = 40
    y, par, path, _, (m0, P0, F, Q, b) = PC.make_data(family, d, T, 11)
    par = np.where(np.isfinite(par), par, 1.0).max(axis=0)          # one size per component: the largest of the cell's
    y = np.minimum(y, par) if family == "binomial" else y
    assert np.isnan(y).any()
    lin_cls, pw_cls = ((kalman.BinomialLinearModel, kalman.BinomialModel) if family == "binomial" else (kalman.NegBinomialLinearModel, kalman.NegBinomialModel))
    lin = lin_cls(y, par, np.eye(d), 0.0, m0, P0, F, Q, b, order=order)
    pw = pw_cls(y, par, m0, P0, F, Q, b, order=order)
    rng = np.random.default_rng(2)
    x = path + 0.1 * rng.standard_normal(path.shape)
    u = x + 0.1 * rng.standard_normal(path.shape)
    for a, bb in zip(lin.observations_factory(x, u, 0.05), pw.observations_factory(x, u, 0.05)):
        npt.assert_allclose(a, bb, rtol=1e-13, atol=1e-15)
    for a, bb in zip(lin.dynamics_factory(x), pw.dynamics_factory(x)):
        npt.assert_array_equal(a, bb)
    npt.assert_allclose(lin.log_potential(x), pw.log_potential(x), rtol=1e-13)
    npt.assert_allclose(LC.oracle_target(lin)(x), LC.oracle_target(pw)(x), rtol=1e-13)


def test_constructor_refusals():
    from aux_ssm_samplers_amd.kalman import BinomialLinearModel as B, NegBinomialLinearModel as N
    d, dy, T = 2, 3, 4
    y, H, c = np.ones((T, dy)), np.ones((dy, d)), np.zeros(dy)
    dyn = (np.zeros(d), np.eye(d), 0.9 * np.eye(d), np.eye(d), np.zeros(d))
    d5 = (np.zeros(5), np.eye(5), 0.9 * np.eye(5), np.eye(5), np.zeros(5))
    for M, par, who in ((B, 3.0, "BinomialLinearModel"), (N, 0.5, "NegBinomialLinearModel")):
        M(y, par, H, c, *dyn)
        M(y, np.full(dy, par), H, c, *dyn)                                  # one size per channel
        assert M(y, par, H, 0.5, *dyn).c.shape == (dy,)                     # a scalar c is broadcast
        with pytest.raises(NotImplementedError, match=r"\(T, dy\) size.*133 of the 160 KB of LDS"):
            M(y, np.full((T, dy), par), H, c, *dyn)
        with pytest.raises(ValueError, match="order"):
            M(y, par, H, c, *dyn, order=3)
        with pytest.raises(ValueError, match=who + r": ys must be \(T, dy\)"):
            M(np.ones(T), par, H, c, *dyn)
        with pytest.raises(ValueError, match=who + r": H must be \(dy, dx\)"):
            M(y, par, np.ones((dy + 1, d)), c, *dyn)
        with pytest.raises(ValueError, match=who + ": H must be finite"):
            M(y, par, np.where(np.eye(dy, d) > 0, np.nan, 1.0), c, *dyn)
        with pytest.raises(ValueError, match=who + ": H must be finite"):
            M(y, par, np.where(np.eye(dy, d) > 0, np.inf, 1.0), c, *dyn)
        with pytest.raises(ValueError, match="c must be"):
            M(y, par, H, np.zeros(dy + 1), *dyn)
        with pytest.raises(ValueError, match="c must be"):
            M(y, par, H, np.full(dy, np.inf), *dyn)
        with pytest.raises(ValueError, match="c must be"):
            M(y, par, H, np.nan, *dyn)
        with pytest.raises(ValueError):
            M(np.where(np.eye(T, dy) > 0, -1.0, 1.0), par, H, c, *dyn)      # a negative y
        with pytest.raises(ValueError, match="> 0"):
            M(y, 0.0, H, c, *dyn)                                           # trials / r <= 0
        with pytest.raises(ValueError, match="> 0"):
            M(y, np.array([par, -1.0, par]), H, c, *dyn)
        with pytest.raises(ValueError, match="must be a scalar"):
            M(y, np.full(dy + 1, par), H, c, *dyn)
        with pytest.raises(ValueError, match="m0, b must be"):
            M(y, par, H, c, np.zeros(d + 1), *dyn[1:])
        with pytest.raises(NotImplementedError, match="<= 4"):
            M(y, par, np.ones((dy, 5)), c, *d5)
        with pytest.raises(NotImplementedError, match="<= 1024"):
            M(np.ones((T, 1025)), par, np.ones((1025, d)), 0.0, *dyn)
        with pytest.raises(NotImplementedError, match="1 <= dy"):
            M(np.ones((T, 0)), par, np.ones((0, d)), 0.0, *dyn)
        assert M.MAX_DY == 1024 and M.MAX_DX == 4 and M.dense_only
    with pytest.raises(ValueError, match=r"\[0, trials\]"):
        B(np.where(np.eye(T, dy) > 0, 4.0, 1.0), 3.0, H, c, *dyn)           # y above trials
    N(np.where(np.eye(T, dy) > 0, 400.0, 1.0), 0.5, H, c, *dyn)             # counts above r are what the negative binomial is for
    B(np.where(np.eye(T, dy) > 0, np.nan, 1.0), 3.0, H, c, *dyn)            # a missing entry is data


@pytest.mark.parametrize("family", LC.FAMILIES)
def test_everything_is_finite_at_eta_200_in_float32(family):
    """|eta| = 200 on either side, in float32: exp(200) overflows there, exp(-|eta|) does not.  Value, gradient, Lam and both factories stay finite, and the
    saturated forms are exact: sigma = 1 / 0, the curvature 0."""
    model, x, rng = small(family, 2, 7, 9, 2)
    for sign in (1.0, -1.0):
        h = model.H[0]
        xs = x.copy()
        xs[3] += ((sign * 200.0 - (xs[3] @ h + model.c[0])) / (h @ h)) * h
        xs = xs.astype(np.float32)
        assert abs(float(xs[3] @ h.astype(np.float32) + np.float32(model.c[0]))) > 199.0
        with np.errstate(over="raise", invalid="raise"):
            val = model.log_potential(xs)
            grad, lam = model.grad_lam(xs)
            out = model.observations_factory(xs, xs + np.float32(0.1), 0.05)
        assert grad.dtype == np.float32 and lam.dtype == np.float32
        assert np.isfinite(val) and np.isfinite(grad).all() and np.isfinite(lam).all() and all(np.isfinite(a).all() for a in out)
        assert np.all(np.linalg.eigvalsh(lam.astype(np.float64)) > -1e-5 * np.abs(lam).max())


@pytest.mark.parametrize("family", LC.FAMILIES)
@pytest.mark.parametrize("dx,dy", [(1, 3), (3, 5), (4, 65)])
def test_curvature_is_bounded_a_priori(family, dx, dy):
    """Lam_t <= H' diag(m_t / 4) H at every x (sigma (1 - sigma) <= 1/4): the smallest eigenvalue of the difference is >= 0, at the path, far from it and at
    eta = 0, where the bound is attained.  So delta = first_order_delta() has delta lambda_max(Lam_t) <= 1 wherever the chain is."""
    model, x, rng = small(family, dx, dy, 9)
    m = np.where(np.isfinite(model.yobs), model.size, 0.0)
    bound = np.einsum("tj,jk,jl->tkl", 0.25 * m, model.H, model.H)
    delta = model.first_order_delta()
    npt.assert_allclose(delta, 4.0 / np.max(np.linalg.eigvalsh(4.0 * bound)), rtol=1e-12)
    for z in (x, x + 3.0 * rng.standard_normal(x.shape), 0.0 * x):
        lam = model.grad_lam(z)[1]
        gap = np.linalg.eigvalsh(bound - lam)
        assert gap.min() >= -1e-12 * np.abs(bound).max(), gap.min()
        assert delta * np.max(np.linalg.eigvalsh(lam)) <= 1.0 + 1e-12
    zero_c = type(model)(model.yobs, model.trials if family == "binomial" else model.r, model.H, 0.0, model.m0, model.P0, model.F, model.Q, model.b)
    npt.assert_allclose(zero_c.grad_lam(0.0 * x)[1], bound, rtol=1e-13, atol=1e-15)     # attained at eta = 0


@pytest.mark.parametrize("family", LC.FAMILIES)
def test_get_kernel_recognises_the_model(family):
    from aux_ssm_samplers_amd import _lib, kalman
    from aux_ssm_samplers_amd.kalman import generic
    model, _, _ = small(family, order=2)
    assert (_lib.KMODEL_LOGISTIC_LIN_FIRST, _lib.KMODEL_LOGISTIC_LIN_SECOND) == (15, 16)
    assert "BinomialLinearModel" in kalman.__all__ and "NegBinomialLinearModel" in kalman.__all__
    assert model.kmodel == 16 and model.p_obs == 7 and model.dx == 3
    assert generic._same_device_model(model.dynamics_factory, model.observations_factory, model.log_likelihood_fn) is model
    assert generic._same_device_model(model.dynamics_factory, lambda *a: model.observations_factory(*a), model.log_likelihood_fn) is None


@pytest.mark.parametrize("family", LC.FAMILIES)
def test_workload_recipe(family):
    from aux_ssm_samplers_amd import kalman
    from aux_ssm_samplers_amd.workloads import logistic_lin_setup
    model, x, H, c, par = logistic_lin_setup(400, 3, 40, family, seed=1, order=2)
    assert isinstance(model, kalman.BinomialLinearModel if family == "binomial" else kalman.NegBinomialLinearModel)
    assert model.order == 2 and x.shape == (400, 3) and H.shape == (40, 3) and c.shape == (40,)
    assert np.abs(H).min() >= 0.1 and c.min() >= -1 and c.max() <= 1
    npt.assert_array_equal(np.diag(model.F), 0.9)
    assert model.F[0, 1] == 0.05 and model.F[1, 0] == -0.05 and not model.m0.any() and not model.b.any()
    npt.assert_array_equal(model.Q, 0.04 * np.eye(3))
    npt.assert_array_equal(model.P0, 0.2 * np.eye(3))
    y = model.yobs
    assert np.isfinite(y).all() and (y >= 0).all()
    if family == "binomial":
        assert par.shape == (40,) and par[0] == 1 and par.min() >= 1 and par.max() <= 40 and np.all(y <= par) and set(np.unique(y[:, 0])) == {0.0, 1.0}
    else:
        assert par == 3.0 and y.max() > 3
    with pytest.raises(ValueError, match="family"):
        logistic_lin_setup(10, 2, 3, "poisson")


@pytest.mark.parametrize("family", LC.FAMILIES)
@pytest.mark.parametrize("order", [1, 2])
def test_oracle_sweep_is_the_same_in_both_scan_forms(family, order):
    cell = LC._build(family, 2, 7, 33, 1, order, 0)
    a, b = LC.oracle_chain(cell, 0, True), LC.oracle_chain(cell, 0, False)
    npt.assert_allclose(a["x_prop"], b["x_prop"], rtol=1e-9, atol=1e-10)
    for k in ("lp_prop", "lp_rev", "lt_prop", "lt_rev"):
        npt.assert_allclose(a[k], b[k], rtol=1e-9)
    assert np.isfinite(a["log_alpha"]) and abs(a["log_alpha"] - b["log_alpha"]) < 1e-9 * max(abs(a[k]) for k in ("lp_prop", "lp_rev", "lt_prop", "lt_rev"))


@pytest.mark.parametrize("family", LC.FAMILIES)
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("shape", LC.ONE_CHAIN_SHAPES + LC.CHAIN_SHAPES, ids=str)
def test_every_cell_builds_and_its_margins_hold(family, shape, order):
    """What the cases module promises of every cell: its special entries, its step size, the saturated start, the oracle's log alpha in a moderate range
    (-45 .. +80 over all cells; asserted here), and the placed uniforms' margins."""
    dx, dy, T = shape[:3]
    Cn, every = (shape[3], shape[4]) if len(shape) == 5 else (1, 1)
    ref = LC.reference(family, dx, dy, T, Cn, order, True, every)
    cell, model = ref["cell"], ref["cell"]["model"]
    y, m = model.yobs, model.size
    ts, ks = cell["sat"]
    assert (y == 0).any() and np.nanmax(np.where(np.isfinite(y), m, np.nan)) >= 1000
    if family == "binomial":
        assert (y == model.trials).any() and model.trials.max() >= 1000 and (dy == 1 or model.trials[0] == 1)
    if dy > 1:
        assert np.isnan(y[T // 2]).all() and np.isnan(y[0]).sum() == 1 and np.isnan(y).sum() == dy + (2 if T > 3 else 1)
    eta0 = cell["x"][::3, ts] @ model.H[ks] + model.c[ks]
    assert np.all(np.abs(eta0) >= LC.ETA_SAT - 1e-9) and np.all(np.sign(eta0) == (1 if family == "binomial" else -1))
    assert cell["delta"] == min(0.3, model.first_order_delta())
    lam_path = model.grad_lam(cell["x"][0])[1]
    assert cell["delta"] * np.max(np.linalg.eigvalsh(lam_path)) <= 1 + 1e-12
    la = ref["logs"][:, 0]
    assert np.all(np.isfinite(ref["logs"])) and ref["attempt"] < 8
    assert -45 < la.min() and la.max() < LC.LOG_ALPHA_MAX, (la.min(), la.max())
    for u, acc in zip(ref["us"], ref["accepted"]):
        margin = np.abs(np.minimum(la, 0.0) - np.log(u[ref["chains"]]))
        assert np.all(margin >= 0.05 - 1e-12)
        npt.assert_array_equal(acc, np.log(u[ref["chains"]]) < np.minimum(la, 0.0))
    if Cn > 1:
        assert ref["accepted"][0].any() and not ref["accepted"][0].all()
    else:
        assert len(ref["us"]) == 2 and ref["accepted"][0][0]     # one uniform on each side where the chain can be rejected at a margin


@pytest.mark.parametrize("name", sorted(LC.QUAD))
def test_quadrature_grids_have_converged(name):
    """The ground truth of tests/test_gpu_kalman_logistic_lin.py's posterior test: refining each grid (101 -> 201 points per axis in 3-D, 41 -> 61 in 4-D) moves
    no posterior mean or variance by more than 1e-6 relative, and the moments are those of a proper posterior near the prior's."""
    coarse, fine = LC.quad_exact(name)
    npt.assert_allclose(coarse, fine, rtol=1e-6, atol=1e-9)
    q = LC.QUAD[name]
    assert fine.shape == (q["y"].shape[0] * q["H"].shape[1], 2) and np.all(fine[:, 1] > 0.05) and np.all(fine[:, 1] < 0.4) and np.all(np.abs(fine[:, 0]) < 1)
    assert np.isnan(q["y"]).sum() == (1 if name == "scalar" else 0) and (name != "scalar" or set(np.unique(q["y"][np.isfinite(q["y"])])) == {0.0, 1.0})
