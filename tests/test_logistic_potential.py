"""The logistic potential of the cSMC family (AUXSSM_POT_LOGISTIC, csmc.BinomialPotential / NegBinomialPotential) without a GPU: known answers, the NaN rule per
component, the closed-form gradient of the helpers (tests/logistic_np.py, tests/potential_np.py) against central differences, the kernels' softplus formula against np.logaddexp, the bound
of the forward pass's shift, validation at construction, the model description, the workload, the compilation of the potential as a user program (hipRTC needs
no device), the quadrature helper on cases with known answers, and the well-posedness of the exact ancestor comparisons tests/test_gpu_logistic.py makes."""
import numpy as np
import numpy.testing as npt
import pytest

from oracle import csmc_np as L
from tests import pit_cases as PC
from tests import logistic_np as LN
from tests import potential_np as P


def _sp(x):
    return np.log1p(np.exp(x))  # (small |x| only: the hand-made answers)


# ---- 1. known answers ------------------------------------------------------------------------------------------------------------------------------------
def test_known_answers_by_hand_and_the_nan_rule_per_component():
    from aux_ssm_samplers_amd.csmc import BinomialPotential, NegBinomialPotential
    log2 = np.log(2.0)
    bino = lambda x, y, n: BinomialPotential(n)(x, y)        # noqa: E731
    negb = lambda x, y, r: NegBinomialPotential(r)(x, y)     # noqa: E731
    # x = 0: softplus = log 2, so y * 0 - m log 2 whatever y
    for f in (LN.log_g, bino):
        assert abs(float(f(np.array([0.0]), [3.0], [5.0])) + 5 * log2) < 1e-15
        # binary data: y = 1 gives log sigma(x), y = 0 gives log(1 - sigma(x))
        assert abs(float(f(np.array([0.7]), [1.0], [1.0])) - np.log(1 / (1 + np.exp(-0.7)))) < 1e-15
        assert abs(float(f(np.array([0.7]), [0.0], [1.0])) - np.log(1 - 1 / (1 + np.exp(-0.7)))) < 1e-15
        # three components by hand
        want = (2 * 1.0 - 4 * _sp(1.0)) + (0 * -1.0 - 3 * _sp(-1.0)) + (6 * 0.5 - 6 * _sp(0.5))
        assert abs(float(f(np.array([1.0, -1.0, 0.5]), [2.0, 0.0, 6.0], [4.0, 3.0, 6.0])) - want) < 1e-14
        # the NaN rule is per component, whatever the size beside it; a row of NaN is flat
        want = (2 * 1.0 - 4 * _sp(1.0)) + (6 * 0.5 - 6 * _sp(0.5))
        assert abs(float(f(np.array([1.0, -1.0, 0.5]), [2.0, np.nan, 6.0], [4.0, np.nan, 6.0])) - want) < 1e-14
        assert float(f(np.array([1.0, -1.0, 0.5]), [np.nan] * 3, [4.0, 3.0, 6.0])) == 0.0
        # non-integers are the same formula
        assert abs(float(f(np.array([0.5]), [2.5], [3.5])) - (1.25 - 3.5 * _sp(0.5))) < 1e-15
    # the negative binomial's size is y + r: NB(r = 0.5) at y = 2, x = -0.3
    assert abs(float(negb(np.array([-0.3]), [2.0], 0.5)) - (2 * -0.3 - 2.5 * _sp(-0.3))) < 1e-15
    assert abs(float(negb(np.array([-0.3, 0.2]), [2.0, np.nan], [0.5, 7.0])) - (2 * -0.3 - 2.5 * _sp(-0.3))) < 1e-15
    # nothing overflows: softplus(800) = 800, softplus(-800) = 0
    assert float(LN.log_g(np.array([800.0]), [3.0], [5.0])) == 3 * 800.0 - 5 * 800.0
    assert float(bino(np.array([-800.0]), [3.0], 5.0)) == -2400.0
    # batched over particles
    x = np.random.default_rng(0).standard_normal((7, 3))
    y, n = np.array([1.0, np.nan, 6.0]), np.array([1.0, 4.0, 9.0])
    want = y[0] * x[:, 0] - n[0] * _sp(x[:, 0]) + y[2] * x[:, 2] - n[2] * _sp(x[:, 2])
    npt.assert_allclose(LN.log_g(x, y, n), want, rtol=0, atol=1e-14)
    npt.assert_allclose(BinomialPotential(n)(x, y), want, rtol=0, atol=1e-14)
    npt.assert_array_equal(LN.grad_log_g(x, y, n)[:, 1], np.zeros(7))
    # the protocol object's two roles
    ys, ms = np.array([[1.0, 2.0], [3.0, np.nan]]), np.array([[1.0, 5.0], [4.0, 0.0]])
    xx = np.array([[0.1, 0.2]])
    assert LN.potential(ys[0], ms[0], first=True)(xx)[0] == LN.log_g(xx, ys[0], ms[0])[0]
    assert LN.potential(ys[1:], ms[1:])(xx, None, np.concatenate([ys[1], ms[1]]))[0] == LN.log_g(xx, ys[1], ms[1])[0]


# ---- 2. gradients ----------------------------------------------------------------------------------------------------------------------------------------
def test_closed_form_gradient_equals_central_differences():
    rng = np.random.default_rng(3)
    for _ in range(6):
        x, n = 0.9 * rng.standard_normal(3), rng.integers(1, 41, 3).astype(float)
        y = rng.binomial(n.astype(int), 0.5).astype(float)
        y[rng.integers(3)] = np.nan if rng.random() < 0.5 else 0.0
        fd = L.grad_fd(lambda v: float(LN.log_g(v, y, n)), x)
        npt.assert_allclose(LN.grad_log_g(x, y, n), fd, rtol=0, atol=1e-6)


@pytest.mark.parametrize("family", LN.FAMILIES)
def test_joint_gradient_of_the_helper_equals_the_oracles_central_differences(family):
    """tests/potential_np.py::joint_grad replaces the central differences of oracle.csmc_np.get_independent_kernel(gradient=True): the same quantity"""
    rng = np.random.default_rng(4)
    for d in (1, 3):
        dev, m, x, _ = LN.case(d, 6, rng, family, nan_steps=(0, 3, 5))
        u = x + 0.3 * rng.standard_normal(x.shape)
        M0, G0, Mt, Gt = m.literal()
        fd = L.grad_fd(lambda v: float(L._log_pdf(v, M0, G0, Mt, Gt)), u)
        npt.assert_allclose(P.joint_grad(m, u), fd, rtol=0, atol=1e-5)


# ---- 3. the formula --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_softplus_formula_against_logaddexp(dtype):
    """softplus as the kernels form it -- e = exp(-|x|), l = log(1 + e), max(x, 0) + l, with no log1p -- against np.logaddexp(0, x) in extended precision over
    x in [-40, 40].  The bound, with eps = the ulp of 1: 1 + e is rounded first (an absolute eps / 2 in an argument >= 1, so at most eps / 2 in the logarithm); exp and
    log are each within an ulp of their results, e <= 1 and l <= log 2 (eps / 2 each); the final sum is rounded once (eps / 2 relative to the result):
    |error| <= 1.5 eps + (eps / 2) softplus(x).  An ABSOLUTE error of order eps where softplus itself is tiny (x << 0): the price of having no log1p, m eps / 2 in a
    log-weight of size m.  Measured with NumPy's exp and log: at most 1.15e-7 (fp32), 1.5e-16 (fp64) for x <= 0."""
    x = np.linspace(-40.0, 40.0, 160001).astype(dtype)
    got = LN.softplus_device_order(x, dtype).astype(np.longdouble)
    ref = np.logaddexp(np.longdouble(0), x.astype(np.longdouble))
    eps = np.longdouble(np.finfo(dtype).eps)
    err = np.abs(got - ref)
    neg = x <= 0
    print(f"{np.dtype(dtype).name}: max |softplus - logaddexp| = {float(err[neg].max()):.2e} for x <= 0, {float(err.max()):.2e} over [-40, 40]; "
          f"max relative to the bound {float((err / (1.5 * eps + 0.5 * eps * ref)).max()):.2f}")
    assert np.all(err <= 1.5 * eps + 0.5 * eps * ref)
    assert got.dtype == np.longdouble and LN.softplus_device_order(x, dtype).dtype == dtype
    # and the value never overflows or goes negative
    big = LN.softplus_device_order(np.array([-1e4, -100.0, 100.0, 1e4], dtype), dtype)
    npt.assert_array_equal(big, np.array([0.0, 0.0, 100.0, 1e4], dtype))


# ---- 4. the bound ------------------------------------------------------------------------------------------------------------------------------------------
def test_bound_dominates_the_potential_and_is_approached_at_logit_y_over_m():
    g = np.linspace(-30.0, 30.0, 3601)
    cases = (([0.0], [1.0]), ([1.0], [1.0]), ([7.0], [20.0]), ([2.5], [3.5]), ([0.0, 3.0], [4.0, 3.0]), ([4.0, np.nan], [9.0, 0.0]),
             ([np.nan, np.nan], [1.0, 1.0]), ([30.0, 1.0, 0.0], [40.0, 1.0, 0.5]))
    for y, m in cases:
        y, m = np.asarray(y), np.asarray(m)
        b = LN.bound(y, m)
        assert np.isfinite(b) and b <= 0
        grid = np.stack(np.meshgrid(*([g[::60]] * len(y)), indexing="ij"), axis=-1).reshape(-1, len(y)) if len(y) > 1 else g[:, None]
        assert np.all(LN.log_g(grid, y, m) <= b + 1e-12 * max(1.0, abs(b)))
        ok = np.isfinite(y)
        inner = ok & (y > 0) & (y < m)
        with np.errstate(divide="ignore", invalid="ignore"):
            xs = np.where(inner, np.log(y / (m - y)), np.where(ok & (y <= 0), -60.0, 60.0))  # logit(y / m); y = 0 and y = m are approached at -inf / +inf
        assert abs(float(LN.log_g(xs, y, m)) - b) <= 1e-12 * max(1.0, abs(b))
    assert LN.bound([0.0], [1.0]) == 0.0 and LN.bound([5.0], [5.0]) == 0.0 and LN.bound([np.nan], [3.0]) == 0.0
    assert abs(LN.bound([1.0], [2.0]) + 2 * np.log(2.0)) < 1e-15


# ---- 5. validation and description ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,msg", [(dict(trials=1.0, y=[2.0]), r"\[0, trials\]"), (dict(trials=3.0, y=[-1.0]), r"\[0, trials\]"),
                                    (dict(trials=0.0, y=[0.0]), "trials must be > 0"), (dict(trials=[1.0, -2.0], y=[np.nan, np.nan]), "trials must be > 0"),
                                    (dict(trials=np.nan, y=[0.0]), "trials must be finite"), (dict(trials=[[1.0, 2.0], [3.0, 0.5]], params=[[1.0, 2.0], [3.0, 1.0]]), r"\[0, trials\]"),
                                    (dict(trials=[1.0, 2.0, 3.0], y=[0.0, 1.0]), "must be a scalar")])
def test_binomial_construction_refusals(kw, msg):
    from aux_ssm_samplers_amd.csmc import BinomialPotential
    with pytest.raises(ValueError, match=msg):
        BinomialPotential(**kw)


@pytest.mark.parametrize("kw,msg", [(dict(r=1.0, y=[-1.0]), "counts must be >= 0"), (dict(r=0.0, y=[1.0]), "r must be > 0"), (dict(r=np.inf, y=[1.0]), "r must be finite"),
                                    (dict(r=[[1.0], [2.0], [3.0]], params=[[1.0], [2.0]]), "must be a scalar")])
def test_negbinomial_construction_refusals(kw, msg):
    from aux_ssm_samplers_amd.csmc import NegBinomialPotential
    with pytest.raises(ValueError, match=msg):
        NegBinomialPotential(**kw)


def test_construction_accepts_non_integers_zeros_and_missing_entries_and_shares_the_kalman_rules():
    from aux_ssm_samplers_amd import _logistic
    from aux_ssm_samplers_amd.csmc import BinomialPotential, NegBinomialPotential
    from aux_ssm_samplers_amd.kalman import BinomialModel, NegBinomialModel
    g0 = BinomialPotential([1.0, 3.5, 2.0], y=[0.0, 2.5, np.nan])
    npt.assert_array_equal(g0.sizes(), [[1.0, 3.5, 0.0]])  # 0 where the data is missing
    gt = BinomialPotential([[np.nan, 7.0, 1.0], [1.0, 1.0, 9.0]], params=[[np.nan, 7.0, 0.0], [0.0, 1.0, 7.25]])  # (a missing y: its trials may be anything)
    npt.assert_array_equal(gt.sizes(), [[0.0, 7.0, 1.0], [1.0, 1.0, 9.0]])
    nb = NegBinomialPotential(0.5, params=[[0.0, np.nan], [3.0, 1.5]])
    npt.assert_array_equal(nb.sizes(), [[0.5, 0.0], [3.5, 2.0]])
    # one set of rules: the same function raises for the Kalman models and for these potentials
    eye = np.eye(1)
    for make in (lambda: BinomialModel(np.array([[2.0]]), 1.0, np.zeros(1), eye, eye, eye, np.zeros(1)), lambda: BinomialPotential(1.0, y=[2.0])):
        with pytest.raises(ValueError, match=r"every observed y must lie in \[0, trials\]"):
            make()
    for make in (lambda: NegBinomialModel(np.array([[1.0]]), -1.0, np.zeros(1), eye, eye, eye, np.zeros(1)), lambda: NegBinomialPotential(-1.0, y=[1.0])):
        with pytest.raises(ValueError, match="r must be > 0"):
            make()
    assert callable(_logistic.binomial_size) and callable(_logistic.negbinomial_r)


@pytest.mark.parametrize("family", LN.FAMILIES)
def test_description_maps_to_kind_eight_with_two_planes(family):
    from aux_ssm_samplers_amd import _lib
    from aux_ssm_samplers_amd.csmc import _device, GaussianInit, LinearGaussianDynamics, SVPotential, PoissonPotential
    rng = np.random.default_rng(0)
    dev, m, x, _ = LN.case(3, 7, rng, family, nan_steps=(0, 3, 6))
    assert LN.has_every_feature(m)
    M0, G0, Mt, Gt = dev
    for fk in (_device.describe_independent(M0, G0, Mt, Gt, Mt), _device.describe_independent(M0, G0, Mt, Gt, Mt, _lib.GRAD_EXACT, True),
               _device.describe_bootstrap(M0, G0, Mt, Gt, Mt), _device.describe_guided(M0, G0, Mt, Gt, Mt, _lib.GRAD_REFERENCE)):
        assert fk.potential == _lib.POT_LOGISTIC == 8 and fk.user is None
        assert fk.y.shape == (2, 7, 3) and fk.prec is None and fk.obs_H is None
        npt.assert_array_equal(fk.y[0], m.y)
        npt.assert_array_equal(fk.y[1], m.size)
        assert np.isnan(fk.y[0, 0, 0]) and np.all(np.isnan(fk.y[0, 3])) and np.all(fk.y[1, 3] == 0) and np.all(np.isfinite(fk.y[1]))
    assert _lib.POT_POISSON == 6 and 7 not in [v for k, v in vars(_lib).items() if k.startswith("POT_")]  # 7 stays unassigned
    with pytest.raises(NotImplementedError):  # G0 and Gt must be the same potential
        _device.describe_independent(M0, SVPotential(y=G0.y), Mt, Gt, Mt)
    with pytest.raises(NotImplementedError):
        _device.describe_independent(M0, PoissonPotential(y=np.zeros(3)), Mt, Gt, Mt)
    with pytest.raises(ValueError):  # the state's dimension
        _device.describe_bootstrap(GaussianInit(m0=np.zeros(2), P0=np.eye(2)), G0, LinearGaussianDynamics(F=np.eye(2), b=np.zeros(2), Q=np.eye(2)), Gt, None)
    bad = type(G0)(1.0, y=np.zeros(3))
    bad.y = -np.ones(3)  # assigned after construction: caught when the model is described
    with pytest.raises(ValueError):
        _device.describe_independent(M0, bad, Mt, Gt, Mt)


@pytest.mark.parametrize("family", LN.FAMILIES)
def test_logistic_workload_is_the_kalman_workload(family):
    from aux_ssm_samplers_amd.csmc import BinomialPotential, NegBinomialPotential
    from aux_ssm_samplers_amd.workloads import logistic_setup, logistic_kalman_setup
    M0, Mt, G0, Gt, x, y, par = logistic_setup(300, 24, family, seed=1)
    assert x.shape == y.shape == (300, 24) and Gt.params.shape == (299, 24)
    assert isinstance(G0, BinomialPotential if family == "binomial" else NegBinomialPotential)
    npt.assert_array_equal(G0.y, y[0])
    npt.assert_array_equal(np.asarray(Mt.F), 0.9 * np.eye(24))
    assert np.all(y >= 0) and np.all(y == np.round(y))
    model, x0 = logistic_kalman_setup(300, 24, family, seed=1, order=2)  # both samplers see the same data
    npt.assert_array_equal(x0, x)
    npt.assert_array_equal(model.yobs, y)
    npt.assert_array_equal(model.size, np.concatenate([G0.sizes(), Gt.sizes()]))
    if family == "binomial":
        assert np.all(par[:, 0] == 1) and par.min() == 1 and par.max() == 40 and np.all(y <= par)
    else:
        assert par == 3.0 and y.max() > 8
    # one density on both sides
    assert abs(model.log_potential(x) - (float(G0(x[0], y[0])) + float(np.sum(Gt(x[1:], y[1:]))))) < 1e-9 * abs(model.log_potential(x))
    with pytest.raises(ValueError, match="family"):
        logistic_setup(10, 2, "poisson")


# ---- 6. the potential as a user program ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dx", [1, 2, 3, 4])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_potential_compiles_as_a_user_program(dtype, dx):
    from aux_ssm_samplers_amd import _lib
    from aux_ssm_samplers_amd.csmc import _device, device_models as U
    for flags in (_lib.FK_USER_POTENTIAL, _lib.FK_USER_POTENTIAL | _lib.FK_USER_GRADIENT):
        info = _device.program_info(_device.compile_program(U.BUILTIN_LOGISTIC, dtype, dx, flags))
        assert info == dict(dtype=_lib.dtype_code(dtype), dx=dx, flags=flags, has_bound=1)


# ---- 7. the quadrature helper ------------------------------------------------------------------------------------------------------------------------------
def test_quadrature_on_cases_with_known_answers():
    """no observation at all: the posterior is the Gaussian prior's marginals, known in closed form.  One step, y observed: against a direct one-dimensional
    quadrature on another grid."""
    m0, P0, F, Q, b = 0.3, 0.5, 0.8, 0.3, 0.1
    out = P.posterior_by_quadrature(LN.scalar_steps([np.nan] * 4, [0.0] * 4), m0, P0, F, Q, b)
    mu, var = m0, P0
    for t in range(4):
        if t:
            mu, var = F * mu + b, F * F * var + Q
        assert abs(out[t, 0] - mu) < 1e-9 and abs(out[t, 1] - var) < 1e-9
    g = np.linspace(-8.0, 8.0, 200001)
    w = np.exp(-0.5 * (g - m0) ** 2 / P0 + 3.0 * g - 5.0 * np.logaddexp(0.0, g))
    w /= w.sum()
    mean = float(w @ g)
    one = P.posterior_by_quadrature(LN.scalar_steps([3.0], [5.0]), m0, P0, F, Q, b)
    assert abs(one[0, 0] - mean) < 1e-9 and abs(one[0, 1] - float(w @ (g - mean) ** 2)) < 1e-9
    # and a later observation moves the earlier steps (the backward pass)
    two = P.posterior_by_quadrature(LN.scalar_steps([np.nan, 19.0], [0.0, 20.0]), m0, P0, F, Q, b)
    assert two[0, 0] > m0 + 0.1 and two[1, 0] > F * m0 + b + 0.3


# ---- 8. well-posedness of the exact ancestor comparisons ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", P.literal_cells(LN.KIND), ids=lambda c: f"{c[0]}-g{c[1]}-bw{int(c[2])}-d{c[3][0]}-N{c[3][1]}")
def test_exact_ancestor_comparison_is_well_posed(cell):
    """tests/test_gpu_logistic.py demands EQUAL ancestors of the device and the fp64 literal while their log-weights agree to 1e-10: fair only if no draw
    r = c[-1] (1 - u) lies within rounding of a cumulative-weight edge c[j].  From the literal sweep of every (cell, shape): the smallest |r - c[j]| over all
    resampling and backward draws is >= 1e-8 (weights normalised to sum 1); tests/potential_np.py::literal_sweep advances the seed until it holds, from the literal
    alone.  The data of every case hold a missing entry, a wholly missing row, y = 0 and a size of 1, and no size above 40."""
    (x, B, h), cs, gap, bump = P.literal_sweep(LN.KIND, *cell)
    print(cell, gap, bump)
    assert gap >= P.GAP_BAR and bump < P.MAX_BUMPS
    m = cs[4]
    T = cs[2]
    assert LN.has_every_feature(m)
    assert np.isnan(m.y[0, 0]) and np.all(np.isnan(m.y[T // 2])) and np.isnan(m.y[T - 1, 0])
    if cs[0] > 1:
        assert np.isfinite(m.y[0, 1:]).all() and np.isfinite(m.y[T - 1, -1])  # rows that are partly NaN


def test_both_families_go_through_every_group_and_binomial_data_reach_y_equal_trials():
    for group in (LN.REGISTER, LN.WIDE, LN.PIT_CELLS):
        assert {LN.family_of(s) for s in group} == set(LN.FAMILIES)
    for shape in LN.REGISTER + LN.WIDE:
        m = P.literal_sweep(LN.KIND, "independent", False, False, shape)[1][4]
        if LN.family_of(shape) == "binomial":
            ok = np.isfinite(m.y)
            assert (m.y[ok] == m.size[ok]).any() and (m.size[ok] == 1).any()


@pytest.mark.parametrize("style,gradient,backward", P.LITERAL_CELLS + P.BOOTSTRAP_CELLS)
def test_every_literal_cell_moves_the_trajectory_somewhere(style, gradient, backward):
    moved = sum(int((P.literal_sweep(LN.KIND, style, gradient, backward, shape)[0][1] != 0).sum()) for shape in LN.REGISTER + LN.WIDE)
    print(style, gradient, backward, moved)
    assert moved > 0


@pytest.mark.parametrize("gradient", [False, True])
@pytest.mark.parametrize("d,N,T", LN.PIT_CELLS)
def test_tree_comparison_is_well_posed(d, N, T, gradient):
    """the smallest draw margin of the literal tree is at least tests/pit_cases.py::margin_threshold(N), and the sweep moves the trajectory"""
    c, (xl, origins, hist) = P.pit_literal(LN.KIND, (d, N, T), gradient)
    print(d, N, T, gradient, hist["min_margin"], int((origins != 0).sum()))
    assert hist["min_margin"] >= PC.margin_threshold(N)
    assert (origins != 0).any()
    assert LN.has_every_feature(c.m)
    assert np.isnan(c.m.y[0, 0]) and np.all(np.isnan(c.m.y[PC.top_boundary(T)]))
