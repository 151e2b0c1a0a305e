"""The Poisson count potential of the cSMC family (AUXSSM_POT_POISSON, csmc.PoissonPotential) without a GPU: known answers, the NaN rule per component, the
closed-form gradient of the helpers (tests/poisson_np.py, tests/potential_np.py) against central differences, the bound of the forward pass's shift, validation at construction, the model
description, the compilation of the potential as a user program (hipRTC needs no device), the quadrature helper on a case solved by hand, and the well-posedness
of the exact ancestor comparisons tests/test_gpu_poisson.py makes."""
import numpy as np
import numpy.testing as npt
import pytest

from oracle import csmc_np as L
from tests import pit_cases as PC
from tests import poisson_np as PN
from tests import potential_np as P


# ---- 1. known answers ------------------------------------------------------------------------------------------------------------------------------------
def test_known_answers_by_hand_zero_counts_and_the_nan_rule_per_component():
    from aux_ssm_samplers_amd.csmc import PoissonPotential
    pot = PoissonPotential()
    # x = 0: y * 0 - e^0 = -1 whatever the count;  x = log 2, y = 3: 3 log 2 - 2
    for f in (PN.log_g, pot):
        assert float(f(np.array([0.0]), [5.0])) == -1.0
        assert abs(float(f(np.array([np.log(2.0)]), [3.0])) - (3 * np.log(2.0) - 2.0)) < 1e-15
        # y = 0: the term is -e^x, not 0 -- a zero count is an observation
        assert abs(float(f(np.array([1.0]), [0.0])) + np.e) < 1e-15
        # three components by hand: (2 * 1 - e) + (0 * -1 - e^-1) + (4 * 0 - 1)
        assert abs(float(f(np.array([1.0, -1.0, 0.0]), [2.0, 0.0, 4.0])) - (2.0 - np.e - np.exp(-1.0) - 1.0)) < 1e-15
        # the NaN rule is per component: a missing y_k drops term k alone; a row of NaN is flat
        assert abs(float(f(np.array([1.0, -1.0, 0.0]), [2.0, np.nan, 4.0])) - (2.0 - np.e - 1.0)) < 1e-15
        assert float(f(np.array([1.0, -1.0, 0.0]), [np.nan] * 3)) == 0.0
        # non-integer counts are the same formula
        assert abs(float(f(np.array([0.5]), [2.5])) - (1.25 - np.exp(0.5))) < 1e-15
    # batched over particles
    x = np.random.default_rng(0).standard_normal((7, 3))
    y = np.array([1.0, np.nan, 6.0])
    want = y[0] * x[:, 0] - np.exp(x[:, 0]) + y[2] * x[:, 2] - np.exp(x[:, 2])
    npt.assert_allclose(PN.log_g(x, y), want, rtol=0, atol=1e-14)
    npt.assert_allclose(pot(x, y), want, rtol=0, atol=1e-14)
    # the gradient's NaN rule
    npt.assert_array_equal(PN.grad_log_g(x, y)[:, 1], np.zeros(7))
    # the protocol object's two roles
    ys = np.array([[1.0, 2.0], [3.0, np.nan]])
    xx = np.array([[0.1, 0.2]])
    assert PN.potential(ys[0], first=True)(xx)[0] == PN.log_g(xx, ys[0])[0]
    assert PN.potential(ys[1:])(xx, None, ys[1])[0] == PN.log_g(xx, ys[1])[0]


# ---- 2. gradients ----------------------------------------------------------------------------------------------------------------------------------------
def test_closed_form_gradient_equals_central_differences():
    rng = np.random.default_rng(3)
    for _ in range(5):
        x, y = 1.0 + 0.7 * rng.standard_normal(3), rng.poisson(3.0, 3).astype(float)
        y[rng.integers(3)] = np.nan if rng.random() < 0.5 else 0.0
        fd = L.grad_fd(lambda v: float(PN.log_g(v, y)), x)
        npt.assert_allclose(PN.grad_log_g(x, y), fd, rtol=0, atol=1e-6)


def test_joint_gradient_of_the_helper_equals_the_oracles_central_differences():
    """tests/potential_np.py::joint_grad replaces the central differences of oracle.csmc_np.get_independent_kernel(gradient=True): the same quantity"""
    rng = np.random.default_rng(4)
    for d in (1, 3):
        dev, m, x, _ = PN.case(d, 6, rng, nan_steps=(0, 3, 5))
        u = x + 0.3 * rng.standard_normal(x.shape)
        M0, G0, Mt, Gt = m.literal()
        fd = L.grad_fd(lambda v: float(L._log_pdf(v, M0, G0, Mt, Gt)), u)
        npt.assert_allclose(P.joint_grad(m, u), fd, rtol=0, atol=1e-5)


# ---- 3. the bound ------------------------------------------------------------------------------------------------------------------------------------------
def test_bound_dominates_the_potential_and_is_attained_at_log_y():
    g = np.linspace(-12.0, 6.0, 3601)
    for y in ([0.0], [1.0], [7.0], [2.5], [0.0, 3.0], [4.0, np.nan], [np.nan, np.nan], [30.0, 1.0, 0.0]):
        y = np.asarray(y)
        b = PN.bound(y)
        assert np.isfinite(b)
        grid = np.stack(np.meshgrid(*([g[::60]] * len(y)), indexing="ij"), axis=-1).reshape(-1, len(y)) if len(y) > 1 else g[:, None]
        assert np.all(PN.log_g(grid, y) <= b + 1e-12 * max(1.0, abs(b)))
        pos = np.isfinite(y) & (y > 0)
        xs = np.where(pos, np.log(np.where(pos, y, 1.0)), -50.0)  # x_k = log y_k; y_k = 0 is approached as x_k -> -inf; a missing component is free
        assert abs(float(PN.log_g(xs, y)) - b) <= 1e-12 * max(1.0, abs(b))
    assert PN.bound([0.0]) == 0.0 and PN.bound([np.nan]) == 0.0 and PN.bound([1.0]) == -1.0


# ---- 4. validation and description ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(y=[-1.0]), dict(y=[2.0, -0.5]), dict(params=[[1.0, 2.0], [3.0, -1e-9]]), dict(y=[np.nan, -3.0])])
def test_construction_refuses_negative_counts(kw):
    from aux_ssm_samplers_amd.csmc import PoissonPotential
    with pytest.raises(ValueError, match="counts must be >= 0"):
        PoissonPotential(**kw)


def test_construction_accepts_non_integers_zeros_and_missing_entries():
    from aux_ssm_samplers_amd.csmc import PoissonPotential
    PoissonPotential(y=[0.0, 2.5, np.nan], params=[[np.nan, np.nan, np.nan], [0.0, 1.0, 7.25]])


def test_description_maps_to_kind_six():
    from aux_ssm_samplers_amd import _lib
    from aux_ssm_samplers_amd.csmc import _device, GaussianInit, LinearGaussianDynamics, PoissonPotential, SVPotential
    rng = np.random.default_rng(0)
    dev, m, x, _ = PN.case(3, 5, rng, nan_steps=(0, 2, 4))
    M0, G0, Mt, Gt = dev
    for fk in (_device.describe_independent(M0, G0, Mt, Gt, Mt), _device.describe_independent(M0, G0, Mt, Gt, Mt, _lib.GRAD_EXACT, True),
               _device.describe_bootstrap(M0, G0, Mt, Gt, Mt), _device.describe_guided(M0, G0, Mt, Gt, Mt, _lib.GRAD_REFERENCE)):
        assert fk.potential == _lib.POT_POISSON == 6 and fk.user is None
        assert fk.y.shape == (5, 3) and fk.prec is None and fk.obs_H is None
        npt.assert_array_equal(fk.y, m.y)
        assert np.isnan(fk.y[0, 0]) and np.all(np.isnan(fk.y[2])) and np.all(np.isnan(fk.y[4, :2])) and np.isfinite(fk.y[4, 2])
    with pytest.raises(NotImplementedError):  # G0 and Gt must be the same potential
        _device.describe_independent(M0, SVPotential(y=G0.y), Mt, Gt, Mt)
    with pytest.raises(ValueError):  # the state's dimension
        _device.describe_bootstrap(GaussianInit(m0=np.zeros(2), P0=np.eye(2)), G0, LinearGaussianDynamics(F=np.eye(2), b=np.zeros(2), Q=np.eye(2)), Gt, None)
    bad = PoissonPotential(y=G0.y)
    bad.y = -np.ones(3)  # assigned after construction: caught when the model is described
    with pytest.raises(ValueError, match="counts must be >= 0"):
        _device.describe_independent(M0, bad, Mt, Gt, Mt)


def test_poisson_workload():
    from aux_ssm_samplers_amd.csmc import PoissonPotential
    from aux_ssm_samplers_amd.workloads import poisson_setup
    M0, Mt, G0, Gt, x, y = poisson_setup(400, 24, seed=1)
    assert x.shape == y.shape == (400, 24) and Gt.params.shape == (399, 24) and isinstance(G0, PoissonPotential)
    F = np.asarray(Mt.F)
    assert np.max(np.abs(np.linalg.eigvals(F))) < 1 and np.all(F[np.abs(np.subtract.outer(np.arange(24), np.arange(24))) > 1] == 0) and F[0, 1] != 0
    npt.assert_allclose(np.linalg.solve(np.eye(24) - F, Mt.b), np.ones(24), rtol=0, atol=1e-12)  # the stationary mean is 1
    assert abs(x.mean() - 1.0) < 0.1 and np.all(y >= 0) and np.all(y == np.round(y)) and np.mean(y <= 30) > 0.999 and y.max() > 8
    npt.assert_array_equal(G0.y, y[0])


# ---- 5. the potential as a user program ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dx", [1, 2, 3, 4])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_potential_compiles_as_a_user_program(dtype, dx):
    from aux_ssm_samplers_amd import _lib
    from aux_ssm_samplers_amd.csmc import _device, device_models as U
    for flags in (_lib.FK_USER_POTENTIAL, _lib.FK_USER_POTENTIAL | _lib.FK_USER_GRADIENT):
        info = _device.program_info(_device.compile_program(U.BUILTIN_POISSON, dtype, dx, flags))
        assert info == dict(dtype=_lib.dtype_code(dtype), dx=dx, flags=flags, has_bound=1)


# ---- 6. the quadrature helper ------------------------------------------------------------------------------------------------------------------------------
def test_quadrature_on_cases_with_known_answers():
    """no observation at all: the posterior is the Gaussian prior's marginals, known in closed form.  One step, y observed: against a direct one-dimensional
    quadrature on another grid."""
    m0, P0, F, Q, b = 0.7, 0.5, 0.8, 0.3, 0.1
    out = P.posterior_by_quadrature(PN.scalar_steps([np.nan] * 4), m0, P0, F, Q, b)
    mu, var = m0, P0
    for t in range(4):
        if t:
            mu, var = F * mu + b, F * F * var + Q
        assert abs(out[t, 0] - mu) < 1e-9 and abs(out[t, 1] - var) < 1e-9
    g = np.linspace(-8.0, 8.0, 200001)
    w = np.exp(-0.5 * (g - m0) ** 2 / P0 + 3.0 * g - np.exp(g))
    w /= w.sum()
    mean = float(w @ g)
    one = P.posterior_by_quadrature(PN.scalar_steps([3.0]), m0, P0, F, Q, b)
    assert abs(one[0, 0] - mean) < 1e-9 and abs(one[0, 1] - float(w @ (g - mean) ** 2)) < 1e-9
    # and a later observation moves the earlier steps (the backward pass)
    two = P.posterior_by_quadrature(PN.scalar_steps([np.nan, 9.0]), m0, P0, F, Q, b)
    assert two[0, 0] > m0 + 0.1 and two[1, 0] > F * m0 + b + 0.3


# ---- 7. well-posedness of the exact ancestor comparisons ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", P.literal_cells(PN.KIND), ids=lambda c: f"{c[0]}-g{c[1]}-bw{int(c[2])}-d{c[3][0]}-N{c[3][1]}")
def test_exact_ancestor_comparison_is_well_posed(cell):
    """tests/test_gpu_poisson.py demands EQUAL ancestors of the device and the fp64 literal while their log-weights agree to 1e-10: fair only if no draw
    r = c[-1] (1 - u) lies within rounding of a cumulative-weight edge c[j].  From the literal sweep of every (cell, shape): the smallest |r - c[j]| over all
    resampling and backward draws is >= 1e-8 (weights normalised to sum 1; the bar of tests/test_lingauss_potential.py); tests/potential_np.py::literal_sweep
    advances the seed until it holds, from the literal alone."""
    (x, B, h), cs, gap, bump = P.literal_sweep(PN.KIND, *cell)
    print(cell, gap, bump)
    assert gap >= 1e-8
    m = cs[4]
    T = cs[2]
    assert np.isnan(m.y[0, 0]) and np.all(np.isnan(m.y[T // 2])) and np.isnan(m.y[T - 1, 0])
    if cs[0] > 1:
        assert np.isfinite(m.y[0, 1:]).all() and np.isfinite(m.y[T - 1, -1])  # rows that are partly NaN


@pytest.mark.parametrize("style,gradient,backward", P.LITERAL_CELLS + P.BOOTSTRAP_CELLS)
def test_every_literal_cell_moves_the_trajectory_somewhere(style, gradient, backward):
    moved = sum(int((P.literal_sweep(PN.KIND, style, gradient, backward, shape)[0][1] != 0).sum()) for shape in PN.REGISTER + PN.WIDE)
    print(style, gradient, backward, moved)
    assert moved > 0


@pytest.mark.parametrize("gradient", [False, True])
@pytest.mark.parametrize("d,N,T", PN.PIT_CELLS)
def test_tree_comparison_is_well_posed(d, N, T, gradient):
    """the smallest draw margin of the literal tree is at least tests/pit_cases.py::margin_threshold(N), and the sweep moves the trajectory"""
    c, (xl, origins, hist) = P.pit_literal(PN.KIND, (d, N, T), gradient)
    print(d, N, T, gradient, hist["min_margin"], int((origins != 0).sum()))
    assert hist["min_margin"] >= PC.margin_threshold(N)
    assert (origins != 0).any()
    assert np.isnan(c.m.y[0, 0]) and np.all(np.isnan(c.m.y[PC.top_boundary(T)]))
