"""The linear-Gaussian observation potential of the cSMC family (AUXSSM_POT_LIN_GAUSS, csmc.LinearGaussianPotential) without a GPU: known answers, the whitening
identity the device's residual form rests on, the closed-form gradient of the helpers (tests/lingauss_np.py, tests/potential_np.py) against central differences, validation at
construction, the model description, the compilation of the potential as a user program (hipRTC needs no device), and the well-posedness of the exact
ancestor comparison tests/test_gpu_lingauss.py makes."""
import numpy as np
import numpy.testing as npt
import pytest

from oracle import csmc_np as L
from tests import lingauss_np as LG
from tests import potential_np as P

HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)


# ---- 1. known answers ------------------------------------------------------------------------------------------------------------------------------------
def test_scalar_and_isotropic_known_answers_and_nan_rule():
    from aux_ssm_samplers_amd.csmc import LinearGaussianPotential
    sig, y = 0.7, 0.4
    x = np.array([[-1.3], [0.4], [2.5], [10.0]])
    want = -0.5 * ((y - x[:, 0]) / sig) ** 2 - np.log(sig) - HALF_LOG_2PI
    npt.assert_allclose(LG.log_g(x, [y], [[1.0]], [[sig * sig]], [0.0]), want, rtol=0, atol=1e-13)
    npt.assert_allclose(LinearGaussianPotential(H=[[1.0]], R=[[sig * sig]])(x, [y]), want, rtol=0, atol=1e-13)
    assert abs(want[1] - (-np.log(0.7) - HALF_LOG_2PI)) < 1e-15
    # H = I, R = sig^2 I: the sum of scalar Gaussians
    rng = np.random.default_rng(1)
    x3, y3 = rng.standard_normal((6, 3)), rng.standard_normal(3)
    want3 = np.sum(-0.5 * ((y3 - x3) / sig) ** 2 - np.log(sig) - HALF_LOG_2PI, axis=1)
    npt.assert_allclose(LG.log_g(x3, y3, np.eye(3), sig * sig * np.eye(3), np.zeros(3)), want3, rtol=0, atol=1e-13)
    npt.assert_allclose(LinearGaussianPotential(H=np.eye(3), R=sig * sig * np.eye(3))(x3, y3), want3, rtol=0, atol=1e-13)
    # two observed mixtures of three components with an offset, by hand: H x + c = (1.5, 0.5) + (0.5, 0.5) = (2, 1), y = (1, 2), r = (-1, 1), R = [[2, 1], [1, 2]]:
    # r' R^-1 r = (2 + 2 + 2) / 3 = 2, log det R = log 3
    H, R, c = np.array([[1.0, 1.0, 0.5], [0.0, -1.0, 0.5]]), np.array([[2.0, 1.0], [1.0, 2.0]]), np.array([0.5, 0.5])
    xh = np.array([1.0, 0.0, 1.0])
    byhand = -1.0 - 0.5 * np.log(3.0) - 2 * HALF_LOG_2PI
    assert abs(LG.log_g(xh, [1.0, 2.0], H, R, c) - byhand) < 1e-14
    assert abs(float(LinearGaussianPotential(H=H, R=R, c=c)(xh, [1.0, 2.0])) - byhand) < 1e-14
    # the NaN rule: any NaN component makes the whole step flat, value and gradient
    assert np.all(LG.log_g(x3, [0.5, np.nan, 0.1], np.eye(3), np.eye(3), np.zeros(3)) == 0)
    assert np.all(LG.grad_log_g(x3, [0.5, np.nan, 0.1], np.eye(3), np.eye(3), np.zeros(3)) == 0)
    assert np.all(LinearGaussianPotential(H=H, R=R, c=c)(x3, [np.nan, 1.0]) == 0)
    assert LG.log_g(xh, [np.nan, 1.0], H, R, c) == 0


# ---- 2. the whitening identity ---------------------------------------------------------------------------------------------------------------------------
def contract_log_g(x, yw_t, Hw, c_lin):
    """c_lin - |yw_t - Hw x|^2 / 2 in the order of include/auxssm.h (kind 5), NumPy float64, one particle per row of x: a_k accumulated over j ascending from 0
    (NumPy float64 has no fused multiply-add: each fma is a product and a sum, two roundings -- far inside the bar), z_k = yw_k - a_k, q over k ascending"""
    n, d = x.shape
    z = np.zeros((n, d))
    for k in range(d):
        a = np.zeros(n)
        for j in range(d):
            a = Hw[k, j] * x[:, j] + a
        z[:, k] = yw_t[k] - a
    q = np.zeros(n)
    for k in range(d):
        q = z[:, k] * z[:, k] + q
    v = c_lin - 0.5 * q
    return np.where(np.isnan(v), 0.0, v)


def _whitening_error(dev, m, xs):
    """max over the steps and the particles xs (T, N, d) of |contract order on the package's whitened quantities - the helper's unwhitened formula|"""
    M0, G0, Mt, Gt = dev
    Hw, yw, c_lin = Gt.whitened(m.y)
    assert Hw.shape == (G0.dx, G0.dx) and yw.shape == (m.y.shape[0], G0.dx) and np.all(Hw[G0.dy:] == 0)
    assert np.array_equal(np.isnan(yw).all(axis=1), np.isnan(m.y).any(axis=1)) and np.all(yw[~np.isnan(yw).any(axis=1), G0.dy:] == 0)
    err = 0.0
    with np.errstate(invalid="ignore"):
        for t in range(m.y.shape[0]):
            err = max(err, float(np.max(np.abs(contract_log_g(xs[t], yw[t], Hw, c_lin) - LG.log_g(xs[t], m.y[t], m.H, m.R, m.c)))))
    return err


def test_whitened_residual_form_equals_the_unwhitened_formula_on_every_gpu_case():
    """every particle of every case of tests/test_gpu_lingauss.py's lists (the literal sweeps' own particle systems; the program shapes' start trajectories and a
    cloud around them): within 1e-11 absolute, a decade inside the GPU file's 1e-10 on log-weights"""
    worst = 0.0
    for cell in P.literal_cells(LG.KIND):
        (x, B, h), (d, N, T, dev, m, x0, delta, nz), _, _ = P.literal_sweep(LG.KIND, *cell)
        worst = max(worst, _whitening_error(dev, m, h["xs"]))
    for d, dy, N, T, Cn in LG.PROGRAM_SHAPES:
        rng = np.random.default_rng(100 * d + N)
        dev, m, xtrue, delta = LG.case(d, dy, T, rng, nan_rows=(3, T - 2))
        worst = max(worst, _whitening_error(dev, m, xtrue[:, None, :] + 0.6 * rng.standard_normal((T, 32, d))))
    print(f"worst |whitened contract order - unwhitened solve| = {worst:.2e}")
    assert worst <= 1e-11


# ---- 3. gradients ----------------------------------------------------------------------------------------------------------------------------------------
def test_closed_form_gradient_equals_central_differences():
    rng = np.random.default_rng(3)
    H, R, c = LG.observation(3, 2, rng)
    for _ in range(5):
        x, y = rng.standard_normal(3), rng.standard_normal(2)
        fd = L.grad_fd(lambda v: float(LG.log_g(v, y, H, R, c)), x)
        npt.assert_allclose(LG.grad_log_g(x, y, H, R, c), fd, rtol=0, atol=1e-6)


def test_joint_gradient_of_the_helper_equals_the_oracles_central_differences():
    """tests/potential_np.py::joint_grad replaces the central differences of oracle.csmc_np.get_independent_kernel(gradient=True): the same quantity"""
    rng = np.random.default_rng(4)
    for d, dy in ((2, 1), (3, 3)):
        dev, m, x, _ = LG.case(d, dy, 6, rng, nan_rows=(3,))
        u = x + 0.3 * rng.standard_normal(x.shape)
        M0, G0, Mt, Gt = m.literal()
        fd = L.grad_fd(lambda v: float(L._log_pdf(v, M0, G0, Mt, Gt)), u)
        npt.assert_allclose(P.joint_grad(m, u), fd, rtol=0, atol=1e-6)


def test_exact_posterior_of_the_helper_on_a_model_solved_by_hand():
    """T = 2, d = 1: prior N(0, 1), x_1 = x_0 + N(0, 1), y_t = x_t + N(0, 1) observed at t = 1 only (y_0 NaN).  Joint precision [[2, -1], [-1, 2]], h = (0, y_1):
    mean = (y_1 / 3, 2 y_1 / 3), covariance = [[2, 1], [1, 2]] / 3"""
    dev, m = LG.build(np.zeros(1), np.eye(1), np.eye(1), np.zeros(1), np.eye(1), np.eye(1), np.eye(1), np.zeros(1), np.array([[np.nan], [1.5]]))
    mean, cov = LG.exact_posterior(m)
    npt.assert_allclose(mean, [0.5, 1.0], rtol=0, atol=1e-14)
    npt.assert_allclose(cov, np.array([[2.0, 1.0], [1.0, 2.0]]) / 3, rtol=0, atol=1e-14)


# ---- 4. validation and description ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(H=np.eye(2), R=[[1.0, 0.5], [0.0, 1.0]]),            # R not symmetric
                                dict(H=np.eye(2), R=[[1.0, 2.0], [2.0, 1.0]]),            # R indefinite
                                dict(H=np.eye(2), R=np.eye(3)),                           # R of another size
                                dict(H=np.eye(2), R=[[1.0, np.nan], [np.nan, 1.0]]),
                                dict(H=[[1.0, np.inf]], R=[[1.0]]),
                                dict(H=np.ones(3), R=[[1.0]]),                            # H not a matrix
                                dict(H=None, R=[[1.0]]), dict(H=np.eye(2), R=None),
                                dict(H=np.eye(2), R=np.eye(2), c=np.zeros(3)),
                                dict(H=np.eye(2), R=np.eye(2), c=[0.0, np.nan]),
                                dict(H=np.ones((1, 2)), R=[[1.0]], y=np.zeros(2)),        # y of the state's, not the observation's dimension
                                dict(H=np.ones((2, 3)), R=np.eye(2), params=np.zeros((5, 3))),
                                dict(H=np.ones((1, 33)), R=[[1.0]])])                      # dx beyond the kernels
def test_validation_at_construction(kw):
    from aux_ssm_samplers_amd.csmc import LinearGaussianPotential
    with pytest.raises(ValueError):
        LinearGaussianPotential(**kw)


def test_more_observations_than_state_components_are_not_implemented():
    from aux_ssm_samplers_amd.csmc import LinearGaussianPotential
    with pytest.raises(NotImplementedError, match="dy = 3 > dx = 2"):
        LinearGaussianPotential(H=np.ones((3, 2)), R=np.eye(3))


def test_description_maps_to_kind_five():
    from aux_ssm_samplers_amd import _lib
    from aux_ssm_samplers_amd.csmc import _device, GaussianInit, LinearGaussianDynamics, LinearGaussianPotential
    rng = np.random.default_rng(0)
    dev, m, x, _ = LG.case(3, 2, 5, rng, nan_rows=(2,))
    M0, G0, Mt, Gt = dev
    Lr = np.linalg.cholesky(m.R)
    Hw = np.zeros((3, 3))
    Hw[:2] = np.linalg.solve(Lr, m.H)
    c_lin = -np.sum(np.log(np.diag(Lr))) - 2 * HALF_LOG_2PI
    for fk in (_device.describe_independent(M0, G0, Mt, Gt, Mt), _device.describe_independent(M0, G0, Mt, Gt, Mt, _lib.GRAD_EXACT, True),
               _device.describe_bootstrap(M0, G0, Mt, Gt, Mt), _device.describe_guided(M0, G0, Mt, Gt, Mt, _lib.GRAD_REFERENCE)):
        assert fk.potential == _lib.POT_LIN_GAUSS == 5 and fk.user is None
        npt.assert_allclose(fk.obs_H, Hw, rtol=0, atol=1e-15)
        assert fk.obs_H.shape == (3, 3) and fk.obs_H.flags.c_contiguous and np.all(fk.obs_H[2] == 0) and abs(fk.obs_const - c_lin) < 1e-15
        assert fk.y.shape == (5, 3) and np.all(np.isnan(fk.y[2])) and np.all(fk.y[[0, 1, 3, 4], 2] == 0)
        npt.assert_allclose(fk.y[[0, 1, 3, 4], :2], np.linalg.solve(Lr, (m.y[[0, 1, 3, 4]] - m.c).T).T, rtol=0, atol=1e-14)
    # G0 and Gt must be the same potential
    for other in (LinearGaussianPotential(H=2 * G0.H, R=G0.R, c=G0.c, y=G0.y), LinearGaussianPotential(H=G0.H, R=2 * G0.R, c=G0.c, y=G0.y),
                  LinearGaussianPotential(H=G0.H, R=G0.R, c=G0.c + 1, y=G0.y)):
        with pytest.raises(ValueError, match="same H, R and c"):
            _device.describe_independent(M0, other, Mt, Gt, Mt)
        with pytest.raises(ValueError, match="same H, R and c"):
            _device.describe_guided(M0, other, Mt, Gt, Mt)
    with pytest.raises(ValueError):  # the state's dimension
        _device.describe_bootstrap(GaussianInit(m0=np.zeros(2), P0=np.eye(2)), G0, LinearGaussianDynamics(F=np.eye(2), b=np.zeros(2), Q=np.eye(2)), Gt, None)
    # the ctypes mirror: the two fields sit behind the unchanged ones
    names = [f[0] for f in _lib.FkModel._fields_] + [f[0] for f in _lib.FkModelObs._fields_]
    assert names[-4:] == ["nu", "prec", "obs_H", "obs_const"] and _lib.FkModelObs.obs_H.offset == _lib.FkModel.prec.offset + 8
    assert _lib.FkModelObs.obs_const.offset == _lib.FkModelObs.obs_H.offset + 8 and _lib.FkModelObs.nu.offset == _lib.FkModel.nu.offset


def test_tracking_workload():
    from aux_ssm_samplers_amd.workloads import lgssm_tracking_setup
    M0, Mt, G0, Gt, x, y, H, R = lgssm_tracking_setup(9, 24, 12, seed=1)
    assert x.shape == (9, 24) and y.shape == (9, 12) and H.shape == (12, 24) and R.shape == (12, 12) and Gt.params.shape == (8, 12)
    assert np.all(np.any(H != 0, axis=0)) and np.max(np.abs(R - np.diag(np.diag(R)))) > 0.05 and np.linalg.cond(R) <= 50
    F = np.asarray(Mt.F)
    assert np.max(np.abs(np.linalg.eigvals(F))) < 1 and np.all(F[np.abs(np.subtract.outer(np.arange(24), np.arange(24))) > 1] == 0)
    npt.assert_array_equal(G0.H, H)
    npt.assert_array_equal(Gt.R, R)


# ---- 5. the potential as a user program ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dx", [1, 4])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_potential_compiles_as_a_user_program(dtype, dx):
    from aux_ssm_samplers_amd import _lib
    from aux_ssm_samplers_amd.csmc import _device, device_models as U
    for src, flags in ((U.BUILTIN_LINGAUSS, _lib.FK_USER_POTENTIAL), (U.BUILTIN_LINGAUSS_GRAD, _lib.FK_USER_POTENTIAL | _lib.FK_USER_GRADIENT)):
        info = _device.program_info(_device.compile_program(src, dtype, dx, flags))
        assert info == dict(dtype=_lib.dtype_code(dtype), dx=dx, flags=flags, has_bound=1)


# ---- 6. well-posedness of the exact ancestor comparison ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", P.literal_cells(LG.KIND), ids=lambda c: f"{c[0]}-g{c[1]}-bw{int(c[2])}-{c[3]}")
def test_exact_ancestor_comparison_is_well_posed(cell):
    """tests/test_gpu_lingauss.py demands EQUAL ancestors of the device and the fp64 literal while their log-weights agree to 1e-10: fair only if no draw
    r = c[-1] (1 - u) lies within rounding of a cumulative-weight edge c[j].  From the literal sweep of every (cell, case): the smallest |r - c[j]| over all
    resampling and backward draws is >= 1e-8 (weights normalised to sum 1; the rule and number of tests/test_user_model_literals.py).  The seeds of
    tests/lingauss_np.py::SEED_BUMPS were advanced until it held with a factor 3 to spare: smallest gap over the list 3.0e-8 (N = 1024, T = 40)."""
    (x, B, h), cs, _, _ = P.literal_sweep(LG.KIND, *cell)
    gap = P.draw_gap((x, B, h), cs[7], cs[4].dyn, cell[2])
    print(cell, dict(gap=gap, moved=float(np.mean(B != 0))))
    assert gap >= 1e-8
