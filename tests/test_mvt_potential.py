"""The multivariate Student-t potential of the cSMC family (AUXSSM_POT_MVT, csmc.MultivariateTPotential) without a GPU: known answers of the NumPy formula the
GPU tests compare against (tests/mvt_np.py), the spatial example's precision builder, validation at construction, the model description and the compilation
of the potential as a user program (hipRTC needs no device)."""
import numpy as np
import numpy.testing as npt
import pytest

from oracle import csmc_np as L
from tests import mvt_np as MV
from tests import potential_np as P


def test_scalar_known_answer_and_nan_rule():
    """d = 1, prec = [[1 / s^2]]: -(nu + 1) / 2 log1p((x - y)^2 / (nu s^2)), computed by hand; a NaN in y gives 0"""
    from aux_ssm_samplers_amd.csmc import MultivariateTPotential
    nu, s, y = 3.0, 0.7, 0.4
    x = np.array([[-1.3], [0.4], [2.5], [10.0]])
    want = -(nu + 1) / 2 * np.log1p((x[:, 0] - y) ** 2 / (nu * s * s))
    prec = [[1 / s ** 2]]
    npt.assert_allclose(MV.log_g(x, [y], nu, prec), want, rtol=0, atol=1e-14)
    npt.assert_allclose(MultivariateTPotential(nu=nu, prec=prec)(x, [y]), want, rtol=0, atol=1e-14)
    assert want[1] == 0 and abs(want[2] - (-2.0 * np.log1p(4.41 / 1.47))) < 1e-14  # ((2.5 - 0.4)^2 = 4.41, nu s^2 = 1.47)
    assert np.all(MV.log_g(x, [np.nan], nu, prec) == 0)
    P2 = np.array([[2.0, 0.3], [0.3, 1.0]])
    x2 = np.array([[0.1, -0.2], [1.0, 2.0]])
    assert np.all(MV.log_g(x2, [0.5, np.nan], nu, P2) == 0) and np.all(MV.grad_log_g(x2, [0.5, np.nan], nu, P2) == 0)
    assert np.all(MultivariateTPotential(nu=nu, prec=P2)(x2, [np.nan, 0.5]) == 0)
    # two coupled components by hand: r = (1, 2) - (0.5, 0.5) = (0.5, 1.5); r^T P r = 2 * 0.25 + 2 * 0.3 * 0.75 + 2.25 = 3.2
    assert abs(MV.log_g(x2, [0.5, 0.5], nu, P2)[1] - (-2.5 * np.log1p(3.2 / 3.0))) < 1e-14


def test_closed_form_gradient_equals_central_differences():
    rng = np.random.default_rng(3)
    d, nu = 3, 2.5
    A = rng.standard_normal((d, d))
    prec = np.eye(d) + A @ A.T / d
    for _ in range(5):
        x, y = rng.standard_normal(d), rng.standard_normal(d)
        fd = L.grad_fd(lambda v: float(MV.log_g(v, y, nu, prec)), x)
        npt.assert_allclose(MV.grad_log_g(x, y, nu, prec), fd, rtol=0, atol=1e-6)


def test_joint_gradient_of_the_helper_equals_the_oracles_central_differences():
    """tests/potential_np.py::joint_grad replaces the central differences of oracle.csmc_np.get_independent_kernel(gradient=True): the same quantity"""
    rng = np.random.default_rng(4)
    for tv in (False, True):  # (time-varying: every transition its own F_t, b_t, Q_t)
        dev, m, x, _ = MV.case(2, 6, rng, nan_rows=(3,), tv=tv)
        u = x + 0.3 * rng.standard_normal(x.shape)
        M0, G0, Mt, Gt = m.literal()
        fd = L.grad_fd(lambda v: float(L._log_pdf(v, M0, G0, Mt, Gt)), u)
        npt.assert_allclose(P.joint_grad(m, u), fd, rtol=0, atol=1e-6)


def test_spatial_precision_of_the_two_by_two_grid():
    """the matrix examples/spatial/model.py:43-46 prints"""
    from aux_ssm_samplers_amd.workloads import spatial_setup
    M0, Mt, G0, Gt, x, y, prec = spatial_setup(7, 2)
    want = [[1, -.25, -.25, 0], [-.25, 1, 0, -.25], [-.25, 0, 1, -.25], [0, -.25, -.25, 1]]
    npt.assert_array_equal(prec, want)
    npt.assert_array_equal(G0.prec, want)
    assert x.shape == y.shape == (7, 4) and np.all(np.isfinite(y)) and Gt.params.shape == (6, 4)
    npt.assert_array_equal(np.asarray(Mt.F), np.eye(4))
    # the 5 x 5 grid of the benchmark leg: symmetric positive definite, four neighbours at -1/4
    P5 = spatial_setup(3, 5)[6]
    assert P5.shape == (25, 25) and np.array_equal(P5, P5.T) and np.linalg.eigvalsh(P5).min() > 0.1
    assert P5[12, 12] == 1 and sorted(np.nonzero(P5[12])[0]) == [7, 11, 12, 13, 17]


@pytest.mark.parametrize("kw", [dict(nu=2.0, prec=[[1.0, 0.5], [0.0, 1.0]]),          # not symmetric
                                dict(nu=2.0, prec=[[1.0, 2.0], [2.0, 1.0]]),          # indefinite
                                dict(nu=0.0, prec=[[1.0]]), dict(nu=-1.0, prec=[[1.0]]), dict(nu=float("nan"), prec=[[1.0]]),
                                dict(nu=2.0, prec=np.eye(2), y=np.zeros(3)),          # y of another dimension
                                dict(nu=2.0, prec=np.eye(2), params=np.zeros((5, 3))),
                                dict(nu=2.0, prec=np.ones((2, 3))), dict(nu=2.0, prec=None)])
def test_validation_at_construction(kw):
    from aux_ssm_samplers_amd.csmc import MultivariateTPotential
    with pytest.raises(ValueError):
        MultivariateTPotential(**kw)


def test_description_maps_to_kind_four():
    from aux_ssm_samplers_amd import _lib
    from aux_ssm_samplers_amd.csmc import _device, GaussianInit, LinearGaussianDynamics, MultivariateTPotential
    rng = np.random.default_rng(0)
    dev, m, x, _ = MV.case(3, 5, rng)
    M0, G0, Mt, Gt = dev
    for fk in (_device.describe_independent(M0, G0, Mt, Gt, Mt), _device.describe_independent(M0, G0, Mt, Gt, Mt, _lib.GRAD_EXACT, True),
               _device.describe_bootstrap(M0, G0, Mt, Gt, Mt), _device.describe_guided(M0, G0, Mt, Gt, Mt, _lib.GRAD_REFERENCE)):
        assert fk.potential == _lib.POT_MVT == 4 and fk.user is None
        assert fk.nu == G0.nu and np.array_equal(fk.prec, G0.prec) and fk.prec.flags.c_contiguous
        npt.assert_array_equal(fk.y, m.y)
    # G0 and Gt must be the same potential
    other = MultivariateTPotential(nu=G0.nu + 1, prec=G0.prec, y=G0.y)
    with pytest.raises(ValueError, match="same nu and prec"):
        _device.describe_independent(M0, other, Mt, Gt, Mt)
    other = MultivariateTPotential(nu=G0.nu, prec=2 * G0.prec, y=G0.y)
    with pytest.raises(ValueError, match="same nu and prec"):
        _device.describe_guided(M0, other, Mt, Gt, Mt)
    with pytest.raises(ValueError):  # the state's dimension
        _device.describe_bootstrap(GaussianInit(m0=np.zeros(2), P0=np.eye(2)), G0, LinearGaussianDynamics(F=np.eye(2), b=np.zeros(2), Q=np.eye(2)), Gt, None)
    # the ctypes mirror: the two fields sit at the end, behind the unchanged head
    names = [f[0] for f in _lib.FkModel._fields_]
    assert names[-2:] == ["nu", "prec"] and names[-4:-2] == ["gradient", "reserved"] and _lib.FkModel.nu.offset == _lib.FkModel.gradient.offset + 8


@pytest.mark.parametrize("dx", [1, 4])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_potential_compiles_as_a_user_program(dtype, dx):
    from aux_ssm_samplers_amd import _lib
    from aux_ssm_samplers_amd.csmc import _device, device_models as U
    for src, flags in ((U.BUILTIN_MVT, _lib.FK_USER_POTENTIAL), (U.BUILTIN_MVT_GRAD, _lib.FK_USER_POTENTIAL | _lib.FK_USER_GRADIENT)):
        info = _device.program_info(_device.compile_program(src, dtype, dx, flags))
        assert info == dict(dtype=_lib.dtype_code(dtype), dx=dx, flags=flags, has_bound=1)
