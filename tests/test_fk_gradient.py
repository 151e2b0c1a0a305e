"""CPU: gradient programs of user-defined Feynman-Kac models (csmc.models.DevicePotential / DeviceGaussianDynamics with gradient=True / "exact").
They compile with no device for every dtype and dx of the sequential sweep. A user-defined part without its derivative (grad_log_g / mean_vjp, or one of
another signature) raises NotImplementedError naming it at get_kernel. gradient=False programs are unchanged, and a gradient program is a cache entry
of its own."""
import numpy as np
import pytest

from aux_ssm_samplers_amd import _lib
from aux_ssm_samplers_amd.csmc import device_models as U

POTENTIAL_ONLY = U.BUILTIN_GAUSS_OBS_GRAD
MEAN_ONLY = U.BUILTIN_LINEAR_MEAN_VJP
POTENTIAL_AND_MEAN = U.BUILTIN_SV_GRAD + U.BUILTIN_LINEAR_MEAN_VJP


def _models(d, pot_src=POTENTIAL_ONLY, mean_src=None):
    from aux_ssm_samplers_amd.csmc import GaussianInit, LinearGaussianDynamics, DevicePotential, DeviceGaussianDynamics
    y = np.zeros((6, d))
    M0 = GaussianInit(m0=np.zeros(d), P0=np.eye(d))
    Mt = DeviceGaussianDynamics(mean_src, Q=np.eye(d), theta=np.concatenate([np.eye(d).reshape(-1), np.zeros(d)])) if mean_src else \
        LinearGaussianDynamics(F=0.9 * np.eye(d), b=np.zeros(d), Q=np.eye(d))
    return M0, DevicePotential(pot_src, y=y[0], theta=[0.5]), Mt, DevicePotential(pot_src, params=y[1:], theta=[0.5])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("dx", [1, 2, 3, 4])
@pytest.mark.parametrize("flags,src", [(_lib.FK_USER_POTENTIAL, POTENTIAL_ONLY), (_lib.FK_USER_MEAN, MEAN_ONLY),
                                       (_lib.FK_USER_POTENTIAL | _lib.FK_USER_MEAN, POTENTIAL_AND_MEAN)])
def test_gradient_programs_compile_without_a_device(dtype, dx, flags, src):
    from aux_ssm_samplers_amd.csmc import _device
    prog = _device.compile_program(src, dtype, dx, flags | _lib.FK_USER_GRADIENT)
    assert prog and prog.value
    info = _device.program_info(prog)
    assert info["flags"] == flags | _lib.FK_USER_GRADIENT and info["dx"] == dx


@pytest.mark.parametrize("gradient", [True, "exact"])
def test_get_kernel_with_gradient_compiles_a_gradient_program(gradient):
    from aux_ssm_samplers_amd.csmc import get_independent_kernel, _device
    from aux_ssm_samplers_amd.csmc.generic import IndependentFactory, get_kernel
    M0, G0, Mt, Gt = _models(2, U.BUILTIN_SV_GRAD, MEAN_ONLY)
    get_independent_kernel(M0, G0, Mt, Gt, 64, True, Mt, gradient=gradient)
    fac = IndependentFactory(M0, G0, Mt, Gt, Mt, _lib.GRAD_EXACT if gradient == "exact" else _lib.GRAD_REFERENCE)
    get_kernel(fac, 64, True, Mt)
    assert fac.fk.user.flags == _lib.FK_USER_POTENTIAL | _lib.FK_USER_MEAN | _lib.FK_USER_GRADIENT
    assert fac.fk.gradient == (_lib.GRAD_EXACT if gradient == "exact" else _lib.GRAD_REFERENCE)
    # a user potential with the built-in dynamics: the built-in part keeps its own derivative (F^T), nothing more is asked of the source
    fk = _device.describe_independent(*_models(1), None, _lib.GRAD_REFERENCE)
    assert fk.user.flags == _lib.FK_USER_POTENTIAL | _lib.FK_USER_GRADIENT


GRAD_WRONG = "template <typename R, int D> __device__ void grad_log_g(int t, const R* x, const R* y, const R* theta, R* gx) { gx[0] = 0; }\n"
GRAD_WRONG_RET = ("template <typename R, int D> __device__ R grad_log_g(int t, const R* x, const R* xprev, const R* y, const R* theta, R* gx, R* gxprev) "
                  "{ return 0; }\n")
VJP_WRONG = "template <typename R, int D> __device__ void mean_vjp(int t, const R* xprev, const R* v, R* out) { out[0] = v[0]; }\n"


@pytest.mark.parametrize("pot_src", [U.BUILTIN_GAUSS_OBS, U.BUILTIN_GAUSS_OBS + GRAD_WRONG, U.BUILTIN_GAUSS_OBS + GRAD_WRONG_RET])
def test_a_user_potential_without_grad_log_g_raises(pot_src):
    from aux_ssm_samplers_amd.csmc import get_independent_kernel
    with pytest.raises(NotImplementedError, match="gradient.*grad_log_g"):
        get_independent_kernel(*_models(1, pot_src), 64, gradient=True)


@pytest.mark.parametrize("mean_src", [U.BUILTIN_LINEAR_MEAN, U.BUILTIN_LINEAR_MEAN + VJP_WRONG])
def test_a_user_mean_without_mean_vjp_raises(mean_src):
    from aux_ssm_samplers_amd.csmc import get_independent_kernel, SVPotential, GaussianInit, DeviceGaussianDynamics
    with pytest.raises(NotImplementedError, match="gradient.*mean_vjp"):
        get_independent_kernel(*_models(2, POTENTIAL_ONLY, mean_src), 64, gradient="exact")
    # the built-in potential with a user mean: only mean_vjp is asked for
    d = 1
    Mt = DeviceGaussianDynamics(mean_src, Q=np.eye(d), theta=[0.9, 0.0])
    y = np.ones((6, d))
    with pytest.raises(NotImplementedError, match="mean_vjp"):
        get_independent_kernel(GaussianInit(m0=np.zeros(d), P0=np.eye(d)), SVPotential(y=y[0]), Mt, SVPotential(params=y[1:]), 64, gradient=True)


def test_the_c_entry_point_refuses_a_missing_derivative_with_unsupported():
    from aux_ssm_samplers_amd.csmc import _device
    with pytest.raises(NotImplementedError, match="gradient") as e:  # AUXSSM_ERR_UNSUPPORTED
        _device.compile_program(U.BUILTIN_SV, np.float32, 1, _lib.FK_USER_POTENTIAL | _lib.FK_USER_GRADIENT)
    assert "grad_log_g" in str(e.value)
    both = _lib.FK_USER_POTENTIAL | _lib.FK_USER_MEAN | _lib.FK_USER_GRADIENT
    with pytest.raises(NotImplementedError, match="mean_vjp") as e:
        _device.compile_program(U.BUILTIN_GAUSS_OBS_GRAD + U.BUILTIN_LINEAR_MEAN, np.float64, 1, both)
    assert "grad_log_g" not in str(e.value)
    with pytest.raises(NotImplementedError, match="grad_log_g.*mean_vjp"):  # every missing derivative is named
        _device.compile_program(U.GROWTH, np.float64, 1, both)


def test_parallel_with_gradient_still_raises_the_parallel_error():
    from aux_ssm_samplers_amd.csmc import get_independent_kernel
    with pytest.raises(NotImplementedError, match="parallel=True"):
        get_independent_kernel(*_models(1), 64, parallel=True, gradient=True)
    with pytest.raises(NotImplementedError, match="parallel=True"):
        get_independent_kernel(*_models(1, U.BUILTIN_GAUSS_OBS), 64, parallel=True, gradient="exact")


def test_gradient_programs_are_cache_entries_of_their_own():
    from aux_ssm_samplers_amd.csmc import get_independent_kernel, _device
    src = U.STUDENT_T_GRAD + "\n// gradient cache probe\n"
    n0 = _device.program_compiles()
    get_independent_kernel(*_models(2, src), 64)
    n1 = _device.program_compiles()
    assert n1 == n0 + 2  # gradient=False: f32 and f64, exactly as before
    fk = _device.describe_independent(*_models(2, src), None)
    assert fk.user.flags == _lib.FK_USER_POTENTIAL and _device.program_info(fk.user.program(np.float32))["flags"] == _lib.FK_USER_POTENTIAL
    get_independent_kernel(*_models(2, src), 64, gradient=True)
    n2 = _device.program_compiles()
    assert n2 == n1 + 2  # the gradient program: f32 and f64
    get_independent_kernel(*_models(2, src), 128, gradient="exact")  # same program (the mode is a sweep argument)
    get_independent_kernel(*_models(2, src), 64)
    assert _device.program_compiles() == n2
    fg = _device.describe_independent(*_models(2, src), None, _lib.GRAD_EXACT)
    assert fg.user.program(np.float64).value != fk.user.program(np.float64).value
