"""CPU: user-defined Feynman-Kac models are compiled (hipRTC, gfx950) when the kernel is built, with no device: valid sources compile for every
dtype and dx of the sequential sweep, bad sources fail at get_kernel with hipRTC's diagnostics, programs are cached by source, and the limits of the
program path raise NotImplementedError naming them."""
import numpy as np
import pytest

from aux_ssm_samplers_amd.csmc import device_models as U

POTENTIAL_ONLY = U.BUILTIN_GAUSS_OBS
POTENTIAL_AND_MEAN = U.BUILTIN_SV + U.BUILTIN_LINEAR_MEAN


def _models(d, src=POTENTIAL_ONLY, user_mean=False, Q=None):
    from aux_ssm_samplers_amd.csmc import GaussianInit, LinearGaussianDynamics, DevicePotential, DeviceGaussianDynamics
    y = np.zeros((6, d))
    M0 = GaussianInit(m0=np.zeros(d), P0=np.eye(d))
    Q = np.eye(d) if Q is None else Q
    Mt = DeviceGaussianDynamics(src, Q=Q, theta=np.concatenate([np.eye(d).reshape(-1), np.zeros(d)])) if user_mean else \
        LinearGaussianDynamics(F=0.9 * np.eye(d), b=np.zeros(d), Q=Q)
    return M0, DevicePotential(src, y=y[0], theta=[0.5]), Mt, DevicePotential(src, params=y[1:], theta=[0.5])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("dx", [1, 2, 3, 4])
@pytest.mark.parametrize("flags,src", [(1, POTENTIAL_ONLY), (3, POTENTIAL_AND_MEAN)])
def test_valid_sources_compile_without_a_device(dtype, dx, flags, src):
    from aux_ssm_samplers_amd.csmc import _device
    prog = _device.compile_program(src, dtype, dx, flags)
    assert prog and prog.value


def test_get_kernel_compiles_both_dtypes_and_routes_to_the_program():
    from aux_ssm_samplers_amd.csmc import get_independent_kernel, _device
    from aux_ssm_samplers_amd._primitives.csmc import get_kernel
    M0, G0, Mt, Gt = _models(2, POTENTIAL_AND_MEAN, user_mean=True)
    get_independent_kernel(M0, G0, Mt, Gt, 64, True, Mt)
    get_kernel(M0, G0, Mt, Gt, 64, backward=True, Pt=Mt)
    fk = _device.describe_independent(M0, G0, Mt, Gt, Mt)
    assert fk.user is not None and fk.user.flags == 3 and fk.user.p == 2
    # a user potential with the built-in dynamics: only the potential is compiled
    M0, G0, Mt, Gt = _models(1)
    fk = _device.describe_bootstrap(M0, G0, Mt, Gt, Mt)
    assert fk.user.flags == 1


def test_syntax_error_raises_with_the_hiprtc_diagnostic():
    from aux_ssm_samplers_amd._lib import AuxSSMError
    from aux_ssm_samplers_amd.csmc import get_independent_kernel
    bad = "template <typename R, int D> __device__ R log_g(int t, const R* x, const R* xprev, const R* y, const R* theta) {\n    return x[0] +;\n}\n"
    with pytest.raises(AuxSSMError) as e:
        get_independent_kernel(*_models(1, bad), 64)
    msg = str(e.value)
    assert "model.hip:2:" in msg and "error: expected expression" in msg


@pytest.mark.parametrize("src", [
    "template <typename R, int D> __device__ R log_potential(int t, const R* x, const R* xprev, const R* y, const R* theta) { return x[0]; }",
    "template <typename R, int D> __device__ R log_g(int t, const R* x, const R* theta) { return x[0]; }",
    "template <typename R, int D> __device__ int log_g(int t, const R* x, const R* xprev, const R* y, const R* theta) { return 0; }",
])
def test_missing_or_wrong_log_g_fails_at_get_kernel(src):
    from aux_ssm_samplers_amd._lib import AuxSSMError
    from aux_ssm_samplers_amd.csmc import get_independent_kernel
    with pytest.raises(AuxSSMError, match="must define"):
        get_independent_kernel(*_models(1, src), 64)


def test_a_second_get_kernel_with_the_same_source_does_not_recompile():
    from aux_ssm_samplers_amd.csmc import get_independent_kernel, _device
    src = POTENTIAL_ONLY + "\n// cache probe\n"
    n0 = _device.program_compiles()
    get_independent_kernel(*_models(3, src), 64)
    n1 = _device.program_compiles()
    assert n1 == n0 + 2  # f32 and f64
    get_independent_kernel(*_models(3, src), 128)
    from aux_ssm_samplers_amd._primitives.csmc import get_kernel
    get_kernel(*_models(3, src), 64)
    assert _device.program_compiles() == n1


def test_out_of_scope_raises_not_implemented():
    from aux_ssm_samplers_amd.csmc import get_independent_kernel, GaussianInit, DevicePotential, LinearGaussianDynamics
    M0, G0, Mt, Gt = _models(1)
    with pytest.raises(NotImplementedError, match="parallel=True"):
        get_independent_kernel(M0, G0, Mt, Gt, 64, parallel=True)
    with pytest.raises(NotImplementedError, match="gradient"):
        get_independent_kernel(M0, G0, Mt, Gt, 64, gradient=True)
    with pytest.raises(NotImplementedError, match="dx=5"):
        get_independent_kernel(*_models(5), 64)
    with pytest.raises(NotImplementedError, match="M0"):
        get_independent_kernel(G0, G0, Mt, Gt, 64)
    with pytest.raises(NotImplementedError, match="time-varying Q"):
        get_independent_kernel(*_models(1, POTENTIAL_AND_MEAN, user_mean=True, Q=np.ones((5, 1, 1))), 64)
    with pytest.raises(NotImplementedError, match="non-Gaussian"):
        get_independent_kernel(M0, G0, object(), Gt, 64)
    Mtv = LinearGaussianDynamics(F=np.ones((5, 1, 1)), b=np.zeros((5, 1)), Q=np.ones((5, 1, 1)))
    with pytest.raises(NotImplementedError, match="time-varying"):
        get_independent_kernel(M0, G0, Mtv, Gt, 64)


def test_the_reference_shaped_pit_entry_refuses_user_models():
    """_primitives.csmc.pit.get_kernel (the reference's own call shape for the parallel-in-time sweep) must not run a user model as the closed family"""
    from aux_ssm_samplers_amd._primitives.csmc import pit
    from aux_ssm_samplers_amd.csmc import _device
    from aux_ssm_samplers_amd.csmc.independent import AuxiliaryMtDistribution, AuxiliaryG0, AuxiliaryGt
    for user_mean in (False, True):
        M0, G0, Mt, Gt = _models(1, POTENTIAL_AND_MEAN, user_mean=user_mean)
        mt = AuxiliaryMtDistribution(params=(np.zeros((6, 1)), 0.5, None))
        with pytest.raises(NotImplementedError, match="parallel"):
            pit.get_kernel(mt, AuxiliaryG0(M0=M0, G0=G0), AuxiliaryGt(Mt=Mt, Gt=Gt), 64)
    # and the PIT sweep itself refuses a description with device-code parts, whoever built it
    fk = _device.describe_independent(*_models(1), None)
    with pytest.raises(NotImplementedError, match="parallel-in-time"):
        _device.pit_sweep(fk, np.zeros((6, 1)), 64, key=0, delta=0.5)


def test_bound_detection_and_unsupported_status():
    from aux_ssm_samplers_amd.csmc import _device
    with_bound = _device.compile_program(U.BUILTIN_SV, np.float32, 1, 1)
    no_bound = _device.compile_program(U.STUDENT_T, np.float64, 2, 1)
    mean_only = _device.compile_program(U.BUILTIN_LINEAR_MEAN, np.float32, 2, 2)
    assert _device.program_info(with_bound) == dict(dtype=0, dx=1, flags=1, has_bound=1)
    assert _device.program_info(no_bound) == dict(dtype=1, dx=2, flags=1, has_bound=0)
    assert _device.program_info(mean_only)["has_bound"] == 0
    with pytest.raises(NotImplementedError, match="dx=5"):  # AUXSSM_ERR_UNSUPPORTED from the C entry point itself
        _device.compile_program(U.BUILTIN_SV, np.float32, 5, 1)
