"""Gradient-informed proposals on user-defined Feynman-Kac models (gradient=True / "exact" with DevicePotential / DeviceGaussianDynamics): the program's
gradient kernel (csrc/csmc_sweep.h::k_csmc_grad with the user policy) and its GRAD = true forward passes.

1. Same kernel: the built-in Gaussian-observation / SV potentials and the linear mean written with their derivatives (device_models.*_GRAD / *_VJP)
   give the closed-family gradient sweep BIT FOR BIT: ancestors, trajectories, particles and log-weights; fp32 / fp64, gradient=True and "exact",
   both backward modes, explicit and Threefry noise, N in {64, 100, 1024}, several chains, resident CsmcChains.
2. Literal parity (fp64, explicit noise) against oracle/csmc_np.py's get_independent_kernel(gradient=True, exact_gradient=...), which differentiates
   the joint log-density numerically (grad_fd): the rare-event, Student-t and growth models, and a potential that reads x_{t-1} (observed increments).
3. Ground truth: the rare-event model with gradient="exact" on 1024 chains matches the Kalman smoother's means and variances."""
import dataclasses

import numpy as np
import numpy.testing as npt
import pytest

from oracle import csmc_np as L
from aux_ssm_samplers_amd import _lib
from aux_ssm_samplers_amd.csmc import device_models as U
from tests.test_gpu_user_model import _builtin_pair, _literal_case

pytestmark = pytest.mark.gpu

_WITH_DERIVATIVES = {U.BUILTIN_GAUSS_OBS: U.BUILTIN_GAUSS_OBS_GRAD, U.BUILTIN_SV: U.BUILTIN_SV_GRAD, U.BUILTIN_LINEAR_MEAN: U.BUILTIN_LINEAR_MEAN_VJP,
                     U.RARE_EVENT: U.RARE_EVENT_GRAD, U.STUDENT_T: U.STUDENT_T_GRAD, U.GROWTH: U.GROWTH_GRAD}


def _with_derivatives(m):
    """the same model objects, their device sources replaced by the ones that also define the derivatives"""
    return tuple(dataclasses.replace(o, source=_WITH_DERIVATIVES[o.source]) if hasattr(o, "source") else o for o in m)


def _describe(m, gradient):
    from aux_ssm_samplers_amd.csmc import _device
    return _device.describe_independent(m[0], m[1], m[2], m[3], m[2], _lib.GRAD_EXACT if gradient == "exact" else _lib.GRAD_REFERENCE)


def _assert_same_sweeps(fb, fu, x0, N, delta, rng, C, T, d, dtype):
    from aux_ssm_samplers_amd import random as R
    from aux_ssm_samplers_amd.csmc import _device
    for backward in (True, False):
        key = R.PRNGKey(int(rng.integers(1 << 30)))
        for kw in (dict(key=key), dict(noise=_device.key_noise(_device._lib.default_handle(), key, C, T, N, d, dtype))):
            xb, ab, hb = _device.sweep(fb, x0, N, backward, delta=delta, want_history=True, **kw)
            xu, au, hu = _device.sweep(fu, x0, N, backward, delta=delta, want_history=True, **kw)
            npt.assert_array_equal(ab, au)
            npt.assert_array_equal(xb, xu)
            for k in ("xs", "log_ws", "As"):
                npt.assert_array_equal(hb[k], hu[k])
            assert (ab != 0).any()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("gradient", [True, "exact"])
@pytest.mark.parametrize("kind", ["gauss", "sv"])
@pytest.mark.parametrize("N", [64, 100, 1024])
def test_gradient_program_sweep_is_the_builtin_gradient_sweep_bit_for_bit(dtype, gradient, kind, N):
    rng = np.random.default_rng(3000 * N + 2 * (kind == "sv") + (gradient == "exact"))
    T, d, C = 40, 2 if kind == "gauss" else 1, 5
    mb, mu, x = _builtin_pair(kind, d, T, rng)
    fb, fu = _describe(mb, gradient), _describe(_with_derivatives(mu), gradient)
    assert fb.user is None and fu.user.flags == _lib.FK_USER_POTENTIAL | _lib.FK_USER_MEAN | _lib.FK_USER_GRADIENT
    x0 = (x[None] + 0.2 * rng.standard_normal((C, T, d))).astype(dtype)
    delta = 0.3 + 0.2 * rng.random(T)
    _assert_same_sweeps(fb, fu, x0, N, delta, rng, C, T, d, dtype)


@pytest.mark.parametrize("parts", ["potential", "mean"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_one_user_part_keeps_the_builtin_derivative_of_the_other(parts, dtype):
    """a user potential with the built-in linear dynamics (F^T from FkDev), or the built-in potential with a user mean: still the built-in sweep"""
    rng = np.random.default_rng(17 + (parts == "mean"))
    T, d, C, N = 30, 3, 4, 100
    mb, mu, x = _builtin_pair("gauss", d, T, rng)
    mu = _with_derivatives(mu)
    mixed = (mb[0], mu[1], mb[2], mu[3]) if parts == "potential" else (mb[0], mb[1], mu[2], mb[3])
    fb, fu = _describe(mb, "exact"), _describe(mixed, "exact")
    assert fu.user.flags == (_lib.FK_USER_POTENTIAL if parts == "potential" else _lib.FK_USER_MEAN) | _lib.FK_USER_GRADIENT
    x0 = (x[None] + 0.2 * rng.standard_normal((C, T, d))).astype(dtype)
    _assert_same_sweeps(fb, fu, x0, N, 0.4, rng, C, T, d, dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("gradient", [True, "exact"])
def test_resident_chains_gradient_program_equals_builtin(dtype, gradient):
    from aux_ssm_samplers_amd import random as R
    from aux_ssm_samplers_amd.csmc import CsmcChains, CSMCState, get_independent_kernel
    rng = np.random.default_rng(12)
    T, d, C, N = 60, 1, 300, 1024
    mb, mu, x = _builtin_pair("sv", d, T, rng)
    mu = _with_derivatives(mu)
    x0 = x[None] + 0.2 * rng.standard_normal((C, T, d))
    h = _lib.default_handle()
    kb = get_independent_kernel(*mb, N, True, mb[2], gradient=gradient)[1]
    ku = get_independent_kernel(*mu, N, True, mu[2], gradient=gradient)[1]
    cb, cu = CsmcChains(h, x0, delta=0.5, dtype=dtype), CsmcChains(h, x0, delta=0.5, dtype=dtype)
    sb, su = CSMCState(x=cb, updated=None), CSMCState(x=cu, updated=None)
    for it in range(3):
        sb = kb(R.PRNGKey(200 + it), sb, None)
        su = ku(R.PRNGKey(200 + it), su, None)
    npt.assert_array_equal(cb.to_host(), cu.to_host())
    npt.assert_array_equal(cb.ancestors.to_host(), cu.ancestors.to_host())
    assert (cu.ancestors.to_host() != 0).mean() > 0.1


# ---- literal parity ---------------------------------------------------------------------------------------------------------------------------------
class _IncrementPot:
    """log N(y_t; x_t - x_{t-1}, s^2 I) (y_0 ~ N(x_0, s^2 I)): a potential of (x_t, x_{t-1}); params = y_t rows"""

    def __init__(self, y, s, first=False):
        self.y, self.s, self.first = y, s, first
        self.params = None if first else y[1:]

    def __call__(self, x, x_prev=None, params=None):
        if self.first:
            return np.sum(L.norm_logpdf(self.y[0], x, self.s), axis=-1)
        return np.sum(L.norm_logpdf(params, x - x_prev, self.s), axis=-1)


def _increment_case(T, rng):
    from aux_ssm_samplers_amd.csmc import GaussianInit, LinearGaussianDynamics, DevicePotential
    d, Fv, Qv, s = 2, 0.9, 0.5, 0.4
    x = np.zeros((T, d))
    x[0] = rng.standard_normal(d)
    for t in range(1, T):
        x[t] = Fv * x[t - 1] + np.sqrt(Qv) * rng.standard_normal(d)
    y = np.diff(x, axis=0, prepend=0.0) + s * rng.standard_normal((T, d))
    Mt = LinearGaussianDynamics(F=Fv * np.eye(d), b=np.zeros(d), Q=Qv * np.eye(d))
    dev = (GaussianInit(m0=np.zeros(d), P0=np.eye(d)), DevicePotential(U.INCREMENT_OBS_GRAD, y=y[0], theta=[s]), Mt,
           DevicePotential(U.INCREMENT_OBS_GRAD, params=y[1:], theta=[s]))
    lit = (L.GaussianInit(np.zeros(d), np.eye(d)), _IncrementPot(y, s, True),
           L.LinearGaussianDynamics(Fv * np.eye(d), np.zeros(d), np.sqrt(Qv) * np.eye(d), T), _IncrementPot(y, s))
    return dev, lit, x


@pytest.mark.parametrize("backward", [True, False])
@pytest.mark.parametrize("gradient", [True, "exact"])
@pytest.mark.parametrize("case", ["rare_event", "student_t", "growth", "increments"])
def test_gradient_program_fp64_equals_the_literal_restatement(case, gradient, backward):
    from aux_ssm_samplers_amd.csmc import _device
    rng = np.random.default_rng(70 + backward)
    T, N = 50, 256
    if case == "increments":
        dev, lit, xtrue = _increment_case(T, rng)
    else:
        dev, lit, xtrue = _literal_case(case, T, rng)
        dev = _with_derivatives(dev)
    d = xtrue.shape[1]
    x0 = xtrue + 0.3 * rng.standard_normal((T, d))
    delta = 0.2 + 0.3 * rng.random(T)
    nz = dict(eps_aux=rng.standard_normal((T, d)), eps_prop=rng.standard_normal((T, N, d)), u_res=rng.random((T - 1, N)), u_bwd=rng.random(T))
    fk = _describe(dev, gradient)
    assert fk.user.flags & _lib.FK_USER_GRADIENT
    x, anc, hist = _device.sweep(fk, x0, N, backward, noise={k: v[None] for k, v in nz.items()}, delta=delta, want_history=True)
    _, kern = L.get_independent_kernel(lit[0], lit[1], lit[2], lit[3], N, backward=backward, Pt=lit[2], gradient=True,
                                       exact_gradient=gradient == "exact")
    xl, Bl, lh = kern(L.Noise(**nz), x0, delta)
    npt.assert_array_equal(hist["As"], lh["As"])
    npt.assert_array_equal(anc, Bl)
    npt.assert_allclose(hist["xs"], lh["xs"], rtol=1e-7, atol=1e-7)
    npt.assert_allclose(x, xl, rtol=1e-7, atol=1e-7)
    assert (hist["As"] != 0).any()  # (the new path may be the reference one -- the rare-event model traced without backward sampling keeps it -- but not every draw)


def test_the_xprev_term_moves_the_proposals():
    """the increments model's gradient includes d_xprev log G_{t+1}: without it (a source whose grad_log_g leaves gxprev alone) the proposals differ"""
    from aux_ssm_samplers_amd.csmc import _device
    rng = np.random.default_rng(5)
    T, N = 20, 64
    dev, _, xtrue = _increment_case(T, rng)
    d = xtrue.shape[1]
    no_xprev = U.INCREMENT_OBS_GRAD.replace("if (gxprev) gxprev[k] = -z / s;", "")
    dev2 = tuple(dataclasses.replace(o, source=no_xprev) if hasattr(o, "source") else o for o in dev)
    nz = dict(eps_aux=rng.standard_normal((1, T, d)), eps_prop=rng.standard_normal((1, T, N, d)), u_res=rng.random((1, T - 1, N)), u_bwd=rng.random((1, T)))
    x0 = xtrue + 0.3 * rng.standard_normal((T, d))
    _, _, h1 = _device.sweep(_describe(dev, "exact"), x0, N, True, noise=nz, delta=0.4, want_history=True)
    _, _, h2 = _device.sweep(_describe(dev2, "exact"), x0, N, True, noise=nz, delta=0.4, want_history=True)
    # every proposal but the reference particle (slot 0) at every step but the last one (which has no t + 1 potential)
    assert np.abs(h1["xs"][:-1, 1:] - h2["xs"][:-1, 1:]).min() > 0
    npt.assert_array_equal(h1["xs"][-1], h2["xs"][-1])


# ---- ground truth ----------------------------------------------------------------------------------------------------------------------------------------
def test_rare_event_gradient_particle_gibbs_matches_the_kalman_smoother():
    """gradient="exact" auxiliary particle Gibbs (resident chains, Threefry keys) on the rare-event model: posterior means and variances at several t
    within 5 Monte Carlo standard errors of the exact Gaussian posterior (AR(1) prior with unit marginals, one observation y ~ N(x_{T-1}, r^2))"""
    from aux_ssm_samplers_amd import random as R
    from aux_ssm_samplers_amd.csmc import CsmcChains, CSMCState, DevicePotential, DeviceGaussianDynamics, GaussianInit, get_independent_kernel
    T, rho, r2, yv = 12, 0.9, 0.25, 2.0
    # the chains start at x = 0: from there the gradient-shifted proposals take longer than the plain ones to reach the posterior (measured: 60 sweeps leave
    # the means 2 - 7 standard errors low at delta = 0.5 - 1, 300 sweeps leave none beyond 2), hence the longer burn-in than the plain sampler's test
    C, N, burn, iters, delta = 1024, 256, 300, 240, 0.5
    th = [T, yv, np.sqrt(r2)]
    M0 = GaussianInit(m0=[0.0], P0=[[1.0]])
    Mt = DeviceGaussianDynamics(U.RARE_EVENT_GRAD, Q=[[1 - rho ** 2]], theta=[rho])
    _, kern = get_independent_kernel(M0, DevicePotential(U.RARE_EVENT_GRAD, theta=th), Mt, DevicePotential(U.RARE_EVENT_GRAD, theta=th), N, True, Mt,
                                     gradient="exact")
    S = rho ** np.abs(np.subtract.outer(np.arange(T), np.arange(T)))
    k = S[:, -1] / (S[-1, -1] + r2)
    mean_true, var_true = k * yv, np.diag(S) - k * S[-1, :]
    h = _lib.default_handle()
    chains = CsmcChains(h, np.zeros((C, T, 1)), delta=delta, dtype=np.float64)
    state = CSMCState(x=chains, updated=None)
    s1, s2 = np.zeros((C, T)), np.zeros((C, T))
    for it in range(burn + iters):
        state = kern(R.PRNGKey(5000 + it), state, None)
        if it >= burn:
            xh = chains.to_host()[..., 0]
            s1 += xh
            s2 += xh * xh
    m1, m2 = s1 / iters, s2 / iters  # per-chain time averages: independent across chains
    est_mean, est_m2 = m1.mean(0), m2.mean(0)
    se_mean, se_m2 = m1.std(0, ddof=1) / np.sqrt(C), m2.std(0, ddof=1) / np.sqrt(C)
    for t in (0, T // 2, T - 2, T - 1):
        assert abs(est_mean[t] - mean_true[t]) < 5 * se_mean[t], (t, est_mean[t], mean_true[t], se_mean[t])
        m2_true = var_true[t] + mean_true[t] ** 2
        assert abs(est_m2[t] - m2_true) < 5 * se_m2[t], (t, est_m2[t], m2_true, se_m2[t])
    assert mean_true[-1] > 1.5
