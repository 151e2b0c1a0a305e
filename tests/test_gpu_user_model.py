"""User-defined Feynman-Kac models compiled into the sequential cSMC sweep (csmc.models.DevicePotential / DeviceGaussianDynamics, csrc/fk_program.hip).

1. Same kernel: the built-in Gaussian-observation and SV potentials, their bounds and the linear mean written as user source (csmc/device_models.py)
   give the closed-family sweep's ancestors, trajectories and log-weights BIT FOR BIT: fp32 / fp64, both proposals, both backward modes, explicit and
   Threefry noise, N in {64, 100, 1024}, several chains, resident CsmcChains.
2. Literal parity on models the closed family cannot express, against oracle/csmc_np.py's generic protocol objects on the same explicit noise (fp64):
   the reference's rare-event model, Student-t observations (lgamma), the nonlinear growth model.  fp32: the tie rate of the resampling draws.
3. Ground truth: the rare-event model's posterior is Gaussian (AR(1) prior, one Gaussian observation at T - 1); particle Gibbs on 1024 chains matches
   the Kalman smoother's means and variances within a stated multiple of their Monte Carlo standard errors."""
import numpy as np
import numpy.testing as npt
import pytest

from oracle import csmc_np as L
from aux_ssm_samplers_amd.csmc import device_models as U

pytestmark = pytest.mark.gpu


def _builtin_pair(kind, d, T, rng):
    """(closed-family model, the same model as user source): M0, G0, Mt, Gt of each, and a reference trajectory"""
    from aux_ssm_samplers_amd.csmc import GaussianInit, LinearGaussianDynamics, GaussianObsPotential, SVPotential, DevicePotential, DeviceGaussianDynamics
    F = 0.9 * np.eye(d) + 0.02 * np.tril(np.ones((d, d)), -1)
    b = 0.1 * np.arange(d)
    Q = 0.5 * np.eye(d) + 0.1
    x = np.zeros((T, d))
    for t in range(1, T):
        x[t] = F @ x[t - 1] + b + np.linalg.cholesky(Q) @ rng.standard_normal(d)
    M0 = GaussianInit(m0=np.zeros(d), P0=np.eye(d))
    Mt = LinearGaussianDynamics(F=F, b=b, Q=Q)
    Mu = DeviceGaussianDynamics(U.BUILTIN_LINEAR_MEAN, Q=Q, theta=np.concatenate([F.reshape(-1), b]))
    if kind == "gauss":
        sig = 0.7
        y = x + sig * rng.standard_normal((T, d))
        G0, Gt = GaussianObsPotential(sig=sig, y=y[0]), GaussianObsPotential(sig=sig, params=y[1:])
        src, th = U.BUILTIN_GAUSS_OBS, [sig]
    else:
        y = np.exp(0.5 * x) * rng.standard_normal((T, d))
        G0, Gt = SVPotential(y=y[0]), SVPotential(params=y[1:])
        src, th = U.BUILTIN_SV, None
    Gu0, Gut = DevicePotential(src, y=y[0], theta=th), DevicePotential(src, params=y[1:], theta=th)
    return (M0, G0, Mt, Gt), (M0, Gu0, Mu, Gut), x


def _describe(proposal, m):
    from aux_ssm_samplers_amd.csmc import _device
    if proposal == "bootstrap":
        return _device.describe_bootstrap(m[0], m[1], m[2], m[3], m[2])
    return _device.describe_independent(m[0], m[1], m[2], m[3], m[2])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("proposal", ["bootstrap", "independent"])
@pytest.mark.parametrize("kind", ["gauss", "sv"])
@pytest.mark.parametrize("N", [64, 100, 1024])
def test_program_sweep_is_the_builtin_sweep_bit_for_bit(dtype, proposal, kind, N):
    from aux_ssm_samplers_amd import random as R
    from aux_ssm_samplers_amd.csmc import _device
    rng = np.random.default_rng(1000 * N + (kind == "sv"))
    T, d, C = 40, 2 if kind == "gauss" else 1, 5
    mb, mu, x = _builtin_pair(kind, d, T, rng)
    fb, fu = _describe(proposal, mb), _describe(proposal, mu)
    assert fu.user is not None and fb.user is None
    x0 = (x[None] + 0.2 * rng.standard_normal((C, T, d))).astype(dtype)
    delta = 0.3 + 0.2 * rng.random(T)
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


def test_program_dx4_fp64_full_workgroup_beyond_64k_lds():
    """dx = 4, fp64, N = 1024: the forward pass needs ~83 KB of LDS (more than a module function gets without asking); still bit for bit"""
    from aux_ssm_samplers_amd import random as R
    from aux_ssm_samplers_amd.csmc import _device
    rng = np.random.default_rng(4)
    T, d, C, N = 24, 4, 3, 1024
    mb, mu, x = _builtin_pair("gauss", d, T, rng)
    x0 = x[None] + 0.2 * rng.standard_normal((C, T, d))
    for proposal in ("bootstrap", "independent"):
        fb, fu = _describe(proposal, mb), _describe(proposal, mu)
        xb, ab, _ = _device.sweep(fb, x0, N, True, key=R.PRNGKey(5), delta=0.4)
        xu, au, _ = _device.sweep(fu, x0, N, True, key=R.PRNGKey(5), delta=0.4)
        npt.assert_array_equal(ab, au)
        npt.assert_array_equal(xb, xu)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_resident_chains_program_equals_builtin(dtype):
    from aux_ssm_samplers_amd import _lib, random as R
    from aux_ssm_samplers_amd.csmc import CsmcChains, CSMCState, get_independent_kernel
    from aux_ssm_samplers_amd._primitives.csmc import get_kernel as get_bootstrap_kernel
    rng = np.random.default_rng(11)
    T, d, C, N = 60, 1, 300, 1024
    mb, mu, x = _builtin_pair("sv", d, T, rng)
    x0 = x[None] + 0.2 * rng.standard_normal((C, T, d))
    h = _lib.default_handle()
    for make in (lambda m: get_independent_kernel(*m, N, True, m[2])[1], lambda m: get_bootstrap_kernel(*m, N, backward=True, Pt=m[2])[1]):
        kb, ku = make(mb), make(mu)
        cb, cu = CsmcChains(h, x0, delta=0.5, dtype=dtype), CsmcChains(h, x0, delta=0.5, dtype=dtype)
        sb, su = CSMCState(x=cb, updated=None), CSMCState(x=cu, updated=None)
        for it in range(3):
            sb = kb(R.PRNGKey(100 + it), sb, None)
            su = ku(R.PRNGKey(100 + it), su, None)
        npt.assert_array_equal(cb.to_host(), cu.to_host())
        npt.assert_array_equal(cb.ancestors.to_host(), cu.ancestors.to_host())
        assert (cu.ancestors.to_host() != 0).mean() > 0.1


# ---- literal parity: generic protocol objects in oracle/csmc_np.py ------------------------------------------------------------------------------------
class _MeanDyn(L.Dynamics):
    """x_t ~ N(mean(x_{t-1}, t), L L^T); params = the time index t of x_t (leading axis T - 1)"""

    def __init__(self, mean, LQ, T):
        self.mean, self.L, self.params = mean, np.asarray(LQ), np.arange(1, T)

    def sample(self, key, x_t, t):
        return self.mean(x_t, t) + key @ self.L.T

    def logpdf(self, x_t_p_1, x_t, t):
        return L._mvn_chol_logpdf(x_t_p_1, self.mean(x_t, t), self.L)


class _Pot:
    """G_t(x_t) = g(t, x_t, y_t); params = (t, y_t) rows"""

    def __init__(self, g, y, T, first=False):
        self.g, self.y, self.T, self.first = g, y, T, first
        self.params = None if first else (np.arange(1, T), y[1:] if y is not None else np.zeros((T - 1, 1)))

    def __call__(self, x, x_prev=None, params=None):
        if self.first:
            return self.g(0, x, None if self.y is None else self.y[0])
        t, yt = params
        return self.g(int(t), x, yt)


def _literal_case(case, T, rng):
    """(device M0, G0, Mt, Gt), (literal M0, G0, Mt, Gt), a reference trajectory"""
    from aux_ssm_samplers_amd.csmc import GaussianInit, LinearGaussianDynamics, DevicePotential, DeviceGaussianDynamics
    from scipy.special import gammaln
    M0 = GaussianInit(m0=[0.0], P0=[[1.0]])
    Mo = L.GaussianInit(np.zeros(1), np.eye(1))
    if case == "rare_event":
        rho, r2, yv = 0.9, 0.1, 2.5
        r, sx = np.sqrt(r2), np.sqrt(1 - rho ** 2)
        th = [T, yv, r]
        dev = (M0, DevicePotential(U.RARE_EVENT, theta=th), DeviceGaussianDynamics(U.RARE_EVENT, Q=[[1 - rho ** 2]], theta=[rho]),
               DevicePotential(U.RARE_EVENT, theta=th))
        g = lambda t, x, y: np.where(t == T - 1, L.norm_logpdf(yv, x[..., 0], r), 0.0)
        lit = (Mo, _Pot(g, None, T, True), _MeanDyn(lambda x, t: rho * x, [[sx]], T), _Pot(g, None, T))
        x = np.zeros((T, 1))
        for t in range(1, T):
            x[t] = rho * x[t - 1] + sx * rng.standard_normal(1)
        x[-1] = yv
        return dev, lit, x
    if case == "student_t":
        nu, s, F, Qv = 4.0, 0.5, 0.95, 0.3
        x = np.zeros((T, 1))
        for t in range(1, T):
            x[t] = F * x[t - 1] + np.sqrt(Qv) * rng.standard_normal(1)
        y = x + s * rng.standard_t(nu, (T, 1))
        Mt = LinearGaussianDynamics(F=[[F]], b=[0.0], Q=[[Qv]])
        dev = (M0, DevicePotential(U.STUDENT_T, y=y[0], theta=[nu, s]), Mt, DevicePotential(U.STUDENT_T, params=y[1:], theta=[nu, s]))
        c = gammaln((nu + 1) / 2) - gammaln(nu / 2) - 0.5 * np.log(nu * np.pi * s * s)

        def g(t, xx, yt):
            z = (yt[0] - xx[..., 0]) / s
            return c - (nu + 1) / 2 * np.log1p(z * z / nu)
        lit = (Mo, _Pot(g, y, T, True), L.LinearGaussianDynamics(np.array([[F]]), np.zeros(1), np.array([[np.sqrt(Qv)]]), T), _Pot(g, y, T))
        return dev, lit, x
    sig, Qv = 1.0, 1.0  # growth
    mean = lambda v, t: v / 2 + 25 * v / (1 + v * v) + 8 * np.cos(1.2 * t)
    x = np.zeros((T, 1))
    x[0] = rng.standard_normal(1)
    for t in range(1, T):
        x[t] = mean(x[t - 1], t) + np.sqrt(Qv) * rng.standard_normal(1)
    y = x ** 2 / 20 + sig * rng.standard_normal((T, 1))
    dev = (M0, DevicePotential(U.GROWTH, y=y[0], theta=[sig]), DeviceGaussianDynamics(U.GROWTH, Q=[[Qv]]),
           DevicePotential(U.GROWTH, params=y[1:], theta=[sig]))
    g = lambda t, xx, yt: L.norm_logpdf(yt[0], xx[..., 0] ** 2 / 20, sig)
    lit = (Mo, _Pot(g, y, T, True), _MeanDyn(mean, [[np.sqrt(Qv)]], T), _Pot(g, y, T))
    return dev, lit, x


@pytest.mark.parametrize("backward", [True, False])
@pytest.mark.parametrize("case,proposal", [("rare_event", "independent"), ("student_t", "independent"), ("growth", "independent"),
                                           ("growth", "bootstrap"), ("student_t", "bootstrap")])
def test_program_sweep_fp64_equals_the_literal_restatement(case, proposal, backward):
    from aux_ssm_samplers_amd.csmc import _device
    rng = np.random.default_rng(7 + backward)
    T, N, d = 50, 256, 1
    dev, lit, xtrue = _literal_case(case, T, rng)
    x0 = xtrue + 0.3 * rng.standard_normal((T, d))
    delta = 0.2 + 0.3 * rng.random(T)
    nz = dict(eps_aux=rng.standard_normal((T, d)), eps_prop=rng.standard_normal((T, N, d)), u_res=rng.random((T - 1, N)), u_bwd=rng.random(T))
    fk = _describe(proposal, dev)
    x, anc, hist = _device.sweep(fk, x0, N, backward, noise={k: v[None] for k, v in nz.items()}, delta=delta, want_history=True)
    if proposal == "independent":
        _, kern = L.get_independent_kernel(lit[0], lit[1], lit[2], lit[3], N, backward=backward, Pt=lit[2])
        xl, Bl, lh = kern(L.Noise(**nz), x0, delta)
    else:
        _, kern = L.get_kernel(lit[0], lit[1], lit[2], lit[3], N, backward=backward, Pt=lit[2])
        xl, Bl, lh = kern(L.Noise(**nz), x0)
    npt.assert_array_equal(hist["As"], lh["As"])
    npt.assert_array_equal(anc, Bl)
    npt.assert_allclose(x, xl, rtol=1e-12, atol=1e-12)
    npt.assert_allclose(hist["xs"], lh["xs"], rtol=1e-12, atol=1e-12)
    npt.assert_allclose(hist["log_ws"], lh["log_ws"], rtol=1e-10, atol=1e-10)
    assert (anc != 0).any()


def test_program_fp32_resampling_tie_rate():
    """fp32 growth model: the device's resampling ancestors vs the literal fp32 order (normalise -> cumsum -> searchsorted) redone from the device's
    own stored log-weights and the same uniforms, step by step (teacher-forced): misses are rare and land on a neighbouring particle"""
    from aux_ssm_samplers_amd.csmc import _device
    rng = np.random.default_rng(21)
    T, N, d, C = 60, 1024, 1, 4
    dev, _, xtrue = _literal_case("growth", T, rng)
    fk = _describe("independent", dev)
    x0 = (xtrue[None] + 0.3 * rng.standard_normal((C, T, d))).astype(np.float32)
    nz = dict(eps_aux=rng.standard_normal((C, T, d)), eps_prop=rng.standard_normal((C, T, N, d)), u_res=rng.random((C, T - 1, N)), u_bwd=rng.random((C, T)))
    nz = {k: v.astype(np.float32) for k, v in nz.items()}
    _, _, hist = _device.sweep(fk, x0, N, True, noise=nz, delta=0.4, want_history=True)
    miss = total = 0
    for c in range(C):
        for t in range(1, T):
            w = L.normalize(hist["log_ws"][c, t - 1])
            ref = L.multinomial(nz["u_res"][c, t - 1], w)
            got = hist["As"][c, t - 1]
            bad = np.nonzero(ref != got)[0]
            total += N - 1
            miss += bad.size
            for i in bad:  # a miss sits at a boundary: only zero-weight particles between the two picks
                lo, hi = sorted((int(ref[i]), int(got[i])))
                assert np.all(w[lo + 1:hi] == 0) or hi - lo == 1
    assert miss / total <= 2e-4, (miss, total)


# ---- ground truth ----------------------------------------------------------------------------------------------------------------------------------------
def test_rare_event_particle_gibbs_matches_the_kalman_smoother():
    """independent auxiliary particle Gibbs (resident chains, Threefry keys) on the rare-event model: posterior means and variances at several t within
    5 Monte Carlo standard errors of the exact Gaussian posterior (AR(1) prior with unit marginals, one observation y ~ N(x_{T-1}, r^2))"""
    from aux_ssm_samplers_amd import _lib, random as R
    from aux_ssm_samplers_amd.csmc import CsmcChains, CSMCState, DevicePotential, DeviceGaussianDynamics, GaussianInit, get_independent_kernel
    T, rho, r2, yv = 12, 0.9, 0.25, 2.0
    C, N, burn, iters = 1024, 256, 60, 240
    th = [T, yv, np.sqrt(r2)]
    M0 = GaussianInit(m0=[0.0], P0=[[1.0]])
    Mt = DeviceGaussianDynamics(U.RARE_EVENT, Q=[[1 - rho ** 2]], theta=[rho])
    _, kern = get_independent_kernel(M0, DevicePotential(U.RARE_EVENT, theta=th), Mt, DevicePotential(U.RARE_EVENT, theta=th), N, True, Mt)
    S = rho ** np.abs(np.subtract.outer(np.arange(T), np.arange(T)))
    k = S[:, -1] / (S[-1, -1] + r2)
    mean_true, var_true = k * yv, np.diag(S) - k * S[-1, :]
    h = _lib.default_handle()
    chains = CsmcChains(h, np.zeros((C, T, 1)), delta=1.0, dtype=np.float64)
    state = CSMCState(x=chains, updated=None)
    s1, s2 = np.zeros((C, T)), np.zeros((C, T))
    for it in range(burn + iters):
        state = kern(R.PRNGKey(1000 + it), state, None)
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
    assert mean_true[-1] > 1.5  # (the observation moves the end of the path well away from the prior)
