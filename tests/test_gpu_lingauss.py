"""The linear-Gaussian observation potential (AUXSSM_POT_LIN_GAUSS, csmc.LinearGaussianPotential) on the GPU, through every kernel family: the register kernels
(dx <= 4), the wide kernels (4 < dx <= 32, N <= 64), the parallel-in-time sweep, gradient and guided proposals, resident chains.

1. Built-in kind 5 against the same potential as a user program (device_models.BUILTIN_LINGAUSS[_GRAD]), bit for bit, dx <= 4, fp32 and fp64.
2. Literal parity in fp64 on explicit noise against oracle/csmc_np.py on the objects of tests/lingauss_np.py: resampling ancestors and backward indices identical,
   particles within 1e-12, log-weights within 1e-10 (the bars of tests/test_gpu_csmc_literal.py).  tests/test_lingauss_potential.py shows on the literal alone
   that no draw of these cases lies within 1e-8 of a cumulative-sum edge: an index mismatch here is a defect, never a tie.
3. fp32 by the teacher-forced tie-rate rule of tests/test_gpu_csmc_literal.py, on the wide and on the register path.
4. The parallel-in-time sweep against the literal tree of oracle/pit_np.py (fp64), keyed against explicit noise (fp32).
5. Resident chains.
6. Ground truth: the whole model is linear-Gaussian, so the posterior is a dense joint Gaussian known exactly at any dimension (tests/lingauss_np.py::
   exact_posterior) -- the first check of the wide kernels against truth at dx > 4.
7. The C entry points' refusals."""
import ctypes as C

import numpy as np
import numpy.testing as npt
import pytest

from oracle import csmc_np as L
from tests import lingauss_np as LG
from tests import pit_cases as PC

pytestmark = pytest.mark.gpu


def _gmode(gradient):
    from aux_ssm_samplers_amd import _lib
    return _lib.GRAD_NONE if not gradient else (_lib.GRAD_EXACT if gradient == "exact" else _lib.GRAD_REFERENCE)


def _describe(style, dev, gradient=False):
    from aux_ssm_samplers_amd.csmc import _device
    M0, G0, Mt, Gt = dev
    if style == "bootstrap":
        return _device.describe_bootstrap(M0, G0, Mt, Gt, Mt)
    if style == "guided":
        return _device.describe_guided(M0, G0, Mt, Gt, Mt, _gmode(gradient))
    return _device.describe_independent(M0, G0, Mt, Gt, Mt, _gmode(gradient))


def _noise(Cn, T, N, d, rng, dtype=np.float64):
    nz = dict(eps_aux=rng.standard_normal((Cn, T, d)), eps_prop=rng.standard_normal((Cn, T, N, d)), u_res=rng.random((Cn, T - 1, N)), u_bwd=rng.random((Cn, T)))
    return {k: v.astype(dtype) for k, v in nz.items()}


# ---- 1. the built-in against the program ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,dy,N,T,Cn", LG.PROGRAM_SHAPES)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_builtin_potential_equals_the_user_program_bit_for_bit(dtype, d, dy, N, T, Cn):
    """bootstrap and independent proposals, gradient False / True / "exact", both backward modes, explicit and Threefry noise; two observation rows carry a NaN,
    c != 0; every case moves the trajectory"""
    from aux_ssm_samplers_amd import random as R
    from aux_ssm_samplers_amd.csmc import _device
    rng = np.random.default_rng(100 * d + N)
    dev, m, xtrue, delta = LG.case(d, dy, T, rng, nan_rows=(3, T - 2))
    assert np.all(m.c != 0) and np.isnan(m.y).any(axis=1).sum() == 2
    x0 = (xtrue[None] + 0.3 * rng.standard_normal((Cn, T, d))).astype(dtype)
    nz = _noise(Cn, T, N, d, rng, dtype)
    for style, gradient in (("bootstrap", False), ("independent", False), ("independent", True), ("independent", "exact")):
        fb, fu = _describe(style, dev, gradient), _describe(style, LG.program(dev, bool(gradient)), gradient)
        assert fb.potential == 5 and fb.user is None and fu.user is not None
        for backward in (False, True):
            for keyed in (False, True):
                kw = dict(key=R.PRNGKey(31 + d)) if keyed else dict(noise=nz)
                xb, ab, hb = _device.sweep(fb, x0, N, backward, delta=delta, want_history=True, **kw)
                xu, au, hu = _device.sweep(fu, x0, N, backward, delta=delta, want_history=True, **kw)
                npt.assert_array_equal(ab, au)
                npt.assert_array_equal(xb, xu)
                for name in ("xs", "log_ws", "As"):
                    npt.assert_array_equal(hb[name], hu[name])
                assert xb.dtype == dtype and np.all(np.isfinite(hb["log_ws"])) and (ab != 0).any(), (style, gradient, backward, keyed)


# ---- 2. literal parity -----------------------------------------------------------------------------------------------------------------------------------
def _against_literal(style, gradient, backward, name):
    """one fp64 sweep on explicit noise next to the literal sampler; returns (ancestors, max particle error, max log-weight error)"""
    from aux_ssm_samplers_amd.csmc import _device
    (xl, Bl, lh), (d, N, T, dev, m, x0, delta, nz) = LG.literal_sweep(style, gradient, backward, name)
    assert np.all(np.isnan(m.y[[0, T // 2, T - 1]]).any(axis=1))
    nz = {k: v[None] for k, v in nz.items() if not (style == "bootstrap" and k == "eps_aux")}
    fk = _describe(style, dev, gradient)
    assert fk.potential == 5 and fk.user is None
    x, anc, hist = _device.sweep(fk, x0, N, backward, noise=nz, delta=None if style == "bootstrap" else delta, want_history=True)
    ex, el = float(np.max(np.abs(hist["xs"] - lh["xs"]))), float(np.max(np.abs(hist["log_ws"] - lh["log_ws"])))
    print(f"{style} gradient={gradient} backward={backward} {name} (d={d} dy={m.H.shape[0]} N={N} T={T}): max |xs - literal| = {ex:.1e}, "
          f"max |log_ws - literal| = {el:.1e}, updated {int((anc != 0).sum())} of {T}")
    npt.assert_array_equal(hist["As"], lh["As"])
    npt.assert_array_equal(anc, Bl)
    npt.assert_allclose(x, xl, rtol=1e-12, atol=1e-12)
    npt.assert_allclose(hist["xs"], lh["xs"], rtol=1e-12, atol=1e-12)
    lw_lit = lh["log_ws"]
    if style == "independent" and gradient is True:
        # the reference's weighting: GradientAuxiliaryGt adds its correction summed over ALL particles (csmc/independent.py:265-266), one constant per step that
        # cancels in every normalisation and that the device does not add (include/auxssm.h, AUXSSM_GRAD_REFERENCE): compared up to that constant, read off particle 0
        lw_lit = lw_lit - (lw_lit[:, :1] - hist["log_ws"][:, :1])
        el = float(np.max(np.abs(hist["log_ws"] - lw_lit)))
        print(f"    up to the reference's per-step constant: max |log_ws - literal| = {el:.1e}")
    npt.assert_allclose(hist["log_ws"], lw_lit, rtol=1e-10, atol=1e-10)
    assert np.all(hist["As"][:, 0] == 0) and np.array_equal(hist["xs"][:, 0], x0)  # row 0 of every step is the reference trajectory
    if style == "independent" and not gradient:
        # the direct identity: the stored log-weights are log g_t + log initial / log transition themselves (the kernels store them before any shift)
        for t in range(T):
            g = LG.log_g(hist["xs"][t], m.y[t], m.H, m.R, m.c)
            if t == 0:
                dens = L._mvn_chol_logpdf(hist["xs"][0], m.m0, m.LP0)
            else:
                dens = L._mvn_chol_logpdf(hist["xs"][t], hist["xs"][t - 1][hist["As"][t - 1]] @ m.F.T + m.b, m.LQ)
            npt.assert_allclose(hist["log_ws"][t], g + dens, rtol=1e-10, atol=1e-10)
    return anc, ex, el


@pytest.mark.parametrize("style,gradient,backward", LG.LITERAL_CELLS)
def test_sweep_fp64_equals_the_literal_sampler(style, gradient, backward):
    """register and wide path; a single case may update nothing, over the set every (style, gradient, backward) cell moves the trajectory somewhere"""
    moved = 0
    for name in LG.REGISTER + LG.WIDE:
        moved += int((_against_literal(style, gradient, backward, name)[0] != 0).sum())
    assert moved > 0


@pytest.mark.parametrize("backward", [False, True])
@pytest.mark.parametrize("name", LG.BOOTSTRAP_CASES)
def test_bootstrap_sweep_fp64_equals_the_literal_sampler(name, backward):
    anc, _, _ = _against_literal("bootstrap", False, backward, name)
    assert (anc != 0).any()


# ---- 3. fp32 tie rate --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dx,dy,N,T,style", [(24, 12, 25, 250, "independent"), (24, 12, 25, 250, "guided"), (4, 2, 64, 1000, "independent")])
def test_fp32_ancestors_against_the_literal_order_tie_rate(dx, dy, N, T, style):
    """the tracking workload on the wide path (dx = 24, dy = 12, which no contract oracle covers in fp32) and on the register path (dx = 4, dy = 2), 4 chains: the
    literal left-to-right draw on the device's own stored fp32 log-weights (tests/test_gpu_csmc_literal.py's rule): disagreeing draws <= 2e-4 of all draws, none
    farther than one visible particle"""
    from aux_ssm_samplers_amd.csmc import _device
    from aux_ssm_samplers_amd.workloads import lgssm_tracking_setup
    from tests.test_gpu_guided import _tie_rate
    Cn = 4
    rng = np.random.default_rng(77)
    M0, Mt, G0, Gt, xtrue, y, H, R = lgssm_tracking_setup(T, dx, dy, seed=3)
    x0 = (xtrue[None] + 0.3 * rng.standard_normal((Cn, T, dx))).astype(np.float32)
    nz = _noise(Cn, T, N, dx, rng, np.float32)
    _, _, hist = _device.sweep(_describe(style, (M0, G0, Mt, Gt)), x0, N, False, noise=nz, delta=0.1, want_history=True)
    assert hist["log_ws"].dtype == np.float32 and np.all(np.isfinite(hist["log_ws"]))
    bad, tot, far = _tie_rate(hist, nz["u_res"])
    print(f"{style} dx={dx} dy={dy} N={N} T={T}: {bad} of {tot} fp32 draws differ from the literal order ({bad / tot:.2e}), {far} farther than one visible particle")
    assert bad / tot <= 2e-4, (bad, tot)
    assert far == 0


# ---- 4. parallel in time ---------------------------------------------------------------------------------------------------------------------------------
PIT_CELLS = [(1, 1, 32, 25), (3, 2, 100, 33), (3, 1, 32, 33), (1, 1, 100, 25), (3, 2, 32, 25)]  # (d, dy, N, T)


class _PitCase(PC._Sides):
    """tests/pit_cases.py's sides of one cell on tests/lingauss_np.py's objects: flat steps at t = 0, on the top-level stitch boundary and at the last step"""

    def __init__(self, d, dy, N, T, gradient):
        self.d, self.N, self.T, self.gradient = d, N, T, bool(gradient)
        rng = np.random.default_rng([11, d, dy, N, T, int(gradient)])
        self.dev, self.m, xtrue, self.delta = LG.case(d, dy, T, rng, nan_rows=(0, PC.top_boundary(T), T - 1))
        self.x0 = xtrue + 0.3 * rng.standard_normal((T, d))
        self.noise = dict(eps_aux=rng.standard_normal((T, d)), eps_prop=rng.standard_normal((T, N, d)), u_res=rng.random((T, N)))

    def literal_objects(self):
        return self.m.literal()

    def joint_grad(self, u):
        return LG.joint_grad(self.m, u)

    def device_objects(self):
        return self.dev


@pytest.mark.parametrize("gradient", [False, True])
@pytest.mark.parametrize("d,dy,N,T", PIT_CELLS)
def test_pit_sweep_fp64_equals_the_literal_tree(d, dy, N, T, gradient):
    """origins identical, trajectory within 1e-12, after the margin condition of tests/pit_cases.margin_threshold on the literal"""
    from aux_ssm_samplers_amd.csmc import _device
    c = _PitCase(d, dy, N, T, gradient)
    xl, origins, hist = c.literal_sweep()
    threshold = PC.margin_threshold(N)
    print(f"d={d} dy={dy} N={N} T={T} gradient={gradient}: smallest draw margin {hist['min_margin']:.2e} (threshold {threshold:.2e})")
    assert hist["min_margin"] >= threshold
    fk = c.device_model()
    assert fk.potential == 5 and fk.user is None
    x, anc = _device.pit_sweep(fk, c.x0, N, noise={k: v[None] for k, v in c.noise.items()}, delta=c.delta)
    print(f"    {int((anc != origins).sum())} of {T} origins differ, max |x - literal| = {float(np.max(np.abs(x - xl))):.1e}, {int((origins != 0).sum())} steps updated")
    assert x.dtype == np.float64
    npt.assert_array_equal(anc[0] if anc.ndim == 2 else anc, origins)
    npt.assert_allclose(x[0] if x.ndim == 3 else x, xl, rtol=1e-12, atol=1e-12)
    assert (origins != 0).any()


@pytest.mark.parametrize("gradient", [False, True])
@pytest.mark.parametrize("d,dy,N,T", PIT_CELLS)
def test_pit_sweep_fp32_keyed_equals_explicit_noise(d, dy, N, T, gradient):
    from aux_ssm_samplers_amd import _lib, random as R
    from aux_ssm_samplers_amd.csmc import _device
    dtype, Cn, delta = np.float32, 3, 0.4
    c = _PitCase(d, dy, N, T, gradient)
    fk = c.device_model()
    x0 = c.chains(Cn, 1)[0].astype(dtype)
    h, key = _lib.default_handle(), R.PRNGKey(5 + d)
    noise = PC.keyed_noise(lambda s, shape: h.rng_normal(key, s, shape, dtype).to_host(), lambda s, shape: h.rng_uniform(key, s, shape, dtype).to_host(), Cn, T, N, d)
    x, anc = _device.pit_sweep(fk, x0, N, noise=noise, delta=delta)
    xk, anck = _device.pit_sweep(fk, x0, N, key=key, delta=delta)
    npt.assert_array_equal(x, xk)
    npt.assert_array_equal(anc, anck)
    assert x.dtype == dtype and np.isfinite(x).all() and anc.min() >= 0 and anc.max() < N and (anc != 0).mean() > 0.2
    npt.assert_array_equal(x[anc == 0], x0[anc == 0])


# ---- 5. resident chains ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,dy,N,T,style", [(3, 2, 100, 33, "independent"), (3, 2, 100, 33, "guided"), (3, 2, 100, 33, "pit"),
                                            (9, 4, 25, 20, "independent"), (9, 4, 25, 20, "guided")])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_resident_chains_equal_host_state_sweeps(dtype, d, dy, N, T, style):
    """three sweeps on CsmcChains equal three host-state sweeps with the same keys, bit for bit: independent proposals with the exact gradient weighting, guided
    proposals with gradient, parallel in time (register kernels only: dx <= 4)"""
    from aux_ssm_samplers_amd import _lib, random as R
    from aux_ssm_samplers_amd.csmc import CsmcChains, CSMCState, get_guided_kernel, get_independent_kernel
    rng = np.random.default_rng(5 + d)
    dev, m, xtrue, delta = LG.case(d, dy, T, rng, nan_rows=(1,))
    Cn = 4
    x0 = (xtrue[None] + 0.3 * rng.standard_normal((Cn, T, d))).astype(dtype)
    if style == "guided":
        init, kern = get_guided_kernel(*dev, N, backward=True, gradient=True)
    else:
        init, kern = get_independent_kernel(*dev, N, backward=True, gradient="exact", parallel=style == "pit")
    chains = CsmcChains(_lib.default_handle(), x0, delta=delta, dtype=dtype)
    rs, hs = CSMCState(x=chains, updated=None), init(x0)
    for it in range(3):
        rs, hs = kern(R.PRNGKey(40 + it), rs, None), kern(R.PRNGKey(40 + it), hs, delta)
    assert hs.x.dtype == dtype and (hs.ancestors != 0).any()
    npt.assert_array_equal(chains.to_host(), hs.x)
    npt.assert_array_equal(chains.ancestors.to_host(), hs.ancestors)


# ---- 6. ground truth: the exact Gaussian posterior ---------------------------------------------------------------------------------------------------------
_models = {}


def _truth_model(which):
    """(a) register: dx = 2, dy = 1, T = 6, F = [[1, 0.3], [0, 0.9]], H = [[1, 0.5]];  (b) wide: dx = 6, dy = 3, T = 5, a banded F, dense H, non-diagonal R.
    Returns (device objects, Model, the same Model with the coupling entries of H zeroed -- in (a) the 0.5, in (b) everything off H's diagonal); built once"""
    if which not in _models:
        rng = np.random.default_rng(2024)
        if which == "a":
            d, T = 2, 6
            F, H, R, c = np.array([[1.0, 0.3], [0.0, 0.9]]), np.array([[1.0, 0.5]]), np.array([[0.5]]), np.array([0.2])
            Q, P0, m0, b = np.diag([0.4, 0.3]), np.eye(2), np.zeros(2), np.array([0.05, -0.05])
            H0 = np.array([[1.0, 0.0]])
        else:
            d, T = 6, 5
            F = 0.8 * np.eye(d) + 0.1 * np.eye(d, k=1) - 0.1 * np.eye(d, k=-1)
            H, R, c = LG.observation(d, 3, rng)
            H = H + 0.6 * np.eye(3, d)
            Q, P0, m0, b = 0.3 * np.eye(d), np.eye(d), np.zeros(d), 0.05 * np.ones(d)
            H0 = H * np.eye(3, d)
            assert np.max(np.abs(R - np.diag(np.diag(R)))) > 0.05 and np.all(H != 0)
        x = np.zeros((T, d))
        x[0] = rng.standard_normal(d)
        for t in range(1, T):
            x[t] = F @ x[t - 1] + b + np.linalg.cholesky(Q) @ rng.standard_normal(d)
        y = x @ H.T + c + rng.standard_normal((T, H.shape[0])) @ np.linalg.cholesky(R).T
        dev, m = LG.build(m0, P0, F, b, Q, H, R, c, y)
        _models[which] = (dev, m, LG.build(m0, P0, F, b, Q, H0, R, c, y)[1])
    return _models[which]


def _moments(m):
    """(E x_t, E x_t x_t^T) of the exact posterior, shapes (T, d) and (T, d, d)"""
    T, d = m.y.shape[0], m.m0.shape[0]
    mean, cov = LG.exact_posterior(m)
    mean = mean.reshape(T, d)
    return mean, np.stack([cov[t * d:(t + 1) * d, t * d:(t + 1) * d] + np.outer(mean[t], mean[t]) for t in range(T)])


def _kernel(sampler, dev, N):
    from aux_ssm_samplers_amd._primitives.csmc import get_kernel as get_bootstrap_kernel
    from aux_ssm_samplers_amd.csmc import get_guided_kernel, get_independent_kernel
    if sampler == "bootstrap":
        return get_bootstrap_kernel(*dev, N, backward=True, Pt=dev[2])[1]
    if sampler.startswith("guided"):
        return get_guided_kernel(*dev, N, backward=True, gradient=sampler.endswith("gradient"))[1]
    if sampler.startswith("pit"):
        return get_independent_kernel(*dev, N, gradient=sampler.endswith("gradient"), parallel=True)[1]
    return get_independent_kernel(*dev, N, backward=sampler != "independent-trace", Pt=dev[2], gradient="exact" if sampler == "exact" else False)[1]


_CASES6 = ([("a", s) for s in ("independent-trace", "independent-backward", "exact", "guided", "guided-gradient", "bootstrap", "pit", "pit-gradient")]
           + [("b", s) for s in ("independent-backward", "exact", "guided", "guided-gradient")])


@pytest.mark.parametrize("which,sampler", _CASES6)
def test_particle_gibbs_matches_the_exact_gaussian_posterior(which, sampler):
    """1024 resident chains: every posterior mean and second moment (cross moments of a step included) within 5 empirical standard errors of the exact value -- the
    standard error is the standard deviation of the per-chain time averages over sqrt(chains), the rule of tests/test_gpu_posterior_quadrature.py.  Power: the
    exact posterior with the coupling entries of H zeroed lies more than 10 of the same standard errors away in at least one compared moment."""
    from tests.test_gpu_mvt import _gibbs_moments
    dev, m, m_zeroed = _truth_model(which)
    T, d = m.y.shape[0], m.m0.shape[0]
    # the step size, from the model alone: the gradient proposals N(u + delta/2 grad, delta/2 I) are one Langevin step, which on a Gaussian target with joint
    # precision J contracts towards the mode only while delta/2 lambda_max(J) < 2 and lands on it along the stiffest direction at delta = 2 / lambda_max(J); a
    # larger delta leaves every sampler valid but the gradient ones overshoot and 60 sweeps of burn-in no longer forget the start.  All samplers of a case share it.
    N = 16 if which == "a" else 32
    delta = min(0.6 if which == "a" else 0.3, 2.0 / float(np.linalg.eigvalsh(np.linalg.inv(LG.exact_posterior(m)[1])).max()))
    m1, se1, m2, se2 = _gibbs_moments(_kernel(sampler, dev, N), T, d, delta, 2000 if which == "a" else 3000, with_delta=sampler != "bootstrap")
    t1, t2 = _moments(m)
    w1, w2 = _moments(m_zeroed)
    z1, z2 = np.abs(m1 - t1) / se1, np.abs(m2 - t2) / se2
    p1, p2 = np.abs(w1 - t1) / se1, np.abs(w2 - t2) / se2
    print(f"({which}) {sampler}: worst z of the means {z1.max():.2f}, of the second moments {z2.max():.2f}; the posterior with H's coupling zeroed lies "
          f"{max(p1.max(), p2.max()):.0f} standard errors away")
    assert max(p1.max(), p2.max()) > 10
    assert z1.max() < 5 and z2.max() < 5


# ---- 7. the C entry points --------------------------------------------------------------------------------------------------------------------------------
def test_c_entry_points_refuse_a_missing_observation_matrix_and_missing_observations():
    from aux_ssm_samplers_amd import _lib
    from aux_ssm_samplers_amd.csmc import _device
    h = _lib.default_handle()
    T, N, d, dt = 6, 64, 2, np.float64
    dev, m, xtrue, _ = LG.case(d, 1, T, np.random.default_rng(0))
    fk = _device.describe_independent(dev[0], dev[1], dev[2], dev[3], dev[2])
    x, anc, shd = h.to_device(np.zeros((1, T, d)), dt), h.zeros((1, T), np.int32), h.to_device(np.full(T, 0.5), dt)
    nz = _lib.CsmcNoise()
    nz.mode, nz.key0, nz.key1 = _lib.NOISE_THREEFRY, 1, 2
    tail = (1, T, N, 1, shd.ptr, x.ptr, C.byref(nz), anc.ptr, None, None, None)
    for field, msg in (("obs_H", "obs_H"), ("y", "observations y")):
        ms = fk.struct(h, dt, T)
        assert ms.potential == 5
        setattr(ms, field, None)
        assert h.lib.auxssm_csmc_sweep(h.h, _lib.dtype_code(dt), C.byref(ms), *tail) == _lib.ERR_ARG
        assert msg in h.lib.auxssm_last_error().decode()
        assert h.lib.auxssm_csmc_pit_sweep(h.h, _lib.dtype_code(dt), C.byref(ms), 1, T, N, shd.ptr, x.ptr, C.byref(nz), anc.ptr) == _lib.ERR_ARG
        assert msg in h.lib.auxssm_last_error().decode()
    ms = fk.struct(h, dt, T)
    assert h.lib.auxssm_csmc_sweep(h.h, _lib.dtype_code(dt), C.byref(ms), *tail) == 0  # and the untampered description runs
    assert h.lib.auxssm_csmc_pit_sweep(h.h, _lib.dtype_code(dt), C.byref(ms), 1, T, N, shd.ptr, x.ptr, C.byref(nz), anc.ptr) == 0
