"""The logistic potential (AUXSSM_POT_LOGISTIC, csmc.BinomialPotential / NegBinomialPotential) on the GPU, through every kernel family: the register kernels
(dx <= 4), the wide kernels (4 < dx <= 32, N <= 64), the parallel-in-time sweep at both widths, gradient and guided proposals, bootstrap, resident chains.  Both
families go through every group (tests/logistic_np.py::family_of alternates them over the shapes); the data of every case hold a missing entry, a wholly
missing row, y = 0, y = trials and a size of 1.

1. Built-in kind 8 against the same potential as a user program (device_models.BUILTIN_LOGISTIC over rows [y | m]), bit for bit, dx <= 4, fp32 and fp64; and a
   cell with sizes >= 1000 started at |x| = 30, whose log-weights must be finite.
2. Literal parity in fp64 on explicit noise against oracle/csmc_np.py / tests/guided_np.py on the objects of tests/logistic_np.py: resampling ancestors and
   backward indices identical, particles within 1e-12, log-weights within 1e-10 (sizes <= 40).  tests/test_logistic_potential.py shows on the literal alone that no
   draw of these cases lies within 1e-8 of a cumulative-sum edge: an index mismatch here is a defect, never a tie.
3. The parallel-in-time sweep against the literal tree of oracle/pit_np.py (fp64, register and wide), keyed against explicit noise (fp32).
4. fp32 by the teacher-forced tie-rate rule of tests/test_gpu_guided.py, on the wide and on the register path; the distance of the fp32 log-weights from the
   fp64 sweep on the same noise is printed (no bar is set on it).
5. Resident chains; and fp32 with more chains than CUs (the eight-wave wide kernels) against the sixteen-wave launches.
6. Ground truth: the posterior of the scalar model by quadrature (tests/logistic_np.py::posterior_by_quadrature); with diagonal F, Q and P0 the components of a
   d = 6 model are independent, so every marginal is its own quadrature answer.
7. The C entry points' refusals."""
import ctypes as C

import numpy as np
import numpy.testing as npt
import pytest

from oracle import csmc_np as L
from tests import pit_cases as PC
from tests import logistic_np as LN

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


def _assert_program_equality(dev, x0, N, delta, nz, key, styles):
    """every (style, gradient) x backward mode x noise mode: the built-in sweep equals the program's, bit for bit; returns the log-weights seen"""
    from aux_ssm_samplers_amd.csmc import _device
    prog = LN.program(dev)
    seen = []
    for style, gradient in styles:
        fb, fu = _describe(style, dev, gradient), _describe(style, prog, gradient)
        assert fb.potential == 8 and fb.user is None and fu.user is not None
        for backward in (False, True):
            for keyed in (False, True):
                kw = dict(key=key) if keyed else dict(noise=nz)
                xb, ab, hb = _device.sweep(fb, x0, N, backward, delta=delta, want_history=True, **kw)
                xu, au, hu = _device.sweep(fu, x0, N, backward, delta=delta, want_history=True, **kw)
                npt.assert_array_equal(ab, au)
                npt.assert_array_equal(xb, xu)
                for name in ("xs", "log_ws", "As"):
                    npt.assert_array_equal(hb[name], hu[name])
                assert xb.dtype == x0.dtype and np.all(np.isfinite(hb["log_ws"])), (style, gradient, backward, keyed)
                seen.append((style, gradient, backward, keyed, ab, hb["log_ws"]))
    return seen


_STYLES1 = (("bootstrap", False), ("independent", False), ("independent", True), ("independent", "exact"))


# ---- 1. the built-in against the program ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,N,family", [(d, N, LN.FAMILIES[i % 2]) for i, (d, N) in enumerate(LN.PROGRAM_SHAPES)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_builtin_potential_equals_the_user_program_bit_for_bit(dtype, d, N, family):
    """bootstrap and independent proposals, gradient False / True / "exact", backward sampling and ancestor tracing, explicit and Threefry noise; ancestors,
    trajectories, particles, log-weights and resampling indices are compared; the two families alternate over the shapes (every d and every N meets both)"""
    from aux_ssm_samplers_amd import random as R
    T, Cn = LN.PROGRAM_T, LN.PROGRAM_CHAINS
    rng = np.random.default_rng(100 * d + N)
    dev, m, xtrue, delta = LN.case(d, T, rng, family, nan_steps=(3, T // 2, T - 2))
    assert np.isnan(m.y).any(axis=1).sum() == 3 and np.isnan(m.y[T // 2]).all() and LN.has_every_feature(m)
    x0 = (xtrue[None] + 0.3 * rng.standard_normal((Cn, T, d))).astype(dtype)
    nz = _noise(Cn, T, N, d, rng, dtype)
    seen = _assert_program_equality(dev, x0, N, delta, nz, R.PRNGKey(31 + d), _STYLES1)
    assert all((s[4] != 0).any() for s in seen)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_large_sizes_and_a_far_start_keep_the_log_weights_finite(dtype):
    """trials in 1000 .. 5000 and a reference trajectory at x = +30 / -30 (alternating over the components): e = det_exp(-|x|) cannot overflow, so every stored
    log-weight is finite -- and the sweep still equals the user program's bit for bit"""
    from aux_ssm_samplers_amd import csmc, random as R
    d, N, T, Cn = 2, 100, 12, 2
    rng = np.random.default_rng(8)
    trials = rng.integers(1000, 5001, size=(T, d)).astype(np.float64)
    y = rng.binomial(trials.astype(np.int64), 0.5).astype(np.float64)
    y[3, 0], y[4, 0], y[5, :] = 0.0, trials[4, 0], np.nan
    M0, Mt = csmc.GaussianInit(m0=np.zeros(d), P0=np.eye(d)), csmc.LinearGaussianDynamics(F=0.9 * np.eye(d), b=np.zeros(d), Q=0.1 * np.eye(d))
    dev = (M0, csmc.BinomialPotential(trials[0], y=y[0]), Mt, csmc.BinomialPotential(trials[1:], params=y[1:]))
    x0 = np.broadcast_to(np.array([30.0, -30.0]), (Cn, T, d)).astype(dtype)
    seen = _assert_program_equality(dev, x0, N, 1e-4, _noise(Cn, T, N, d, rng, dtype), R.PRNGKey(3), _STYLES1)
    assert max(float(np.abs(s[5]).max()) for s in seen) > 1e4  # (log-weights of order m |x|: far from the mode, and finite)


@pytest.mark.parametrize("family", LN.FAMILIES)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_user_mean_program_keeps_the_builtin_potential(dtype, family):
    """a program that supplies only the transition mean (device_models.BUILTIN_LINEAR_MEAN_VJP, the built-in mean as user source) evaluates kind 8 through
    potential_rt / potential_grad_rt inside the program's kernels, the sizes loaded from plane 1 at run time: the same sweep as the closed family, bit for bit"""
    from aux_ssm_samplers_amd.csmc import _device, DeviceGaussianDynamics, device_models as U
    d, N, T, Cn = 3, 100, 24, 3
    rng = np.random.default_rng(12)
    dev, m, xtrue, delta = LN.case(d, T, rng, family, nan_steps=(2, T // 2, T - 1))
    M0, G0, Mt, Gt = dev
    Mu = DeviceGaussianDynamics(U.BUILTIN_LINEAR_MEAN_VJP, Q=Mt.Q, theta=np.concatenate([np.reshape(Mt.F, -1), Mt.b]))
    x0 = (xtrue[None] + 0.3 * rng.standard_normal((Cn, T, d))).astype(dtype)
    nz = _noise(Cn, T, N, d, rng, dtype)
    for gradient in (False, "exact"):
        fb, fu = _describe("independent", dev, gradient), _describe("independent", (M0, G0, Mu, Gt), gradient)
        assert fb.potential == fu.potential == 8 and fb.user is None and fu.user is not None
        for backward in (False, True):
            xb, ab, hb = _device.sweep(fb, x0, N, backward, delta=delta, want_history=True, noise=nz)
            xu, au, hu = _device.sweep(fu, x0, N, backward, delta=delta, want_history=True, noise=nz)
            npt.assert_array_equal(ab, au)
            npt.assert_array_equal(xb, xu)
            for name in ("xs", "log_ws", "As"):
                npt.assert_array_equal(hb[name], hu[name])
            assert (ab != 0).any()


# ---- 2. literal parity -----------------------------------------------------------------------------------------------------------------------------------
def _against_literal(style, gradient, backward, shape):
    """one fp64 sweep on explicit noise next to the literal sampler; returns the ancestors"""
    from aux_ssm_samplers_amd.csmc import _device
    (xl, Bl, lh), (d, N, T, dev, m, x0, delta, nz), gap, bump = LN.literal_sweep(style, gradient, backward, shape)
    assert gap >= LN.GAP_BAR
    nz = {k: v[None] for k, v in nz.items() if not (style == "bootstrap" and k == "eps_aux")}
    fk = _describe(style, dev, gradient)
    assert fk.potential == 8 and fk.user is None
    x, anc, hist = _device.sweep(fk, x0, N, backward, noise=nz, delta=None if style == "bootstrap" else delta, want_history=True)
    ex, el = float(np.max(np.abs(hist["xs"] - lh["xs"]))), float(np.max(np.abs(hist["log_ws"] - lh["log_ws"])))
    print(f"{LN.family_of(shape)} {style} gradient={gradient} backward={backward} d={d} N={N} T={T}: max |xs - literal| = {ex:.1e}, max |log_ws - literal| = {el:.1e}, "
          f"updated {int((anc != 0).sum())} of {T}, smallest draw gap {gap:.1e}")
    npt.assert_array_equal(hist["As"], lh["As"])
    npt.assert_array_equal(anc, Bl)
    npt.assert_allclose(x, xl, rtol=1e-12, atol=1e-12)
    npt.assert_allclose(hist["xs"], lh["xs"], rtol=1e-12, atol=1e-12)
    lw_lit = lh["log_ws"]
    if style == "independent" and gradient is True:
        # the reference's weighting: GradientAuxiliaryGt adds its correction summed over ALL particles (csmc/independent.py:265-266), one constant per step that
        # cancels in every normalisation and that the device does not add (include/auxssm.h, AUXSSM_GRAD_REFERENCE): compared up to that constant, read off particle 0
        lw_lit = lw_lit - (lw_lit[:, :1] - hist["log_ws"][:, :1])
        print(f"    up to the reference's per-step constant: max |log_ws - literal| = {float(np.max(np.abs(hist['log_ws'] - lw_lit))):.1e}")
    npt.assert_allclose(hist["log_ws"], lw_lit, rtol=1e-10, atol=1e-10)
    assert np.all(hist["As"][:, 0] == 0) and np.array_equal(hist["xs"][:, 0], x0)  # row 0 of every step is the reference trajectory
    if style == "independent" and not gradient:
        # the direct identity: the stored log-weights are log g_t + log initial / log transition themselves (the kernels store them before any shift)
        for t in range(T):
            g = LN.log_g(hist["xs"][t], m.y[t], m.size[t])
            if t == 0:
                dens = L._mvn_chol_logpdf(hist["xs"][0], m.m0, m.LP0)
            else:
                dens = L._mvn_chol_logpdf(hist["xs"][t], hist["xs"][t - 1][hist["As"][t - 1]] @ m.F.T + m.b, m.LQ)
            npt.assert_allclose(hist["log_ws"][t], g + dens, rtol=1e-10, atol=1e-10)
    return anc


@pytest.mark.parametrize("style,gradient,backward", LN.LITERAL_CELLS)
def test_sweep_fp64_equals_the_literal_sampler(style, gradient, backward):
    """register and wide path; a single case may update nothing, over the set every (style, gradient, backward) cell moves the trajectory somewhere"""
    moved = 0
    for shape in LN.REGISTER + LN.WIDE:
        moved += int((_against_literal(style, gradient, backward, shape) != 0).sum())
    assert moved > 0


# ---- 3. parallel in time ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gradient", [False, True])
@pytest.mark.parametrize("d,N,T", LN.PIT_CELLS)
def test_pit_sweep_fp64_equals_the_literal_tree(d, N, T, gradient):
    """origins identical, trajectory within 1e-12, after the margin condition of tests/pit_cases.margin_threshold on the literal"""
    from aux_ssm_samplers_amd.csmc import _device
    c, (xl, origins, hist) = LN.pit_literal(d, N, T, gradient)
    threshold = PC.margin_threshold(N)
    print(f"{LN.family_of((d, N, T))} d={d} N={N} T={T} gradient={gradient}: smallest draw margin {hist['min_margin']:.2e} (threshold {threshold:.2e})")
    assert hist["min_margin"] >= threshold
    fk = c.device_model()
    assert fk.potential == 8 and fk.user is None
    x, anc = _device.pit_sweep(fk, c.x0, N, noise={k: v[None] for k, v in c.noise.items()}, delta=c.delta)
    print(f"    {int((anc != origins).sum())} of {T} origins differ, max |x - literal| = {float(np.max(np.abs(x - xl))):.1e}, {int((origins != 0).sum())} steps updated")
    assert x.dtype == np.float64
    npt.assert_array_equal(anc[0] if anc.ndim == 2 else anc, origins)
    npt.assert_allclose(x[0] if x.ndim == 3 else x, xl, rtol=1e-12, atol=1e-12)
    assert (origins != 0).any()


@pytest.mark.parametrize("gradient", [False, True])
@pytest.mark.parametrize("d,N,T", LN.PIT_CELLS)
def test_pit_sweep_fp32_keyed_equals_explicit_noise(d, N, T, gradient):
    from aux_ssm_samplers_amd import _lib, random as R
    from aux_ssm_samplers_amd.csmc import _device
    dtype, Cn = np.float32, 3
    c = LN.pit_literal(d, N, T, gradient)[0]
    fk = c.device_model()
    x0 = c.chains(Cn, 1)[0].astype(dtype)
    h, key = _lib.default_handle(), R.PRNGKey(5 + d)
    noise = PC.keyed_noise(lambda s, shape: h.rng_normal(key, s, shape, dtype).to_host(), lambda s, shape: h.rng_uniform(key, s, shape, dtype).to_host(), Cn, T, N, d)
    x, anc = _device.pit_sweep(fk, x0, N, noise=noise, delta=c.delta)
    xk, anck = _device.pit_sweep(fk, x0, N, key=key, delta=c.delta)
    npt.assert_array_equal(x, xk)
    npt.assert_array_equal(anc, anck)
    assert x.dtype == dtype and np.isfinite(x).all() and anc.min() >= 0 and anc.max() < N and (anc != 0).any()
    npt.assert_array_equal(x[anc == 0], x0[anc == 0])


# ---- 4. fp32 tie rate --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dx,N,T,style,family", [(24, 25, 250, "independent", "binomial"), (24, 25, 250, "guided", "negbinomial"), (4, 64, 1000, "independent", "binomial"),
                                                 (4, 64, 1000, "independent", "negbinomial")])
def test_fp32_ancestors_against_the_literal_order_tie_rate(dx, N, T, style, family):
    """workloads.logistic_setup on the wide path (dx = 24) and on the register path (dx = 4), 4 chains: the literal left-to-right draw on the device's own stored
    fp32 log-weights (tests/test_gpu_guided.py::_tie_rate): disagreeing draws <= 2e-4 of all draws, none farther than one visible particle -- the project's standing
    bar.  Printed beside it, with no bar: the distance of the fp32 log-weights from the fp64 sweep on the same noise, over the particles of the first step and over
    all steps whose resampling indices agree so far.
    Measured on an MI355X: DESIGN 4q."""
    from aux_ssm_samplers_amd.csmc import _device
    from aux_ssm_samplers_amd.workloads import logistic_setup
    from tests.test_gpu_guided import _tie_rate
    Cn = 4
    rng = np.random.default_rng(77)
    M0, Mt, G0, Gt, xtrue, y, _ = logistic_setup(T, dx, family, seed=3)
    x64 = xtrue[None] + 0.1 * rng.standard_normal((Cn, T, dx))
    nz = _noise(Cn, T, N, dx, rng, np.float32)
    fk = _describe(style, (M0, G0, Mt, Gt))
    assert fk.potential == 8
    delta = 0.2 / dx
    _, _, hist = _device.sweep(fk, x64.astype(np.float32), N, False, noise=nz, delta=delta, want_history=True)
    assert hist["log_ws"].dtype == np.float32 and np.all(np.isfinite(hist["log_ws"]))
    _, _, h64 = _device.sweep(fk, x64.astype(np.float32).astype(np.float64), N, False, noise={k: v.astype(np.float64) for k, v in nz.items()}, delta=delta,
                              want_history=True)
    same = np.cumprod(np.all(hist["As"] == h64["As"], axis=2), axis=1).astype(bool)  # (Cn, T - 1): every resampling up to and including step t agrees
    agree = np.concatenate([np.ones((Cn, 1), bool), same], axis=1)
    dlw = np.abs(hist["log_ws"].astype(np.float64) - h64["log_ws"])
    scale = float(np.max(np.abs(h64["log_ws"][agree])))
    print(f"{family} {style} dx={dx} N={N} T={T}: fp32 log-weights against the fp64 sweep on the same noise: max |diff| {float(dlw[:, 0].max()):.2e} at t = 0, "
          f"{float(dlw[agree].max()):.2e} over the {int(agree.sum())} of {Cn * T} steps whose ancestry still agrees (largest |log w| there {scale:.1f})")
    bad, tot, far = _tie_rate(hist, nz["u_res"])
    print(f"{family} {style} dx={dx} N={N} T={T}: {bad} of {tot} fp32 draws differ from the literal order ({bad / tot:.2e}), {far} farther than one visible particle")
    assert bad / tot <= 2e-4, (bad, tot)
    assert far == 0


# ---- 5. resident chains ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,N,T,style,family", [(3, 100, 33, "independent", "binomial"), (3, 100, 33, "guided", "negbinomial"), (3, 100, 33, "pit", "binomial"),
                                                (9, 25, 20, "independent", "negbinomial"), (9, 25, 20, "guided", "binomial"), (9, 25, 20, "pit", "negbinomial")])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_resident_chains_equal_host_state_sweeps(dtype, d, N, T, style, family):
    """three sweeps on CsmcChains equal three host-state sweeps with the same keys, bit for bit: independent proposals with the exact gradient weighting, guided
    proposals with gradient, parallel in time; one register shape and one wide shape"""
    from aux_ssm_samplers_amd import _lib, random as R
    from aux_ssm_samplers_amd.csmc import CsmcChains, CSMCState, get_guided_kernel, get_independent_kernel
    rng = np.random.default_rng(5 + d)
    dev, m, xtrue, delta = LN.case(d, T, rng, family, nan_steps=(1, 5, T - 1))
    assert LN.has_every_feature(m)
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


# ---- 5b. more chains than CUs: the eight-wave fp32 wide kernels ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("style,gradient,backward", [("bootstrap", False, False), ("independent", False, True), ("independent", "exact", True), ("guided", True, True)])
@pytest.mark.parametrize("d,N,T,family", [(9, 25, 8, "binomial"), (32, 64, 5, "negbinomial")])
def test_one_launch_equals_sixteen_wave_launches(d, N, T, family, style, gradient, backward):
    """k_cw2_fwd<float, 8, false, LOGI> / k_cw2_bwd<float, 8> (fp32 with more chains than CUs) against the sixteen-wave instantiations that sections 1 - 4 hold:
    one launch of CUs + 3 chains is bit-identical to the same chains as launches of CUs and 3 (the construction of tests/test_gpu_csmc_wide_chains.py)"""
    from tests import test_gpu_csmc_wide_chains as W
    cu = W._cu()
    Cn = cu + 3
    dev, m, xtrue, delta = LN.case(d, T, np.random.default_rng([3, d, T]), family, nan_steps=(0, T // 2, T - 1))
    assert LN.has_every_feature(m)
    nz = dict(W._inputs(300 + d, Cn, T, N, d))
    x0 = (xtrue[None] + np.float32(0.3) * nz.pop("x0")).astype(np.float32)
    if style == "bootstrap":
        nz.pop("eps_aux")
        delta = None
    fk = _describe(style, dev, gradient)
    assert fk.potential == 8
    one = W._sweep(fk, x0, N, backward, nz, delta)
    parts = [W._sweep(fk, x0[a:b], N, backward, {k: v[a:b] for k, v in nz.items()}, delta) for a, b in ((0, cu), (cu, Cn))]
    for name in W.FIELDS:
        W._assert_same(one[name], np.concatenate([p[name] for p in parts]), f"{name}, one launch of {Cn} chains against launches of {cu} and 3")
    assert one["xs"].dtype == np.float32 and np.all(np.isfinite(one["log_ws"]))
    assert np.all(one["As"][:, :, 0] == 0) and np.array_equal(one["xs"][:, :, 0], x0)
    assert (one["ancestors"] != 0).any()


# ---- 6. ground truth: the posterior by quadrature -------------------------------------------------------------------------------------------------------------
_models = {}


def _truth_model(which):
    """"a": d = 1, T = 6, binomial with trials in 1 .. 20;  "binary": the same with trials = 1;  "nb": d = 1, T = 6, negative binomial with r = 0.5;  "b": d = 6,
    T = 5, negative binomial with r in {0.5, 1, 3} per component and diagonal F, Q and P0 with distinct values per component, so the components are independent
    scalar models.  Returns (device objects, the parameters (m0, P0, F, Q, b) as vectors of the diagonals, y, family, the family's parameter (T, d)); built once"""
    if which not in _models:
        rng = np.random.default_rng(2025)
        d, T = (6, 5) if which == "b" else (1, 6)
        k = np.arange(d)
        F, Q, P0 = 0.9 - 0.07 * k, 0.3 + 0.05 * k, 0.5 + 0.1 * k
        m0, b = 0.2 - 0.1 * k, 0.05 * (k - 1.0)
        assert d == 1 or (len(set(F)) == len(set(Q)) == len(set(P0)) == d)
        x = np.zeros((T, d))
        x[0] = m0 + np.sqrt(P0) * rng.standard_normal(d)
        for t in range(1, T):
            x[t] = F * x[t - 1] + b + np.sqrt(Q) * rng.standard_normal(d)
        if which in ("a", "binary"):
            family = "binomial"
            par = np.ones((T, d)) if which == "binary" else rng.integers(1, 21, size=(T, d)).astype(np.float64)
            y = rng.binomial(par.astype(np.int64), 1.0 / (1.0 + np.exp(-x))).astype(np.float64)
        else:
            family = "negbinomial"
            par = np.full((T, d), 0.5) if which == "nb" else np.broadcast_to(np.array([0.5, 1.0, 3.0])[k % 3], (T, d)).copy()
            y = rng.poisson(rng.gamma(par, np.exp(x))).astype(np.float64)
        y[2, 0] = np.nan  # one missing observation
        dev, m = LN.build(m0, np.diag(P0), np.diag(F), b, np.diag(Q), y, family, par)
        _models[which] = (dev, (m0, P0, F, Q, b), y, family, par)
    return _models[which]


def _moments(par, y, size):
    """(E x_t, E x_t x_t^T) of the posterior: per component by quadrature, cross moments as products of the means (the components are independent)"""
    m0, P0, F, Q, b = par
    T, d = y.shape
    q = np.stack([LN.posterior_by_quadrature(y[:, k], size[:, k], m0[k], P0[k], F[k], Q[k], b[k]) for k in range(d)], axis=1)  # (T, d, 2)
    mean = q[..., 0]
    second = mean[:, :, None] * mean[:, None, :]
    second[:, np.arange(d), np.arange(d)] += q[..., 1]
    return mean, second


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
           + [("b", s) for s in ("independent-backward", "exact", "guided", "guided-gradient")] + [("binary", "exact"), ("nb", "guided-gradient")])


@pytest.mark.parametrize("which,sampler", _CASES6)
def test_particle_gibbs_matches_the_posterior_by_quadrature(which, sampler):
    """1024 resident chains: every posterior mean and second moment (cross moments of a step included) within 5 empirical standard errors of the quadrature value --
    the standard error is the standard deviation of the per-chain time averages over sqrt(chains), the rule of tests/test_gpu_posterior_quadrature.py.  Power: the
    quadrature posterior for the data y + 1 (binomial: trials + 1 as well, so that the data stay valid; negative binomial: the same r) lies more than 10 of the same
    standard errors away in at least one compared moment."""
    from tests.test_gpu_mvt import _gibbs_moments
    dev, par, y, family, fpar = _truth_model(which)
    m0, P0, F, Q, b = par
    T, d = y.shape
    size = fpar if family == "binomial" else y + fpar
    size1 = fpar + 1.0 if family == "binomial" else y + 1.0 + fpar
    # the step size, from the model alone: the gradient proposals N(u + delta/2 grad, delta/2 I) are one Langevin step, which contracts towards the mode only while
    # delta/2 lambda < 2, lambda the largest curvature of the negative log-target.  The Gaussian part's curvature is at most max_k (1 / P0_k + 1 / Q_k + F_k^2 / Q_k)
    # (the model is diagonal); the logistic term's is m sigma (1 - sigma) <= m / 4.  delta = 2 / lambda lands on the mode along the stiffest direction.
    lam = float(np.max(1.0 / P0 + 1.0 / Q + F * F / Q)) + float(np.nanmax(np.where(np.isfinite(y), size, np.nan))) / 4.0
    delta = 2.0 / lam
    N = 32 if which == "b" else 16
    m1, se1, m2, se2 = _gibbs_moments(_kernel(sampler, dev, N), T, d, delta, 5000 if which == "b" else 4000, burn=200, with_delta=sampler != "bootstrap")
    t1, t2 = _moments(par, y, size)
    w1, w2 = _moments(par, y + 1.0, size1)
    z1, z2 = np.abs(m1 - t1) / se1, np.abs(m2 - t2) / se2
    p1, p2 = np.abs(w1 - t1) / se1, np.abs(w2 - t2) / se2
    print(f"({which}, {family}) {sampler}: delta = {delta:.3f}; worst z of the means {z1.max():.2f}, of the second moments {z2.max():.2f}; the posterior for the data "
          f"y + 1 lies {max(p1.max(), p2.max()):.0f} standard errors away")
    assert max(p1.max(), p2.max()) > 10
    assert z1.max() < 5 and z2.max() < 5


# ---- 7. the C entry points --------------------------------------------------------------------------------------------------------------------------------
def test_c_entry_points_refuse_missing_observations_and_unknown_kinds():
    from aux_ssm_samplers_amd import _lib
    from aux_ssm_samplers_amd.csmc import _device
    h = _lib.default_handle()
    T, N, d, dt = 6, 64, 2, np.float64
    dev, m, xtrue, _ = LN.case(d, T, np.random.default_rng(0))
    fk = _device.describe_independent(dev[0], dev[1], dev[2], dev[3], dev[2])
    x, anc, shd = h.to_device(np.ones((1, T, d)), dt), h.zeros((1, T), np.int32), h.to_device(np.full(T, 0.3), dt)
    nz = _lib.CsmcNoise()
    nz.mode, nz.key0, nz.key1 = _lib.NOISE_THREEFRY, 1, 2
    tail = (1, T, N, 1, shd.ptr, x.ptr, C.byref(nz), anc.ptr, None, None, None)

    def both(ms, msg):
        assert h.lib.auxssm_csmc_sweep(h.h, _lib.dtype_code(dt), C.byref(ms), *tail) == _lib.ERR_ARG
        assert msg in h.lib.auxssm_last_error().decode()
        assert h.lib.auxssm_csmc_pit_sweep(h.h, _lib.dtype_code(dt), C.byref(ms), 1, T, N, shd.ptr, x.ptr, C.byref(nz), anc.ptr) == _lib.ERR_ARG
        assert msg in h.lib.auxssm_last_error().decode()
    ms = fk.struct(h, dt, T)
    assert ms.potential == 8
    ms.y = None
    both(ms, "observations y")
    for kind in (7, 9):
        ms = fk.struct(h, dt, T)
        ms.potential = kind
        both(ms, f"unknown potential kind {kind}")
    ms = fk.struct(h, dt, T)
    assert h.lib.auxssm_csmc_sweep(h.h, _lib.dtype_code(dt), C.byref(ms), *tail) == 0  # and the untampered description runs
    assert h.lib.auxssm_csmc_pit_sweep(h.h, _lib.dtype_code(dt), C.byref(ms), 1, T, N, shd.ptr, x.ptr, C.byref(nz), anc.ptr) == 0
    with pytest.raises(ValueError, match="time steps"):
        fk.struct(h, dt, T + 1)
