"""The multivariate Student-t potential (AUXSSM_POT_MVT, csmc.MultivariateTPotential) on the GPU, through every kernel family: the register kernels
(dx <= 4), the wide kernels (4 < dx <= 32, N <= 64: the spatial example on grids up to 5 x 5 at its own N = 25), the parallel-in-time sweep, gradient and
guided proposals, resident chains.

1. Built-in kind 4 against the same potential as a user program (device_models.BUILTIN_MVT[_GRAD]), bit for bit, dx <= 4, fp32 and fp64.
2. Literal parity in fp64 on explicit noise against oracle/csmc_np.py on the objects of tests/mvt_np.py: resampling ancestors and backward indices identical,
   particles within 1e-12, log-weights within 1e-10 (the bars of tests/test_gpu_csmc_literal.py and tests/test_gpu_guided.py).
3. fp32 by the teacher-forced tie-rate rule of tests/test_gpu_csmc_literal.py: the wide path (no contract oracle covers it) and the register path at dx = 4.
4. The parallel-in-time sweep and resident chains.
5. Ground truth by quadrature, no restatement in the loop: a scalar model with T = 3 for every sampler style, and a two-dimensional model with a
   non-diagonal precision matrix, which pins the coupling of the components itself.
6. The C entry point's refusals."""
import ctypes as C

import numpy as np
import numpy.testing as npt
import pytest

from oracle import csmc_np as L
from tests import mvt_np as MV

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
@pytest.mark.parametrize("d,N,T,Cn", [(1, 1024, 40, 5), (2, 100, 40, 5), (4, 64, 24, 3)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_builtin_potential_equals_the_user_program_bit_for_bit(dtype, d, N, T, Cn):
    """bootstrap and independent proposals, gradient False / True / "exact", both backward modes, explicit and Threefry noise; two observation rows carry a NaN"""
    from aux_ssm_samplers_amd import random as R
    from aux_ssm_samplers_amd.csmc import _device
    rng = np.random.default_rng(100 * d + N)
    dev, m, xtrue, delta = MV.case(d, T, rng, nan_rows=(3, T - 2))
    x0 = (xtrue[None] + 0.3 * rng.standard_normal((Cn, T, d))).astype(dtype)
    nz = _noise(Cn, T, N, d, rng, dtype)
    for style, gradient in (("bootstrap", False), ("independent", False), ("independent", True), ("independent", "exact")):
        fb, fu = _describe(style, dev, gradient), _describe(style, MV.program(dev, bool(gradient)), gradient)
        assert fb.potential == 4 and fb.user is None and fu.user is not None
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
def _literal_case(name, rng):
    """(d, N, T) and the model: register path (1, 1024, 40), (3, 100, 33); wide path (5, 33, 20), the 3 x 3 and 5 x 5 grids of the spatial example
    (random walk, its precision matrix; nu = 1 on the 5 x 5 grid, the example's own value) and (32, 64, 12); time-varying transitions on the register path at
    N = 65, 512 and 1024 (a partial last wave, eight and sixteen full waves: this potential runs the generic workgroup at every N), three steps"""
    from aux_ssm_samplers_amd.workloads import spatial_precision
    d, N, T = dict(r1=(1, 1024, 40), r3=(3, 100, 33), w5=(5, 33, 20), grid3=(9, 25, 20), grid5=(25, 25, 25), w32=(32, 64, 12),
                   tv65=(1, 65, 3), tv512=(1, 512, 3), tv1024=(1, 1024, 3))[name]
    if name.startswith("tv"):
        dev, m, xtrue, delta = MV.case(d, T, rng, tv=True)
    elif name.startswith("grid"):
        dev, m, xtrue, delta = MV.case(d, T, rng, nu=1.0 if name == "grid5" else 3.0, prec=spatial_precision(int(name[-1])), walk=True, nan_rows=(4,))
    else:
        dev, m, xtrue, delta = MV.case(d, T, rng, nan_rows=(2, T - 1))
    return d, N, T, dev, m, xtrue + 0.3 * rng.standard_normal((T, d)), delta


def _against_literal(style, gradient, backward, name, seed):
    """one fp64 sweep on explicit noise next to the literal sampler; returns (ancestors, max particle error, max log-weight error)"""
    from aux_ssm_samplers_amd.csmc import _device
    rng = np.random.default_rng(seed)
    d, N, T, dev, m, x0, delta = _literal_case(name, rng)
    nz = {k: v[0] for k, v in _noise(1, T, N, d, rng).items()}
    if style == "bootstrap":
        nz.pop("eps_aux")
    x, anc, hist = _device.sweep(_describe(style, dev, gradient), x0, N, backward, noise={k: v[None] for k, v in nz.items()},
                                 delta=None if style == "bootstrap" else delta, want_history=True)
    if style == "bootstrap":
        xl, Bl, lh = MV.bootstrap_kernel(m, N, backward)[1](L.Noise(**nz), x0)
    elif style == "guided":
        xl, Bl, lh = MV.guided_kernel(m, N, backward, gradient)[1](L.Noise(**nz), x0, delta)
    else:
        xl, Bl, lh = MV.independent_kernel(m, N, backward, gradient)[1](L.Noise(**nz), x0, delta)
    ex, el = float(np.max(np.abs(hist["xs"] - lh["xs"]))), float(np.max(np.abs(hist["log_ws"] - lh["log_ws"])))
    print(f"{style} gradient={gradient} backward={backward} {name} (d={d} N={N} T={T}): max |xs - literal| = {ex:.1e}, max |log_ws - literal| = {el:.1e}, "
          f"updated {int((anc != 0).sum())} of {T}")
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
        # the direct identity: the stored log-weights are log g_t + log initial / log transition themselves (the kernels store them before any shift: shift 0)
        for t in range(T):
            g = MV.log_g(hist["xs"][t], m.y[t], m.nu, m.prec)
            if t == 0:
                dens = L._mvn_chol_logpdf(hist["xs"][0], m.m0, m.LP0)
            else:
                F, b, _, LQ = m.trans(t)
                dens = L._mvn_chol_logpdf(hist["xs"][t], hist["xs"][t - 1][hist["As"][t - 1]] @ F.T + b, LQ)
            npt.assert_allclose(hist["log_ws"][t], g + dens, rtol=1e-10, atol=1e-10)
    return anc, ex, el


@pytest.mark.parametrize("backward", [False, True])
@pytest.mark.parametrize("style,gradient", [("independent", False), ("independent", True), ("independent", "exact"), ("guided", False), ("guided", True)])
def test_sweep_fp64_equals_the_literal_sampler(style, gradient, backward):
    """register and wide path; a single case may update nothing, over the set every (style, gradient, backward) cell moves the trajectory somewhere"""
    moved = 0
    names = ("r1", "r3", "w5", "grid3", "grid5", "w32") + (() if style == "guided" else ("tv65", "tv512", "tv1024"))  # (guided: time-invariant transitions only)
    for i, name in enumerate(names):
        moved += int((_against_literal(style, gradient, backward, name, 7000 + 10 * i + backward)[0] != 0).sum())
    assert moved > 0


@pytest.mark.parametrize("backward", [False, True])
@pytest.mark.parametrize("name", ["r3", "grid3"])
def test_bootstrap_sweep_fp64_equals_the_literal_sampler(name, backward):
    anc, _, _ = _against_literal("bootstrap", False, backward, name, 7100 + backward)
    assert (anc != 0).any()


# ---- 3. fp32 on the wide path ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid,N", [(5, 25), (2, 64)])
@pytest.mark.parametrize("style", ["independent", "guided"])
def test_fp32_ancestors_against_the_literal_order_tie_rate(style, grid, N):
    """the spatial example on the 5 x 5 grid at its own N = 25, T = 250, 4 chains (the wide path, which no contract oracle covers in fp32), and on the 2 x 2 grid
    (the register path at dx = 4): the literal left-to-right draw on the device's own stored fp32 log-weights (tests/test_gpu_csmc_literal.py's rule):
    disagreeing draws <= 2e-4 of all draws, none farther than one visible particle"""
    from aux_ssm_samplers_amd.csmc import _device
    from aux_ssm_samplers_amd.workloads import spatial_setup
    from tests.test_gpu_guided import _tie_rate
    d, T, Cn = grid * grid, 250, 4
    rng = np.random.default_rng(77)
    M0, Mt, G0, Gt, xtrue, y, prec = spatial_setup(T, grid, seed=3)
    x0 = (xtrue[None] + 0.3 * rng.standard_normal((Cn, T, d))).astype(np.float32)
    nz = _noise(Cn, T, N, d, rng, np.float32)
    _, _, hist = _device.sweep(_describe(style, (M0, G0, Mt, Gt)), x0, N, False, noise=nz, delta=0.1, want_history=True)
    assert hist["log_ws"].dtype == np.float32 and np.all(np.isfinite(hist["log_ws"]))
    bad, tot, far = _tie_rate(hist, nz["u_res"])
    print(f"{style} d={d} N={N}: {bad} of {tot} fp32 draws differ from the literal order ({bad / tot:.2e}), {far} farther than one visible particle")
    assert bad / tot <= 2e-4, (bad, tot)
    assert far == 0


# ---- 4. parallel in time, resident chains ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gradient", [False, True])
@pytest.mark.parametrize("d,N,T", [(1, 32, 25), (3, 100, 33), (1, 100, 33), (3, 32, 25)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_parallel_in_time_sweep_runs_and_returns_consistent_paths(dtype, d, N, T, gradient):
    """parallel=True: finite trajectories whose every step is the leaf particle its ancestor index names (slot 0 = the reference trajectory), keyed ==
    explicit noise, and the trajectory moves.  WHICH particles the stitches pick -- the observation row, the transition term and the whole precision matrix in the
    stitch weights -- is held against the literal tree of oracle/pit_np.py in tests/test_gpu_pit_literal.py::test_hip_pit_sweep_student_t_fp64_equals_the_literal_tree"""
    from aux_ssm_samplers_amd import _lib, random as R
    from aux_ssm_samplers_amd.csmc import _device
    rng = np.random.default_rng(10 * d + N)
    dev, m, xtrue, _ = MV.case(d, T, rng, nan_rows=(5,))
    Cn, delta = 3, 0.4
    fk = _device.describe_independent(dev[0], dev[1], dev[2], dev[3], None, _gmode("exact" if gradient else False), parallel=True)
    x0 = (xtrue[None] + 0.3 * rng.standard_normal((Cn, T, d))).astype(dtype)
    h, key = _lib.default_handle(), R.PRNGKey(5 + d)
    noise = dict(eps_aux=h.rng_normal(key, 1, (Cn, T, d), dtype).to_host(), eps_prop=h.rng_normal(key, 2, (Cn, T, N, d), dtype).to_host(),
                 u_res=h.rng_uniform(key, 3, (Cn, T, N), dtype).to_host())
    x, anc = _device.pit_sweep(fk, x0, N, noise=noise, delta=delta)
    xk, anck = _device.pit_sweep(fk, x0, N, key=key, delta=delta)
    npt.assert_array_equal(x, xk)
    npt.assert_array_equal(anc, anck)
    assert x.dtype == dtype and np.isfinite(x).all() and anc.min() >= 0 and anc.max() < N and (anc != 0).mean() > 0.2
    npt.assert_array_equal(x[anc == 0], x0[anc == 0])
    if not gradient:  # the leaves: x_t^n = u_t + s eps_t^n around u = x0 + s eps_aux
        s = dtype(np.sqrt(0.5 * delta))
        leaves = (x0 + s * noise["eps_aux"])[:, :, None, :] + s * noise["eps_prop"]
        leaves[:, :, 0] = x0
        tol = 1e-5 if dtype == np.float32 else 1e-12
        npt.assert_allclose(x, np.take_along_axis(leaves, anc[:, :, None, None], axis=2)[:, :, 0], rtol=tol, atol=tol)


@pytest.mark.parametrize("d,N,T", [(1, 32, 25), (3, 100, 33)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("style", ["independent", "guided", "pit"])
def test_resident_chains_equal_host_state_sweeps(style, dtype, d, N, T):
    """three sweeps on CsmcChains equal three host-state sweeps with the same keys, bit for bit"""
    from aux_ssm_samplers_amd import _lib, random as R
    from aux_ssm_samplers_amd.csmc import CsmcChains, CSMCState, get_guided_kernel, get_independent_kernel
    rng = np.random.default_rng(5 + d)
    dev, m, xtrue, delta = MV.case(d, T, rng, nan_rows=(1,))
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


# ---- 5. ground truth by quadrature ---------------------------------------------------------------------------------------------------------------------
def _trapezoid(n, half_width):
    g = np.linspace(-half_width, half_width, n)
    w = np.full(n, g[1] - g[0])
    w[[0, -1]] *= 0.5
    return g, w


def _scalar_truth(y, nu, lam, n):
    """E x_t and E x_t^2, t < 3, of  N(x_0; 0, 1) prod_t g(x_t) prod_t N(x_t; x_{t-1}, 1)  on the tensor trapezoid grid of n^3 points over [-14, 14]^3 (evaluated
    through the chain structure of the integrand: the same sum, factorised)"""
    g, w = _trapezoid(n, 14.0)
    pot = [np.exp(MV.log_g(g[:, None], [yt], nu, [[lam]])) for yt in y]
    K = np.exp(-0.5 * (g[:, None] - g[None, :]) ** 2)  # K[i, j]: x_t = g[i] given x_{t-1} = g[j] (constants cancel)
    f = [np.exp(-0.5 * g * g) * pot[0] * w]
    for t in (1, 2):
        f.append((K @ f[-1]) * pot[t] * w)
    b = [None, None, np.ones(n)]
    for t in (1, 0):
        b[t] = K.T @ (b[t + 1] * pot[t + 1] * w)
    out = np.zeros((3, 2))
    for t in range(3):
        p = f[t] * b[t]
        out[t] = np.sum(p * g) / np.sum(p), np.sum(p * g * g) / np.sum(p)
    return out


def _refined(fn, n0):
    """fn on grids of n0, 2 n0 - 1, ... points until two successive grids agree to 1e-10"""
    prev, n = fn(n0), n0
    for _ in range(4):
        n = 2 * n - 1
        cur = fn(n)
        if np.max(np.abs(cur - prev)) < 1e-10:
            return cur
        prev = cur
    raise AssertionError("the quadrature did not converge to 1e-10")


_truth = {}


def _scalar_model():
    """T = 3, d = 1, nu = 3, prec = [[2]], a random walk with sigma = 1 from N(0, 1); the reference is computed once"""
    from aux_ssm_samplers_amd.csmc import GaussianInit, LinearGaussianDynamics, MultivariateTPotential
    y, nu, lam = np.array([[0.8], [-0.5], [1.7]]), 3.0, 2.0
    if "scalar" not in _truth:
        _truth["scalar"] = _refined(lambda n: _scalar_truth(y[:, 0], nu, lam, n), 281)
    M0, Mt = GaussianInit(m0=[0.0], P0=[[1.0]]), LinearGaussianDynamics(F=[[1.0]], b=[0.0], Q=[[1.0]])
    return (M0, MultivariateTPotential(nu=nu, prec=[[lam]], y=y[0]), Mt, MultivariateTPotential(nu=nu, prec=[[lam]], params=y[1:])), _truth["scalar"]


def _gibbs_moments(kernel, T, d, delta, seed, Cn=1024, burn=60, iters=240, with_delta=True):
    """per-chain time averages of x and of the products x_i x_j over `iters` sweeps of 1024 resident chains: (means, second moments) with their empirical
    standard errors across the chains, which are independent"""
    from aux_ssm_samplers_amd import _lib, random as R
    from aux_ssm_samplers_amd.csmc import CsmcChains, CSMCState
    chains = CsmcChains(_lib.default_handle(), np.zeros((Cn, T, d)), delta=delta if with_delta else None, dtype=np.float64)
    state = CSMCState(x=chains, updated=None)
    s1, s2 = np.zeros((Cn, T, d)), np.zeros((Cn, T, d, d))
    for it in range(burn + iters):
        state = kernel(R.PRNGKey(seed + it), state, None) if with_delta else kernel(R.PRNGKey(seed + it), state)
        if it >= burn:
            xh = chains.to_host()
            s1 += xh
            s2 += xh[..., :, None] * xh[..., None, :]
    m1, m2 = s1 / iters, s2 / iters
    return m1.mean(0), m1.std(0, ddof=1) / np.sqrt(Cn), m2.mean(0), m2.std(0, ddof=1) / np.sqrt(Cn)


@pytest.mark.parametrize("sampler", ["independent-trace", "independent-backward", "exact", "guided", "guided-gradient", "bootstrap", "pit", "pit-gradient"])
def test_particle_gibbs_matches_the_posterior_by_quadrature(sampler):
    """1024 resident chains: every posterior mean and second moment within 5 of its empirical standard errors"""
    from aux_ssm_samplers_amd._primitives.csmc import get_kernel as get_bootstrap_kernel
    from aux_ssm_samplers_amd.csmc import get_guided_kernel, get_independent_kernel
    dev, truth = _scalar_model()
    N = 16
    if sampler == "bootstrap":
        kernel = get_bootstrap_kernel(*dev, N, backward=True, Pt=dev[2])[1]
    elif sampler.startswith("guided"):
        kernel = get_guided_kernel(*dev, N, backward=True, gradient=sampler.endswith("gradient"))[1]
    elif sampler.startswith("pit"):
        kernel = get_independent_kernel(*dev, N, gradient=sampler.endswith("gradient"), parallel=True)[1]
    else:
        kernel = get_independent_kernel(*dev, N, backward=sampler != "independent-trace", Pt=dev[2], gradient="exact" if sampler == "exact" else False)[1]
    m1, se1, m2, se2 = _gibbs_moments(kernel, 3, 1, 1.0, 2000, with_delta=sampler != "bootstrap")
    z1, z2 = np.abs(m1[:, 0] - truth[:, 0]) / se1[:, 0], np.abs(m2[:, 0, 0] - truth[:, 1]) / se2[:, 0, 0]
    print(f"{sampler}: means {m1[:, 0]} (truth {truth[:, 0]}), worst z {z1.max():.2f}; second moments {m2[:, 0, 0]} (truth {truth[:, 1]}), worst z {z2.max():.2f}")
    assert z1.max() < 5 and z2.max() < 5


def _coupled_truth(y, nu, prec, n):
    """E x_t and E x_t x_t^T, t < 2, d = 2, of  N(x_0; 0, I) g(x_0) N(x_1; x_0, I) g(x_1)  on the tensor trapezoid grid of n^4 points over [-10, 10]^4; the
    transition density is a product over the two components, so the sum over x_0 (x_1) is two matrix products"""
    g, w = _trapezoid(n, 10.0)
    X = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1)  # X[i, j] = (g[i], g[j])
    W = w[:, None] * w[None, :]
    pot = [np.exp(MV.log_g(X.reshape(-1, 2), yt, nu, prec)).reshape(n, n) for yt in y]
    K = np.exp(-0.5 * (g[:, None] - g[None, :]) ** 2)
    f0 = np.exp(-0.5 * np.sum(X * X, axis=-1)) * pot[0] * W
    p1 = (K @ f0 @ K.T) * pot[1] * W               # the marginal of x_1 on the grid
    p0 = f0 * (K.T @ (pot[1] * W) @ K)             # the marginal of x_0
    out = []
    for p in (p0, p1):
        p = p / p.sum()
        out.append(np.concatenate([np.einsum("ij,ijk->k", p, X), np.einsum("ij,ijk,ijl->kl", p, X, X).reshape(-1)]))
    return np.array(out)  # rows t: [E x_0, E x_1, E x_0 x_0, E x_0 x_1, E x_1 x_0, E x_1 x_1]


def test_coupled_components_match_the_posterior_by_quadrature():
    """d = 2, T = 2, a non-diagonal precision matrix: independent proposals with backward sampling reproduce the means, the second moments and the cross moment
    E x_{t,0} x_{t,1} of the 4-dimensional quadrature -- the coupling term of the potential is pinned by truth"""
    from aux_ssm_samplers_amd.csmc import GaussianInit, LinearGaussianDynamics, MultivariateTPotential, get_independent_kernel
    y, nu, prec = np.array([[0.9, -0.6], [-0.4, 1.2]]), 3.0, np.array([[2.0, 1.2], [1.2, 1.5]])
    truth = _refined(lambda n: _coupled_truth(y, nu, prec, n), 161)
    diag = _refined(lambda n: _coupled_truth(y, nu, np.diag(np.diag(prec)), n), 161)
    assert np.max(np.abs(truth - diag)) > 0.05  # (the off-diagonal entry matters at this size: a kernel that dropped it would miss by many standard errors)
    M0, Mt = GaussianInit(m0=np.zeros(2), P0=np.eye(2)), LinearGaussianDynamics(F=np.eye(2), b=np.zeros(2), Q=np.eye(2))
    dev = (M0, MultivariateTPotential(nu=nu, prec=prec, y=y[0]), Mt, MultivariateTPotential(nu=nu, prec=prec, params=y[1:]))
    kernel = get_independent_kernel(*dev, 16, backward=True, Pt=Mt)[1]
    m1, se1, m2, se2 = _gibbs_moments(kernel, 2, 2, 1.0, 3000)
    est = np.concatenate([m1, m2.reshape(2, 4)], axis=1)
    z = np.abs(est - truth) / np.concatenate([se1, se2.reshape(2, 4)], axis=1)
    print(f"estimates {est}\ntruth {truth}\nworst z {z.max():.2f}")
    assert z.max() < 5


# ---- 6. the C entry point ----------------------------------------------------------------------------------------------------------------------------------
def test_c_entry_point_refuses_a_missing_precision_matrix_and_a_bad_nu():
    from aux_ssm_samplers_amd import _lib
    from aux_ssm_samplers_amd.csmc import _device
    h = _lib.default_handle()
    T, N, d, dt = 6, 64, 2, np.float64
    dev, m, xtrue, _ = MV.case(d, T, np.random.default_rng(0))
    fk = _device.describe_independent(dev[0], dev[1], dev[2], dev[3], dev[2])
    x, anc, shd = h.to_device(np.zeros((1, T, d)), dt), h.zeros((1, T), np.int32), h.to_device(np.full(T, 0.5), dt)
    nz = _lib.CsmcNoise()
    nz.mode, nz.key0, nz.key1 = _lib.NOISE_THREEFRY, 1, 2
    tail = (1, T, N, 1, shd.ptr, x.ptr, C.byref(nz), anc.ptr, None, None, None)
    for fields, msg in ((dict(prec=None), "prec"), (dict(nu=0.0), "nu > 0"), (dict(nu=-2.0), "nu > 0"), (dict(nu=float("nan")), "nu > 0")):
        ms = fk.struct(h, dt, T)
        for name, value in fields.items():
            setattr(ms, name, value)
        assert h.lib.auxssm_csmc_sweep(h.h, _lib.dtype_code(dt), C.byref(ms), *tail) == _lib.ERR_ARG
        assert msg in h.lib.auxssm_last_error().decode()
        assert h.lib.auxssm_csmc_pit_sweep(h.h, _lib.dtype_code(dt), C.byref(ms), 1, T, N, shd.ptr, x.ptr, C.byref(nz), anc.ptr) == _lib.ERR_ARG
    ms = fk.struct(h, dt, T)
    assert h.lib.auxssm_csmc_sweep(h.h, _lib.dtype_code(dt), C.byref(ms), *tail) == 0  # and the untampered description runs
