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
6. The C entry point's refusals.

The shared assertion blocks are those of tests/potential_gpu.py, run with this kind's record."""
import numpy as np
import numpy.testing as npt
import pytest

from tests import mvt_np as MV
from tests import potential_gpu as GP

pytestmark = pytest.mark.gpu
KIND = MV.KIND


# ---- 1. the built-in against the program ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,N,T,Cn", [(1, 1024, 40, 5), (2, 100, 40, 5), (4, 64, 24, 3)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_builtin_potential_equals_the_user_program_bit_for_bit(dtype, d, N, T, Cn):
    """bootstrap and independent proposals, gradient False / True / "exact", both backward modes, explicit and Threefry noise; two observation rows carry a NaN"""
    from aux_ssm_samplers_amd import random as R
    rng = np.random.default_rng(100 * d + N)
    dev, m, xtrue, delta = MV.case(d, T, rng, nan_rows=(3, T - 2))
    x0 = (xtrue[None] + 0.3 * rng.standard_normal((Cn, T, d))).astype(dtype)
    seen = GP.assert_program_equality(KIND, dev, x0, N, delta, GP.noise(Cn, T, N, d, rng, dtype), R.PRNGKey(31 + d))
    assert all((s[4] != 0).any() for s in seen)


# ---- 2. literal parity (the cases: tests/mvt_np.py::LITERAL_CASES) -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backward", [False, True])
@pytest.mark.parametrize("style,gradient", [("independent", False), ("independent", True), ("independent", "exact"), ("guided", False), ("guided", True)])
def test_sweep_fp64_equals_the_literal_sampler(style, gradient, backward):
    """register and wide path; a single case may update nothing, over the set every (style, gradient, backward) cell moves the trajectory somewhere"""
    GP.literal_cell_moves(KIND, style, gradient, backward)


@pytest.mark.parametrize("backward", [False, True])
@pytest.mark.parametrize("name", MV.BOOTSTRAP_CASES)
def test_bootstrap_sweep_fp64_equals_the_literal_sampler(name, backward):
    assert (GP.against_literal(KIND, "bootstrap", False, backward, name) != 0).any()


# ---- 3. fp32 on the wide path ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid,N", [(5, 25), (2, 64)])
@pytest.mark.parametrize("style", ["independent", "guided"])
def test_fp32_ancestors_against_the_literal_order_tie_rate(style, grid, N):
    """the spatial example on the 5 x 5 grid at its own N = 25, T = 250, 4 chains (the wide path, which no contract oracle covers in fp32), and on the 2 x 2 grid
    (the register path at dx = 4): the literal left-to-right draw on the device's own stored fp32 log-weights (tests/test_gpu_csmc_literal.py's rule):
    disagreeing draws <= 2e-4 of all draws, none farther than one visible particle"""
    from aux_ssm_samplers_amd.workloads import spatial_setup
    d, T, Cn = grid * grid, 250, 4
    rng = np.random.default_rng(77)
    M0, Mt, G0, Gt, xtrue, y, prec = spatial_setup(T, grid, seed=3)
    x0 = (xtrue[None] + 0.3 * rng.standard_normal((Cn, T, d))).astype(np.float32)
    nz = GP.noise(Cn, T, N, d, rng, np.float32)
    GP.tie_rate_within_the_bar(GP.describe(style, (M0, G0, Mt, Gt)), x0, N, nz, 0.1, f"{style} d={d} N={N}")


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
    fk = _device.describe_independent(dev[0], dev[1], dev[2], dev[3], None, GP.gmode("exact" if gradient else False), parallel=True)
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
    rng = np.random.default_rng(5 + d)
    dev, m, xtrue, delta = MV.case(d, T, rng, nan_rows=(1,))
    GP.resident_equals_host(dev, (xtrue[None] + 0.3 * rng.standard_normal((4, T, d))).astype(dtype), delta, N, style)


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


@pytest.mark.parametrize("sampler", ["independent-trace", "independent-backward", "exact", "guided", "guided-gradient", "bootstrap", "pit", "pit-gradient"])
def test_particle_gibbs_matches_the_posterior_by_quadrature(sampler):
    """1024 resident chains: every posterior mean and second moment within 5 of its empirical standard errors"""
    dev, truth = _scalar_model()
    m1, se1, m2, se2 = GP.gibbs_moments(GP.kernel_of(sampler, dev, 16), 3, 1, 1.0, 2000, with_delta=sampler != "bootstrap")
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
    m1, se1, m2, se2 = GP.gibbs_moments(kernel, 2, 2, 1.0, 3000)
    est = np.concatenate([m1, m2.reshape(2, 4)], axis=1)
    z = np.abs(est - truth) / np.concatenate([se1, se2.reshape(2, 4)], axis=1)
    print(f"estimates {est}\ntruth {truth}\nworst z {z.max():.2f}")
    assert z.max() < 5


# ---- 6. the C entry point ----------------------------------------------------------------------------------------------------------------------------------
def test_c_entry_point_refuses_a_missing_precision_matrix_and_a_bad_nu():
    T, N, d = 6, 64, 2
    dev, m, xtrue, _ = MV.case(d, T, np.random.default_rng(0))
    ep = GP.EntryPoints(dev, T, N, d, x=0.0, sqrt_half_delta=0.5)
    for fields, msg in ((dict(prec=None), "prec"), (dict(nu=0.0), "nu > 0"), (dict(nu=-2.0), "nu > 0"), (dict(nu=float("nan")), "nu > 0")):
        ms = ep.struct()
        for name, value in fields.items():
            setattr(ms, name, value)
        assert ep.sweep(ms) == ep.ERR_ARG
        assert msg in ep.error()
        assert ep.pit_sweep(ms) == ep.ERR_ARG
    assert ep.sweep(ep.struct()) == 0  # and the untampered description runs
