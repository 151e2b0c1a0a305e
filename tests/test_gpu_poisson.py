"""The Poisson count potential (AUXSSM_POT_POISSON, csmc.PoissonPotential) on the GPU, through every kernel family: the register kernels (dx <= 4), the wide
kernels (4 < dx <= 32, N <= 64), the parallel-in-time sweep at both widths, gradient and guided proposals, bootstrap, resident chains.

1. Built-in kind 6 against the same potential as a user program (device_models.BUILTIN_POISSON), bit for bit, dx <= 4, fp32 and fp64.
2. Literal parity in fp64 on explicit noise against oracle/csmc_np.py / tests/guided_np.py on the objects of tests/poisson_np.py: resampling ancestors and backward
   indices identical, particles within 1e-12, log-weights within 1e-10.  tests/test_poisson_potential.py shows on the literal alone that no draw of these cases
   lies within 1e-8 of a cumulative-sum edge: an index mismatch here is a defect, never a tie.
3. The parallel-in-time sweep against the literal tree of oracle/pit_np.py (fp64, register and wide), keyed against explicit noise (fp32).
4. fp32 by the teacher-forced tie-rate rule of tests/potential_gpu.py::tie_rate, on the wide and on the register path; the distance of the fp32 log-weights from the
   fp64 sweep on the same noise is printed (no bar is set on it).
5. Resident chains; and fp32 with more chains than CUs (the eight-wave wide kernels) against the sixteen-wave launches.
6. Ground truth: the posterior of the scalar model by quadrature (tests/potential_np.py::posterior_by_quadrature); with diagonal F, Q and P0 the components of a
   d = 6 model are independent, so every marginal is its own quadrature answer -- a check of the wide kernels against truth on a non-Gaussian target.
7. The C entry points' refusals."""
import numpy as np
import pytest

from tests import poisson_np as PN
from tests import potential_gpu as GP
from tests import potential_np as P

pytestmark = pytest.mark.gpu
KIND = PN.KIND


# ---- 1. the built-in against the program ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,N", PN.PROGRAM_SHAPES)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_builtin_potential_equals_the_user_program_bit_for_bit(dtype, d, N):
    """bootstrap and independent proposals, gradient False / True / "exact", backward sampling and ancestor tracing, explicit and Threefry noise; the data have a
    missing component, a whole missing row and a partly missing row; ancestors, trajectories, particles, log-weights and resampling indices are compared"""
    from aux_ssm_samplers_amd import random as R
    T, Cn = PN.PROGRAM_T, PN.PROGRAM_CHAINS
    rng = np.random.default_rng(100 * d + N)
    dev, m, xtrue, delta = PN.case(d, T, rng, nan_steps=(3, T // 2, T - 2))
    assert np.isnan(m.y).any(axis=1).sum() == 3 and np.isnan(m.y[T // 2]).all()
    x0 = (xtrue[None] + 0.3 * rng.standard_normal((Cn, T, d))).astype(dtype)
    seen = GP.assert_program_equality(KIND, dev, x0, N, delta, GP.noise(Cn, T, N, d, rng, dtype), R.PRNGKey(31 + d))
    assert all((s[4] != 0).any() for s in seen)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_user_mean_program_keeps_the_builtin_potential(dtype):
    """a program that supplies only the transition mean (device_models.BUILTIN_LINEAR_MEAN_VJP, the built-in mean as user source) evaluates kind 6 through
    potential_rt / potential_grad_rt inside the program's kernels: the same sweep as the closed family, bit for bit, with and without the exact gradient weighting"""
    from aux_ssm_samplers_amd.csmc import DeviceGaussianDynamics, device_models as U
    d, N, T, Cn = 3, 100, 24, 3
    rng = np.random.default_rng(12)
    dev, m, xtrue, delta = PN.case(d, T, rng, nan_steps=(2, T // 2, T - 1))
    M0, G0, Mt, Gt = dev
    Mu = DeviceGaussianDynamics(U.BUILTIN_LINEAR_MEAN_VJP, Q=Mt.Q, theta=np.concatenate([np.reshape(Mt.F, -1), Mt.b]))
    x0 = (xtrue[None] + 0.3 * rng.standard_normal((Cn, T, d))).astype(dtype)
    nz = GP.noise(Cn, T, N, d, rng, dtype)
    for gradient in (False, "exact"):
        fb, fu = GP.describe("independent", dev, gradient), GP.describe("independent", (M0, G0, Mu, Gt), gradient)
        assert fb.potential == fu.potential == 6 and fb.user is None and fu.user is not None
        for backward in (False, True):
            assert (GP.assert_same_sweeps(fb, fu, x0, N, backward, delta, noise=nz)[0] != 0).any()


# ---- 2. literal parity -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("style,gradient,backward", P.LITERAL_CELLS + P.BOOTSTRAP_CELLS)
def test_sweep_fp64_equals_the_literal_sampler(style, gradient, backward):
    """register and wide path; a single case may update nothing, over the set every (style, gradient, backward) cell moves the trajectory somewhere"""
    GP.literal_cell_moves(KIND, style, gradient, backward)


# ---- 3. parallel in time ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gradient", [False, True])
@pytest.mark.parametrize("d,N,T", PN.PIT_CELLS)
def test_pit_sweep_fp64_equals_the_literal_tree(d, N, T, gradient):
    """origins identical, trajectory within 1e-12, after the margin condition of tests/pit_cases.margin_threshold on the literal"""
    GP.pit_equals_literal_tree(KIND, (d, N, T), gradient)


@pytest.mark.parametrize("gradient", [False, True])
@pytest.mark.parametrize("d,N,T", PN.PIT_CELLS)
def test_pit_sweep_fp32_keyed_equals_explicit_noise(d, N, T, gradient):
    assert (GP.pit_keyed_equals_explicit(KIND, (d, N, T), gradient) != 0).any()


# ---- 4. fp32 tie rate --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dx,N,T,style", [(24, 25, 250, "independent"), (24, 25, 250, "guided"), (4, 64, 1000, "independent")])
def test_fp32_ancestors_against_the_literal_order_tie_rate(dx, N, T, style):
    """the count workload on the wide path (dx = 24) and on the register path (dx = 4), 4 chains: the literal left-to-right draw on the device's own stored fp32
    log-weights (tests/potential_gpu.py::tie_rate_within_the_bar): disagreeing draws <= 2e-4 of all draws, none farther than one visible particle -- the project's
    bar for the SV and linear-Gaussian potentials.  Printed beside it, with no bar: the distance of the fp32 log-weights from the fp64 sweep on the same noise.
    Measured on an MI355X: DESIGN 4m."""
    from aux_ssm_samplers_amd.workloads import poisson_setup
    Cn = 4
    rng = np.random.default_rng(77)
    M0, Mt, G0, Gt, xtrue, y = poisson_setup(T, dx, seed=3)
    x0 = (xtrue[None] + 0.1 * rng.standard_normal((Cn, T, dx))).astype(np.float32)
    nz = GP.noise(Cn, T, N, dx, rng, np.float32)
    GP.tie_rate_within_the_bar(GP.describe(style, (M0, G0, Mt, Gt)), x0, N, nz, 0.2 / dx, f"{style} dx={dx} N={N} T={T}", against_fp64=True)


# ---- 5. resident chains ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,N,T,style", [(3, 100, 33, "independent"), (3, 100, 33, "guided"), (3, 100, 33, "pit"),
                                         (9, 25, 20, "independent"), (9, 25, 20, "guided"), (9, 25, 20, "pit")])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_resident_chains_equal_host_state_sweeps(dtype, d, N, T, style):
    """three sweeps on CsmcChains equal three host-state sweeps with the same keys, bit for bit: independent proposals with the exact gradient weighting, guided
    proposals with gradient, parallel in time; one register shape and one wide shape"""
    rng = np.random.default_rng(5 + d)
    dev, m, xtrue, delta = PN.case(d, T, rng, nan_steps=(1, 5, T - 1))
    GP.resident_equals_host(dev, (xtrue[None] + 0.3 * rng.standard_normal((4, T, d))).astype(dtype), delta, N, style)


# ---- 5b. more chains than CUs: the eight-wave fp32 wide kernels ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("style,gradient,backward", [("bootstrap", False, False), ("independent", False, True), ("independent", "exact", True), ("guided", True, True)])
@pytest.mark.parametrize("d,N,T", [(9, 25, 8), (32, 64, 5)])
def test_one_launch_equals_sixteen_wave_launches(d, N, T, style, gradient, backward):
    """k_cw2_fwd<float, 8, false, POIS> / k_cw2_bwd<float, 8> (fp32 with more chains than CUs) against the sixteen-wave instantiations that sections 1 - 4 hold:
    one launch of CUs + 3 chains is bit-identical to the same chains as launches of CUs and 3 (tests/potential_gpu.py::one_launch_equals_sixteen_wave); the data
    have a missing component, a whole missing row and a partly missing row"""
    dev, m, xtrue, delta = PN.case(d, T, np.random.default_rng([3, d, T]), nan_steps=(0, T // 2, T - 1))
    fk = GP.describe(style, dev, gradient)
    assert fk.potential == 6
    assert GP.one_launch_equals_sixteen_wave(fk, style, xtrue, delta, N, backward) > 0


# ---- 6. ground truth: the posterior by quadrature -------------------------------------------------------------------------------------------------------------
_models = {}


def _truth_model(which):
    """(a) register: d = 1, T = 6;  (b) wide: d = 6, T = 5, diagonal F, Q and P0 with distinct values per component, so the components are independent scalar
    models.  Returns (device objects, the parameters (m0, P0, F, Q, b) as vectors of the diagonals, y, the posterior's moments by quadrature, those of the
    posterior for the counts y + 1); built once and shared by the samplers of a model"""
    if which not in _models:
        rng = np.random.default_rng(2025)
        d, T = (1, 6) if which == "a" else (6, 5)
        k = np.arange(d)
        F, Q, P0 = 0.9 - 0.07 * k, 0.3 + 0.05 * k, 0.5 + 0.1 * k
        one = 1.0 - 0.1 * k
        m0, b = one + 0.2, one * (1 - F)
        assert d == 1 or (len(set(F)) == len(set(Q)) == len(set(P0)) == d)
        x = np.zeros((T, d))
        x[0] = m0 + np.sqrt(P0) * rng.standard_normal(d)
        for t in range(1, T):
            x[t] = F * x[t - 1] + b + np.sqrt(Q) * rng.standard_normal(d)
        y = rng.poisson(np.exp(x)).astype(np.float64)
        y[2, 0] = np.nan  # one missing count
        dev, m = PN.build(m0, np.diag(P0), np.diag(F), b, np.diag(Q), y)
        par = (m0, P0, F, Q, b)
        _models[which] = (dev, par, y, _moments(par, y), _moments(par, y + 1.0))
    return _models[which]


def _moments(par, y):
    """(E x_t, E x_t x_t^T) of the posterior, by quadrature component by component"""
    return P.independent_moments(lambda k: PN.scalar_steps(y[:, k]), y.shape[1], par)


_CASES6 = ([("a", s) for s in ("independent-trace", "independent-backward", "exact", "guided", "guided-gradient", "bootstrap", "pit", "pit-gradient")]
           + [("b", s) for s in ("independent-backward", "exact", "guided", "guided-gradient")])


@pytest.mark.parametrize("which,sampler", _CASES6)
def test_particle_gibbs_matches_the_posterior_by_quadrature(which, sampler):
    """1024 resident chains: every posterior mean and second moment (cross moments of a step included) within 5 empirical standard errors of the quadrature value --
    the standard error is the standard deviation of the per-chain time averages over sqrt(chains), the rule of tests/test_gpu_posterior_quadrature.py.  Power: the
    quadrature posterior for the counts y + 1 lies more than 10 of the same standard errors away in at least one compared moment."""
    dev, par, y, truth, other = _truth_model(which)
    m0, P0, F, Q, b = par
    T, d = y.shape
    # the step size, from the model alone: the gradient proposals N(u + delta/2 grad, delta/2 I) are one Langevin step, which contracts towards the mode only while
    # delta/2 lambda < 2, lambda the largest curvature of the negative log-target.  The Gaussian part's curvature is at most max_k (1 / P0_k + 1 / Q_k + F_k^2 / Q_k)
    # (the model is diagonal); the Poisson term's is exp(x_k), which near the mode lies between the prior intensity and the count -- bounded here by max(y) + 1.
    # delta = 2 / lambda lands on the mode along the stiffest direction.  All samplers of a case share it.
    lam = float(np.max(1.0 / P0 + 1.0 / Q + F * F / Q)) + float(np.nanmax(y)) + 1.0
    delta = 2.0 / lam
    N = 16 if which == "a" else 32
    # (burn-in: the chains start at x = 0, one prior standard deviation and more below the posterior, and a step moves them by sqrt(delta / 2) at most)
    est = GP.gibbs_moments(GP.kernel_of(sampler, dev, N), T, d, delta, 4000 if which == "a" else 5000, burn=200, with_delta=sampler != "bootstrap")
    GP.moments_match(est, truth, other, f"({which}) {sampler}: delta = {delta:.3f}", "the posterior for the counts y + 1")


# ---- 7. the C entry points --------------------------------------------------------------------------------------------------------------------------------
def test_c_entry_points_refuse_missing_observations_and_an_unknown_kind():
    T, N, d = 6, 64, 2
    dev, m, xtrue, _ = PN.case(d, T, np.random.default_rng(0))
    ep = GP.EntryPoints(dev, T, N, d, x=1.0, sqrt_half_delta=0.3)
    ms = ep.struct()
    assert ms.potential == 6
    ms.y = None
    ep.both_refuse(ms, "observations y")
    ms = ep.struct()
    ms.potential = 7
    ep.both_refuse(ms, "unknown potential kind 7")
    ms = ep.struct()
    assert ep.sweep(ms) == 0 and ep.pit_sweep(ms) == 0  # and the untampered description runs
