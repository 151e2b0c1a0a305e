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
4. fp32 by the teacher-forced tie-rate rule of tests/potential_gpu.py::tie_rate, on the wide and on the register path; the distance of the fp32 log-weights from
   the fp64 sweep on the same noise is printed (no bar is set on it).
5. Resident chains; and fp32 with more chains than CUs (the eight-wave wide kernels) against the sixteen-wave launches.
6. Ground truth: the posterior of the scalar model by quadrature (tests/potential_np.py::posterior_by_quadrature); with diagonal F, Q and P0 the components of a
   d = 6 model are independent, so every marginal is its own quadrature answer.
7. The C entry points' refusals.

The assertion blocks are those of tests/potential_gpu.py, run with this kind's record."""
import numpy as np
import pytest

from tests import logistic_np as LN
from tests import potential_gpu as GP
from tests import potential_np as P

pytestmark = pytest.mark.gpu
KIND = LN.KIND


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
    seen = GP.assert_program_equality(KIND, dev, x0, N, delta, GP.noise(Cn, T, N, d, rng, dtype), R.PRNGKey(31 + d))
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
    seen = GP.assert_program_equality(KIND, dev, x0, N, 1e-4, GP.noise(Cn, T, N, d, rng, dtype), R.PRNGKey(3))
    assert max(float(np.abs(s[5]).max()) for s in seen) > 1e4  # (log-weights of order m |x|: far from the mode, and finite)


@pytest.mark.parametrize("family", LN.FAMILIES)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_user_mean_program_keeps_the_builtin_potential(dtype, family):
    """a program that supplies only the transition mean (device_models.BUILTIN_LINEAR_MEAN_VJP, the built-in mean as user source) evaluates kind 8 through
    potential_rt / potential_grad_rt inside the program's kernels, the sizes loaded from plane 1 at run time: the same sweep as the closed family, bit for bit"""
    from aux_ssm_samplers_amd.csmc import DeviceGaussianDynamics, device_models as U
    d, N, T, Cn = 3, 100, 24, 3
    rng = np.random.default_rng(12)
    dev, m, xtrue, delta = LN.case(d, T, rng, family, nan_steps=(2, T // 2, T - 1))
    M0, G0, Mt, Gt = dev
    Mu = DeviceGaussianDynamics(U.BUILTIN_LINEAR_MEAN_VJP, Q=Mt.Q, theta=np.concatenate([np.reshape(Mt.F, -1), Mt.b]))
    x0 = (xtrue[None] + 0.3 * rng.standard_normal((Cn, T, d))).astype(dtype)
    nz = GP.noise(Cn, T, N, d, rng, dtype)
    for gradient in (False, "exact"):
        fb, fu = GP.describe("independent", dev, gradient), GP.describe("independent", (M0, G0, Mu, Gt), gradient)
        assert fb.potential == fu.potential == 8 and fb.user is None and fu.user is not None
        for backward in (False, True):
            assert (GP.assert_same_sweeps(fb, fu, x0, N, backward, delta, noise=nz)[0] != 0).any()


# ---- 2. literal parity -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("style,gradient,backward", P.LITERAL_CELLS + P.BOOTSTRAP_CELLS)
def test_sweep_fp64_equals_the_literal_sampler(style, gradient, backward):
    """register and wide path; a single case may update nothing, over the set every (style, gradient, backward) cell moves the trajectory somewhere"""
    GP.literal_cell_moves(KIND, style, gradient, backward)


# ---- 3. parallel in time ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gradient", [False, True])
@pytest.mark.parametrize("d,N,T", LN.PIT_CELLS)
def test_pit_sweep_fp64_equals_the_literal_tree(d, N, T, gradient):
    """origins identical, trajectory within 1e-12, after the margin condition of tests/pit_cases.margin_threshold on the literal"""
    GP.pit_equals_literal_tree(KIND, (d, N, T), gradient)


@pytest.mark.parametrize("gradient", [False, True])
@pytest.mark.parametrize("d,N,T", LN.PIT_CELLS)
def test_pit_sweep_fp32_keyed_equals_explicit_noise(d, N, T, gradient):
    assert (GP.pit_keyed_equals_explicit(KIND, (d, N, T), gradient) != 0).any()


# ---- 4. fp32 tie rate --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dx,N,T,style,family", [(24, 25, 250, "independent", "binomial"), (24, 25, 250, "guided", "negbinomial"), (4, 64, 1000, "independent", "binomial"),
                                                 (4, 64, 1000, "independent", "negbinomial")])
def test_fp32_ancestors_against_the_literal_order_tie_rate(dx, N, T, style, family):
    """workloads.logistic_setup on the wide path (dx = 24) and on the register path (dx = 4), 4 chains: the literal left-to-right draw on the device's own stored
    fp32 log-weights (tests/potential_gpu.py::tie_rate_within_the_bar): disagreeing draws <= 2e-4 of all draws, none farther than one visible particle -- the
    project's standing bar.  Printed beside it, with no bar: the distance of the fp32 log-weights from the fp64 sweep on the same noise.
    Measured on an MI355X: DESIGN 4q."""
    from aux_ssm_samplers_amd.workloads import logistic_setup
    Cn = 4
    rng = np.random.default_rng(77)
    M0, Mt, G0, Gt, xtrue, y, _ = logistic_setup(T, dx, family, seed=3)
    x0 = (xtrue[None] + 0.1 * rng.standard_normal((Cn, T, dx))).astype(np.float32)
    nz = GP.noise(Cn, T, N, dx, rng, np.float32)
    fk = GP.describe(style, (M0, G0, Mt, Gt))
    assert fk.potential == 8
    GP.tie_rate_within_the_bar(fk, x0, N, nz, 0.2 / dx, f"{family} {style} dx={dx} N={N} T={T}", against_fp64=True)


# ---- 5. resident chains ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,N,T,style,family", [(3, 100, 33, "independent", "binomial"), (3, 100, 33, "guided", "negbinomial"), (3, 100, 33, "pit", "binomial"),
                                                (9, 25, 20, "independent", "negbinomial"), (9, 25, 20, "guided", "binomial"), (9, 25, 20, "pit", "negbinomial")])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_resident_chains_equal_host_state_sweeps(dtype, d, N, T, style, family):
    """three sweeps on CsmcChains equal three host-state sweeps with the same keys, bit for bit: independent proposals with the exact gradient weighting, guided
    proposals with gradient, parallel in time; one register shape and one wide shape"""
    rng = np.random.default_rng(5 + d)
    dev, m, xtrue, delta = LN.case(d, T, rng, family, nan_steps=(1, 5, T - 1))
    assert LN.has_every_feature(m)
    GP.resident_equals_host(dev, (xtrue[None] + 0.3 * rng.standard_normal((4, T, d))).astype(dtype), delta, N, style)


# ---- 5b. more chains than CUs: the eight-wave fp32 wide kernels ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("style,gradient,backward", [("bootstrap", False, False), ("independent", False, True), ("independent", "exact", True), ("guided", True, True)])
@pytest.mark.parametrize("d,N,T,family", [(9, 25, 8, "binomial"), (32, 64, 5, "negbinomial")])
def test_one_launch_equals_sixteen_wave_launches(d, N, T, family, style, gradient, backward):
    """k_cw2_fwd<float, 8, false, LOGI> / k_cw2_bwd<float, 8> (fp32 with more chains than CUs) against the sixteen-wave instantiations that sections 1 - 4 hold:
    one launch of CUs + 3 chains is bit-identical to the same chains as launches of CUs and 3 (tests/potential_gpu.py::one_launch_equals_sixteen_wave)"""
    dev, m, xtrue, delta = LN.case(d, T, np.random.default_rng([3, d, T]), family, nan_steps=(0, T // 2, T - 1))
    assert LN.has_every_feature(m)
    fk = GP.describe(style, dev, gradient)
    assert fk.potential == 8
    assert GP.one_launch_equals_sixteen_wave(fk, style, xtrue, delta, N, backward) > 0


# ---- 6. ground truth: the posterior by quadrature -------------------------------------------------------------------------------------------------------------
_models = {}


def _truth_model(which):
    """"a": d = 1, T = 6, binomial with trials in 1 .. 20;  "binary": the same with trials = 1;  "nb": d = 1, T = 6, negative binomial with r = 0.5;  "b": d = 6,
    T = 5, negative binomial with r in {0.5, 1, 3} per component and diagonal F, Q and P0 with distinct values per component, so the components are independent
    scalar models.  Returns (device objects, the parameters (m0, P0, F, Q, b) as vectors of the diagonals, y, family, the sizes m (T, d), the posterior's moments by
    quadrature, those of the posterior for the data y + 1 (binomial: trials + 1 as well, so that the data stay valid; negative binomial: the same r)); built once
    and shared by the samplers of a model"""
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
        par5 = (m0, P0, F, Q, b)
        size, size1 = (par, par + 1.0) if family == "binomial" else (y + par, y + 1.0 + par)
        _models[which] = (dev, par5, y, family, size, _moments(par5, y, size), _moments(par5, y + 1.0, size1))
    return _models[which]


def _moments(par, y, size):
    """(E x_t, E x_t x_t^T) of the posterior, by quadrature component by component"""
    return P.independent_moments(lambda k: LN.scalar_steps(y[:, k], size[:, k]), y.shape[1], par)


_CASES6 = ([("a", s) for s in ("independent-trace", "independent-backward", "exact", "guided", "guided-gradient", "bootstrap", "pit", "pit-gradient")]
           + [("b", s) for s in ("independent-backward", "exact", "guided", "guided-gradient")] + [("binary", "exact"), ("nb", "guided-gradient")])


@pytest.mark.parametrize("which,sampler", _CASES6)
def test_particle_gibbs_matches_the_posterior_by_quadrature(which, sampler):
    """1024 resident chains: every posterior mean and second moment (cross moments of a step included) within 5 empirical standard errors of the quadrature value --
    the standard error is the standard deviation of the per-chain time averages over sqrt(chains), the rule of tests/test_gpu_posterior_quadrature.py.  Power: the
    quadrature posterior for the data y + 1 (binomial: trials + 1 as well, so that the data stay valid; negative binomial: the same r) lies more than 10 of the same
    standard errors away in at least one compared moment."""
    dev, par, y, family, size, truth, other = _truth_model(which)
    m0, P0, F, Q, b = par
    T, d = y.shape
    # the step size, from the model alone: the gradient proposals N(u + delta/2 grad, delta/2 I) are one Langevin step, which contracts towards the mode only while
    # delta/2 lambda < 2, lambda the largest curvature of the negative log-target.  The Gaussian part's curvature is at most max_k (1 / P0_k + 1 / Q_k + F_k^2 / Q_k)
    # (the model is diagonal); the logistic term's is m sigma (1 - sigma) <= m / 4.  delta = 2 / lambda lands on the mode along the stiffest direction.
    lam = float(np.max(1.0 / P0 + 1.0 / Q + F * F / Q)) + float(np.nanmax(np.where(np.isfinite(y), size, np.nan))) / 4.0
    delta = 2.0 / lam
    N = 32 if which == "b" else 16
    est = GP.gibbs_moments(GP.kernel_of(sampler, dev, N), T, d, delta, 5000 if which == "b" else 4000, burn=200, with_delta=sampler != "bootstrap")
    GP.moments_match(est, truth, other, f"({which}, {family}) {sampler}: delta = {delta:.3f}",
                     "the posterior for the data y + 1")


# ---- 7. the C entry points --------------------------------------------------------------------------------------------------------------------------------
def test_c_entry_points_refuse_missing_observations_and_unknown_kinds():
    T, N, d = 6, 64, 2
    dev, m, xtrue, _ = LN.case(d, T, np.random.default_rng(0))
    ep = GP.EntryPoints(dev, T, N, d, x=1.0, sqrt_half_delta=0.3)
    ms = ep.struct()
    assert ms.potential == 8
    ms.y = None
    ep.both_refuse(ms, "observations y")
    for kind in (7, 9):
        ms = ep.struct()
        ms.potential = kind
        ep.both_refuse(ms, f"unknown potential kind {kind}")
    ms = ep.struct()
    assert ep.sweep(ms) == 0 and ep.pit_sweep(ms) == 0  # and the untampered description runs
    with pytest.raises(ValueError, match="time steps"):
        ep.struct(T + 1)
