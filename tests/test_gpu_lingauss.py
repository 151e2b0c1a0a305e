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
7. The C entry points' refusals.

The assertion blocks are those of tests/potential_gpu.py, run with this kind's record."""
import numpy as np
import pytest

from tests import lingauss_np as LG
from tests import potential_gpu as GP
from tests import potential_np as P

pytestmark = pytest.mark.gpu
KIND = LG.KIND


# ---- 1. the built-in against the program ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,dy,N,T,Cn", LG.PROGRAM_SHAPES)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_builtin_potential_equals_the_user_program_bit_for_bit(dtype, d, dy, N, T, Cn):
    """bootstrap and independent proposals, gradient False / True / "exact", both backward modes, explicit and Threefry noise; two observation rows carry a NaN,
    c != 0; every case moves the trajectory"""
    from aux_ssm_samplers_amd import random as R
    rng = np.random.default_rng(100 * d + N)
    dev, m, xtrue, delta = LG.case(d, dy, T, rng, nan_rows=(3, T - 2))
    assert np.all(m.c != 0) and np.isnan(m.y).any(axis=1).sum() == 2
    x0 = (xtrue[None] + 0.3 * rng.standard_normal((Cn, T, d))).astype(dtype)
    seen = GP.assert_program_equality(KIND, dev, x0, N, delta, GP.noise(Cn, T, N, d, rng, dtype), R.PRNGKey(31 + d))
    assert all((s[4] != 0).any() for s in seen)


# ---- 2. literal parity -----------------------------------------------------------------------------------------------------------------------------------
def _flat_rows_and_literal(style, gradient, backward, name):
    """tests/potential_gpu.py::against_literal on a case whose observations have a NaN at t = 0, mid-series and T - 1"""
    d, N, T, dev, m = P.literal_sweep(KIND, style, gradient, backward, name)[1][:5]
    assert np.all(np.isnan(m.y[[0, T // 2, T - 1]]).any(axis=1))
    return GP.against_literal(KIND, style, gradient, backward, name)


@pytest.mark.parametrize("style,gradient,backward", P.LITERAL_CELLS)
def test_sweep_fp64_equals_the_literal_sampler(style, gradient, backward):
    """register and wide path; a single case may update nothing, over the set every (style, gradient, backward) cell moves the trajectory somewhere"""
    moved = 0
    for name in LG.REGISTER + LG.WIDE:
        moved += int((_flat_rows_and_literal(style, gradient, backward, name) != 0).sum())
    assert moved > 0


@pytest.mark.parametrize("backward", [False, True])
@pytest.mark.parametrize("name", LG.BOOTSTRAP_CASES)
def test_bootstrap_sweep_fp64_equals_the_literal_sampler(name, backward):
    assert (_flat_rows_and_literal("bootstrap", False, backward, name) != 0).any()


# ---- 3. fp32 tie rate --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dx,dy,N,T,style", [(24, 12, 25, 250, "independent"), (24, 12, 25, 250, "guided"), (4, 2, 64, 1000, "independent")])
def test_fp32_ancestors_against_the_literal_order_tie_rate(dx, dy, N, T, style):
    """the tracking workload on the wide path (dx = 24, dy = 12, which no contract oracle covers in fp32) and on the register path (dx = 4, dy = 2), 4 chains: the
    literal left-to-right draw on the device's own stored fp32 log-weights (tests/test_gpu_csmc_literal.py's rule): disagreeing draws <= 2e-4 of all draws, none
    farther than one visible particle"""
    from aux_ssm_samplers_amd.workloads import lgssm_tracking_setup
    Cn = 4
    rng = np.random.default_rng(77)
    M0, Mt, G0, Gt, xtrue, y, H, R = lgssm_tracking_setup(T, dx, dy, seed=3)
    x0 = (xtrue[None] + 0.3 * rng.standard_normal((Cn, T, dx))).astype(np.float32)
    nz = GP.noise(Cn, T, N, dx, rng, np.float32)
    GP.tie_rate_within_the_bar(GP.describe(style, (M0, G0, Mt, Gt)), x0, N, nz, 0.1, f"{style} dx={dx} dy={dy} N={N} T={T}")


# ---- 4. parallel in time ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gradient", [False, True])
@pytest.mark.parametrize("d,dy,N,T", LG.PIT_CELLS)
def test_pit_sweep_fp64_equals_the_literal_tree(d, dy, N, T, gradient):
    """origins identical, trajectory within 1e-12, after the margin condition of tests/pit_cases.margin_threshold on the literal"""
    GP.pit_equals_literal_tree(KIND, (d, dy, N, T), gradient)


@pytest.mark.parametrize("gradient", [False, True])
@pytest.mark.parametrize("d,dy,N,T", LG.PIT_CELLS)
def test_pit_sweep_fp32_keyed_equals_explicit_noise(d, dy, N, T, gradient):
    assert (GP.pit_keyed_equals_explicit(KIND, (d, dy, N, T), gradient, delta=0.4) != 0).mean() > 0.2


# ---- 5. resident chains ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,dy,N,T,style", [(3, 2, 100, 33, "independent"), (3, 2, 100, 33, "guided"), (3, 2, 100, 33, "pit"),
                                            (9, 4, 25, 20, "independent"), (9, 4, 25, 20, "guided")])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_resident_chains_equal_host_state_sweeps(dtype, d, dy, N, T, style):
    """three sweeps on CsmcChains equal three host-state sweeps with the same keys, bit for bit: independent proposals with the exact gradient weighting, guided
    proposals with gradient, parallel in time (register kernels only: dx <= 4)"""
    rng = np.random.default_rng(5 + d)
    dev, m, xtrue, delta = LG.case(d, dy, T, rng, nan_rows=(1,))
    GP.resident_equals_host(dev, (xtrue[None] + 0.3 * rng.standard_normal((4, T, d))).astype(dtype), delta, N, style)


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


_CASES6 = ([("a", s) for s in ("independent-trace", "independent-backward", "exact", "guided", "guided-gradient", "bootstrap", "pit", "pit-gradient")]
           + [("b", s) for s in ("independent-backward", "exact", "guided", "guided-gradient")])


@pytest.mark.parametrize("which,sampler", _CASES6)
def test_particle_gibbs_matches_the_exact_gaussian_posterior(which, sampler):
    """1024 resident chains: every posterior mean and second moment (cross moments of a step included) within 5 empirical standard errors of the exact value -- the
    standard error is the standard deviation of the per-chain time averages over sqrt(chains), the rule of tests/test_gpu_posterior_quadrature.py.  Power: the
    exact posterior with the coupling entries of H zeroed lies more than 10 of the same standard errors away in at least one compared moment."""
    dev, m, m_zeroed = _truth_model(which)
    T, d = m.y.shape[0], m.m0.shape[0]
    # the step size, from the model alone: the gradient proposals N(u + delta/2 grad, delta/2 I) are one Langevin step, which on a Gaussian target with joint
    # precision J contracts towards the mode only while delta/2 lambda_max(J) < 2 and lands on it along the stiffest direction at delta = 2 / lambda_max(J); a
    # larger delta leaves every sampler valid but the gradient ones overshoot and 60 sweeps of burn-in no longer forget the start.  All samplers of a case share it.
    N = 16 if which == "a" else 32
    delta = min(0.6 if which == "a" else 0.3, 2.0 / float(np.linalg.eigvalsh(np.linalg.inv(LG.exact_posterior(m)[1])).max()))
    est = GP.gibbs_moments(GP.kernel_of(sampler, dev, N), T, d, delta, 2000 if which == "a" else 3000, with_delta=sampler != "bootstrap")
    GP.moments_match(est, _moments(m), _moments(m_zeroed), f"({which}) {sampler}", "the posterior with H's coupling zeroed")


# ---- 7. the C entry points --------------------------------------------------------------------------------------------------------------------------------
def test_c_entry_points_refuse_a_missing_observation_matrix_and_missing_observations():
    T, N, d = 6, 64, 2
    dev, m, xtrue, _ = LG.case(d, 1, T, np.random.default_rng(0))
    ep = GP.EntryPoints(dev, T, N, d, x=0.0, sqrt_half_delta=0.5)
    for field, msg in (("obs_H", "obs_H"), ("y", "observations y")):
        ms = ep.struct()
        assert ms.potential == 5
        setattr(ms, field, None)
        ep.both_refuse(ms, msg)
    ms = ep.struct()
    assert ep.sweep(ms) == 0 and ep.pit_sweep(ms) == 0  # and the untampered description runs
