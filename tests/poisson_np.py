"""The Poisson count potential (AUXSSM_POT_POISSON) for the literal NumPy cSMC (tests/potential_np.py on oracle/csmc_np.py, oracle/pit_np.py, tests/guided_np.py)
and the cases the tests of this potential share.  Test infrastructure only, written independently of the package:

    log g_t(x) = sum_k [ y_{t,k} x_k - exp(x_k) ]   over the components whose y_{t,k} is finite (the -log y! constant left out)

with np.exp and a masked np.sum -- neither the kernels' det_exp nor their fused multiply-add: agreement is to rounding."""
import functools

import numpy as np

from oracle import csmc_np as L
from tests import pit_cases as PC
from tests import potential_np as P


def log_g(x, y):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        v = y * np.atleast_2d(x) - np.exp(np.atleast_2d(x))
    v = np.sum(np.where(np.isfinite(y), v, 0.0), axis=-1)
    return v if x.ndim > 1 else v[0]


def grad_log_g(x, y):
    """d log g / dx_k = y_k - exp(x_k); 0 for a missing component"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        g = np.where(np.isfinite(y), y - np.exp(x), 0.0)
    return g


def bound(y):
    """sup_x log g = sum_k (y_k > 0 ? y_k (log y_k - 1) : 0), attained at x_k = log y_k"""
    y = np.asarray(y, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.sum(np.where(y > 0, y * (np.log(np.where(y > 0, y, 1.0)) - 1.0), 0.0)))


def potential(y, first=False):
    """g_t as a protocol object of oracle/csmc_np.py: of the rows y[1:] or (first) of row y[0]"""
    return P.RowPotential(KIND, y, (), first)


def scalar_steps(y):
    """log g_t of the scalar model y_t ~ Poisson(exp(x_t)) for tests/potential_np.py::posterior_by_quadrature (NaN: not observed)"""
    return [functools.partial(log_g, y=[v]) for v in np.asarray(y, np.float64).reshape(-1)]


# ---- cases: the model on both sides ---------------------------------------------------------------------------------------------------------------------
def build(m0, P0, F, b, Q, y):
    """(device objects (M0, G0, Mt, Gt), literal Model) of one model"""
    from aux_ssm_samplers_amd import csmc
    T = y.shape[0]
    M0, Mt = csmc.GaussianInit(m0=m0, P0=P0), csmc.LinearGaussianDynamics(F=F, b=b, Q=Q)
    dev = (M0, csmc.PoissonPotential(y=y[0]), Mt, csmc.PoissonPotential(params=y[1:]))
    return dev, P.Model(KIND, m0, P0, L.LinearGaussianDynamics(F, b, np.linalg.cholesky(Q), T), Q, y)


def case(d, T, rng, nan_steps=()):
    """tests/potential_np.py::dynamics moved to a stationary mean of about 1 (intensities around e), observed as counts.  nan_steps: up to three time steps with
    missing data (tests/potential_np.py::knock_out).  Returns (device objects (M0, G0, Mt, Gt), literal Model, a trajectory, delta in [0.1, 0.4] / d: proposals that
    N <= 64 particles can follow at every d, below the Langevin stability limit of the gradient proposals at these intensities)."""
    m0, P0, F, b, Q = P.dynamics(d, rng, level=1.0)
    x = P.trajectory(m0, P0, F, b, Q, T, rng)
    y = rng.poisson(np.exp(x)).astype(np.float64)
    P.knock_out(y, nan_steps)
    dev, m = build(m0, P0, F, b, Q, y)
    return dev, m, x, (0.1 + 0.3 * rng.random(T)) / d


def program(dev, grad=False):
    """the same model with the potential as user source (device_models.BUILTIN_POISSON: value, bound and gradient in one source; no theta)"""
    from aux_ssm_samplers_amd.csmc import DevicePotential, device_models as U
    M0, G0, Mt, Gt = dev
    d = int(np.size(G0.y))
    return M0, DevicePotential(U.BUILTIN_POISSON, y=G0.y, p=d), Mt, DevicePotential(U.BUILTIN_POISSON, params=np.reshape(Gt.params, (-1, d)), p=d)


# ---- the cases of tests/test_gpu_poisson.py, shared with the CPU tests that vouch for them (well-posedness of the ancestor comparison) -----------------------
PROGRAM_SHAPES = [(d, N) for d in (1, 2, 4) for N in (64, 100, 1024)]  # (d, N) at T = 40, 3 chains
PROGRAM_T, PROGRAM_CHAINS = 40, 3
REGISTER = [(d, N, 33) for d in (1, 3) for N in (64, 100)]       # (d, N, T)
WIDE = [(d, N, 25) for d in (5, 13, 32) for N in (25, 64)]
PIT_CELLS = ((1, 32, 25), (3, 100, 33), (1, 100, 25), (6, 25, 25), (13, 32, 33))  # (d, N, T): three register cells, two wide ones


def _literal_model(shape, rng):
    """NaN entries at t = 0 (one component), mid-series (the whole row) and T - 1 (all but the last component)"""
    d, N, T = shape
    return shape + case(d, T, rng, nan_steps=(0, T // 2, T - 1))


def _pit_model(cell, rng):
    """missing data at t = 0 (one component), on the top-level stitch boundary (the whole row) and at the last step (all but the last component)"""
    d, N, T = cell
    return cell + case(d, T, rng, nan_steps=(0, PC.top_boundary(T), T - 1))


# the seeds advance until the cell is well-posed (at N <= 100 and T <= 33 a first seed fails about once in a hundred cells)
KIND = P.Kind("poisson", 6, log_g, grad_log_g, cells=lambda style, gradient, backward: REGISTER + WIDE, literal_model=_literal_model,
              seeds=lambda style, gradient, backward, shape: ([6000 + P.seed_index(style, gradient, backward), *shape, bump] for bump in range(P.MAX_BUMPS)),
              label=lambda shape: "d={} N={} T={}".format(*shape),
              pit_cells=PIT_CELLS, pit_model=_pit_model, pit_seeds=lambda cell, gradient: ([17, *cell, int(gradient), bump] for bump in range(P.MAX_BUMPS)),
              program=program)
