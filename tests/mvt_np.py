"""The multivariate Student-t potential (AUXSSM_POT_MVT) for the literal NumPy cSMC (tests/potential_np.py on oracle/csmc_np.py), and the cases the tests of this
potential share.  Test infrastructure only.

    log g_t(x) = -(nu + d) / 2 log(1 + (x - y_t)^T prec (x - y_t) / nu),   NaN -> 0          (examples/spatial/t_distribution.py:98-104, model.py:121-124)

written here with NumPy's own matrix product and log1p -- not in the kernels' operation order: agreement is to rounding, not bit for bit."""
import numpy as np

from oracle import csmc_np as L
from tests import guided_np as G
from tests import potential_np as P


def log_g(x, y, nu, prec):
    x = np.asarray(x)
    r = np.atleast_2d(x) - np.asarray(y, x.dtype)
    with np.errstate(invalid="ignore"):
        q = np.sum((r @ np.asarray(prec, x.dtype).T) * r, axis=-1)
        v = -x.dtype.type(0.5 * (nu + r.shape[-1])) * np.log1p(q / x.dtype.type(nu))
    v = np.where(np.isnan(v), x.dtype.type(0), v)
    return v if x.ndim > 1 else v[0]


def grad_log_g(x, y, nu, prec):
    """d log g / dx = -(nu + d) / (nu + q) prec (x - y); 0 where the value was NaN"""
    x = np.asarray(x, np.float64)
    r = x - np.asarray(y, np.float64)
    z = r @ np.asarray(prec).T
    with np.errstate(invalid="ignore"):
        q = np.sum(z * r, axis=-1, keepdims=True)
        g = -(nu + x.shape[-1]) / (nu + q) * z
    return np.where(np.isnan(g), 0.0, g)


def potential(nu, prec, y, first=False):
    """g_t as a protocol object of oracle/csmc_np.py: of the rows y[1:] or (first) of row y[0]"""
    return P.RowPotential(KIND, y, (float(nu), np.asarray(prec, np.float64)), first)


def model(m0, P0, dyn, Q, nu, prec, y):
    return P.Model(KIND, m0, P0, dyn, Q, y, (float(nu), np.asarray(prec, np.float64)), nu=float(nu), prec=np.asarray(prec, np.float64))


# ---- cases: the model on both sides ---------------------------------------------------------------------------------------------------------------------
def case(d, T, rng, nu=4.0, prec=None, nan_rows=(), walk=False, tv=False):
    """linear-Gaussian dynamics with the multivariate-t potential: tests/potential_np.py::dynamics, or (walk) the spatial example's random walk
    x_t = x_{t-1} + eps, or (tv) the former with an F_t, b_t and Q_t of its own for each of the T - 1 transitions; prec: default a dense random SPD
    matrix.  nan_rows: time steps whose observation has a NaN component (the step is flat).
    Returns (device objects (M0, G0, Mt, Gt), literal Model, a trajectory, delta in [0.2, 0.8] / d: proposals that N <= 64 particles can follow at every d)."""
    from aux_ssm_samplers_amd.csmc import GaussianInit, LinearGaussianDynamics, MultivariateTPotential
    m0, P0, F, b, Q = (np.zeros(d), np.eye(d), np.eye(d), np.zeros(d), np.eye(d)) if walk else P.dynamics(d, rng)
    Q0 = Q
    if tv:
        F = F + 0.05 * rng.standard_normal((T - 1, d, d)) / np.sqrt(d)
        b = b + 0.05 * rng.standard_normal((T - 1, d))
        Q = np.stack([G.spd(d, rng) for _ in range(T - 1)])
        Q0 = Q[0]
    if prec is None:
        A = rng.standard_normal((d, d))
        prec = 1.5 * np.eye(d) + 0.8 * (A @ A.T) / d
        prec = 0.5 * (prec + prec.T)
    x = P.trajectory(m0, P0, F, b, Q, T, rng)
    Lc = np.linalg.cholesky(np.linalg.inv(prec))
    y = x + (rng.standard_normal((T, d)) @ Lc.T) / np.sqrt(rng.chisquare(nu, T) / nu)[:, None]
    for i, t in enumerate(nan_rows):
        y[t, i % d] = np.nan
    M0, Mt = GaussianInit(m0=m0, P0=P0), LinearGaussianDynamics(F=F, b=b, Q=Q)
    dev = (M0, MultivariateTPotential(nu=nu, prec=prec, y=y[0]), Mt, MultivariateTPotential(nu=nu, prec=prec, params=y[1:]))
    m = model(m0, P0, L.LinearGaussianDynamics(F, b, np.linalg.cholesky(Q), T), Q0, nu, prec, y)
    m.tv = tv
    return dev, m, x, (0.2 + 0.6 * rng.random(T)) / d


def program(dev, grad=False):
    """the same model with the potential as user source (device_models.BUILTIN_MVT[_GRAD]), theta = [nu, prec row-major]"""
    from aux_ssm_samplers_amd.csmc import DevicePotential, device_models as U
    M0, G0, Mt, Gt = dev
    src = U.BUILTIN_MVT_GRAD if grad else U.BUILTIN_MVT
    theta = np.concatenate([[G0.nu], np.reshape(G0.prec, -1)])
    d = G0.dx
    return M0, DevicePotential(src, y=G0.y, theta=theta, p=d), Mt, DevicePotential(src, params=Gt.params, theta=theta, p=d)


# ---- the cases of tests/test_gpu_mvt.py ---------------------------------------------------------------------------------------------------------------------
# register path (1, 1024, 40), (3, 100, 33); wide path (5, 33, 20), the 3 x 3 and 5 x 5 grids of the spatial example (random walk, its precision matrix; nu = 1 on
# the 5 x 5 grid, the example's own value) and (32, 64, 12); time-varying transitions on the register path at N = 65, 512 and 1024 (a partial last wave, eight and
# sixteen full waves: this potential runs the generic workgroup at every N), three steps
LITERAL_CASES = dict(r1=(1, 1024, 40), r3=(3, 100, 33), w5=(5, 33, 20), grid3=(9, 25, 20), grid5=(25, 25, 25), w32=(32, 64, 12),
                     tv65=(1, 65, 3), tv512=(1, 512, 3), tv1024=(1, 1024, 3))  # (d, N, T)
TIME_VARYING = ("tv65", "tv512", "tv1024")
BOOTSTRAP_CASES = ("r3", "grid3")


def _cells(style, gradient, backward):
    if style == "bootstrap":
        return BOOTSTRAP_CASES
    return tuple(n for n in LITERAL_CASES if style != "guided" or n not in TIME_VARYING)  # (guided: time-invariant transitions only)


def _literal_model(name, rng):
    from aux_ssm_samplers_amd.workloads import spatial_precision
    d, N, T = LITERAL_CASES[name]
    if name in TIME_VARYING:
        out = case(d, T, rng, tv=True)
    elif name.startswith("grid"):
        out = case(d, T, rng, nu=1.0 if name == "grid5" else 3.0, prec=spatial_precision(int(name[-1])), walk=True, nan_rows=(4,))
    else:
        out = case(d, T, rng, nan_rows=(2, T - 1))
    return (d, N, T) + out


def _seeds(style, gradient, backward, name):
    """one seed per (case, backward), whatever the style: these cases predate the well-posedness advance of the later potentials and have none"""
    return [(7100 if style == "bootstrap" else 7000 + 10 * list(LITERAL_CASES).index(name)) + backward]


KIND = P.Kind("mvt", 4, log_g, grad_log_g, cells=_cells, literal_model=_literal_model, seeds=_seeds,
              label=lambda name: "{} (d={} N={} T={})".format(name, *LITERAL_CASES[name]), program=program)
