"""The closed Feynman-Kac model family the HIP cSMC kernels evaluate in-kernel (include/auxssm.h, auxssm_fk_model).

They subclass the reference's protocol classes so they can be passed wherever the reference takes
(M0, G0, Mt, Gt, Pt); the kernels read their parameters, they never call Python methods on the hot path."""
from dataclasses import dataclass, field
from typing import Any, Optional

import numpy as np

from .. import _logistic
from .._primitives.csmc.base import Distribution, UnivariatePotential, Dynamics, Potential


@dataclass
class GaussianInit(Distribution, UnivariatePotential):
    """M0 = N(m0, P0) (e.g. test_csmc/common.py:34-49; examples/stochastic_volatility/auxiliary_csmc.py:21-27).
    Used as a potential it is log N(x; m0, P0)."""
    m0: Any
    P0: Any

    def chol(self):
        return np.linalg.cholesky(np.atleast_2d(np.asarray(self.P0, np.float64)))


@dataclass
class LinearGaussianDynamics(Dynamics, Potential):
    """x_{t+1} | x_t ~ N(F x_t + b, Q) (test_csmc/common.py:11-31; SV auxiliary_csmc.py:29-37).  Time-invariant: F (d, d), b (d,), Q (d, d);
    time-varying (the reference scans Mt.params over time, _primitives/csmc/csmc.py:103): F (T-1, d, d), b (T-1, d), Q (T-1, d, d), row t =
    the transition t -> t + 1."""
    F: Any
    b: Any
    Q: Any
    params: Optional[Any] = None

    @property
    def time_varying(self):
        return np.ndim(self.F) == 3

    def chol(self):
        """lower Cholesky factor(s) of Q: (d, d), or (T-1, d, d) when time-varying"""
        Q = np.asarray(self.Q, np.float64)
        return np.linalg.cholesky(Q if Q.ndim == 3 else np.atleast_2d(Q))


@dataclass
class FlatPotential(UnivariatePotential, Potential):
    """G = 0 (test_csmc/common.py:61-75)."""
    params: Optional[Any] = None


@dataclass
class GaussianObsPotential(UnivariatePotential, Potential):
    """log N(y_t; x_t, sig^2 I).  As G0 give y=(d,) [the reference uses GaussianDistribution(mu=y0, sig) there,
    test_csmc.py:88]; as Gt give params = ys[1:] (test_csmc/common.py:52-58)."""
    sig: float = 1.0
    y: Optional[Any] = None
    params: Optional[Any] = None


@dataclass
class SVPotential(UnivariatePotential, Potential):
    """sum_k log N(y_{t,k}; 0, exp(x_{t,k})) (examples/stochastic_volatility/auxiliary_csmc.py:39-46).
    As G0 give y = ys[0]; as Gt give params = ys[1:]."""
    y: Optional[Any] = None
    params: Optional[Any] = None


@dataclass
class Lorenz63Dynamics(Dynamics, Potential):
    """Euler-Maruyama step of the stochastic Lorenz-63 system, examples/lorenz/model.py:10-25:
    x_{t+1} | x_t ~ N(x_t + dt (phi_0(x_t) + theta * phi(x_t)), dt sigma_x^2 I),
    phi_0 = (0, -x2 - x1 x3, x1 x2), phi = (x2 - x1, x1, -x3), theta = (sigma, rho, beta)."""
    theta: Any
    sigma_x: float
    dt: float
    params: Optional[Any] = None

    def chol(self):
        return float(self.sigma_x) * np.sqrt(float(self.dt)) * np.eye(3)

    def mean(self, x):
        x = np.asarray(x)
        th = np.asarray(self.theta, np.float64)
        x1, x2, x3 = x[..., 0], x[..., 1], x[..., 2]
        f = np.stack([th[0] * (x2 - x1), th[1] * x1 - x2 - x1 * x3, x1 * x2 - th[2] * x3], axis=-1)
        return x + self.dt * f


@dataclass
class MaskedGaussianObsPotential(UnivariatePotential, Potential):
    """sum over the FINITE components of y_t of log N(y_{t,k}; x_{t,k}, sig^2): state components observed directly, missing
    components / whole missing steps carry NaN (examples/lorenz/model.py:43-56 observes x2, x3 every 80th step).
    As G0 give y = ys[0]; as Gt give params = ys[1:]."""
    sig: float = 1.0
    y: Optional[Any] = None
    params: Optional[Any] = None


@dataclass
class MultivariateTPotential(UnivariatePotential, Potential):
    """The unnormalised multivariate Student-t log-density with a precision matrix (examples/spatial/t_distribution.py:98-104, model.py:121-124):
        log g_t(x) = -(nu + d) / 2 log(1 + (x - y_t)^T prec (x - y_t) / nu),   the whole value 0 when it is NaN
    (a NaN anywhere in y_t makes the step flat).  The one potential of the closed family that couples the components of a state.
    As G0 give y = ys[0]; as Gt give params = ys[1:]; both carry the same nu and prec.  Validated here, without a GPU: nu > 0, prec square,
    symmetric to 1e-12 relative, positive definite, of y's dimension -- anything else raises ValueError."""
    nu: float = 1.0
    prec: Any = None
    y: Optional[Any] = None
    params: Optional[Any] = None

    def __post_init__(self):
        if not (np.ndim(self.nu) == 0 and float(self.nu) > 0 and np.isfinite(float(self.nu))):
            raise ValueError(f"MultivariateTPotential: nu must be a finite scalar > 0 (got {self.nu!r})")
        if self.prec is None:
            raise ValueError("MultivariateTPotential: prec (the precision matrix) is required")
        P = np.atleast_2d(np.asarray(self.prec, np.float64))
        if P.ndim != 2 or P.shape[0] != P.shape[1]:
            raise ValueError(f"MultivariateTPotential: prec must be a square matrix (got shape {np.shape(self.prec)})")
        if not np.all(np.isfinite(P)) or np.max(np.abs(P - P.T)) > 1e-12 * np.max(np.abs(P)):
            raise ValueError("MultivariateTPotential: prec must be finite and symmetric (to 1e-12 relative)")
        try:
            np.linalg.cholesky(P)
        except np.linalg.LinAlgError:
            raise ValueError("MultivariateTPotential: prec must be positive definite") from None
        d = P.shape[0]
        if self.y is not None and np.size(self.y) != d:
            raise ValueError(f"MultivariateTPotential: y has shape {np.shape(self.y)}, prec is {d} x {d}")
        if self.params is not None and (np.shape(self.params)[-1] if np.ndim(self.params) >= 2 else (d if d == 1 else -1)) != d:
            raise ValueError(f"MultivariateTPotential: params has shape {np.shape(self.params)}, expected (T - 1, {d})")
        self.nu, self.prec = float(self.nu), 0.5 * (P + P.T)

    @property
    def dx(self):
        return self.prec.shape[0]

    def __call__(self, x, y):
        """the NumPy formula (batched over the leading axes of x), with the reference's NaN rule"""
        r = np.asarray(x, np.float64) - np.asarray(y, np.float64)
        with np.errstate(invalid="ignore"):
            q = np.einsum("...i,ij,...j->...", r, self.prec, r)
            v = -0.5 * (self.nu + self.dx) * np.log1p(q / self.nu)
        return np.where(np.isnan(v), 0.0, v)


@dataclass
class LinearGaussianPotential(UnivariatePotential, Potential):
    """The linear-Gaussian observation y_t ~ N(H x_t + c, R):
        log g_t(x) = log N(y_t; H x + c, R),   the whole value 0 when it is NaN
    (a NaN anywhere in y_t makes the step flat: a step is observed whole or not at all).  H is (dy, dx) with 1 <= dy <= dx <= 32, R (dy, dy) symmetric
    positive definite, c (dy,) with default 0.  As G0 give y = ys[0]; as Gt give params = ys[1:]; both carry the same H, R and c.  Validated here, without a
    GPU: shapes, finiteness, R symmetric to 1e-12 relative and positive definite -- anything else raises ValueError; dy > dx raises NotImplementedError.
    The device evaluates the whitened residual form c_lin - |yw_t - Hw x|^2 / 2 (whitened(): Hw = L^-1 H, yw = L^-1 (y - c), L = chol R, formed once in float64)."""
    H: Any = None
    R: Any = None
    c: Optional[Any] = None
    y: Optional[Any] = None
    params: Optional[Any] = None

    def __post_init__(self):
        name = "LinearGaussianPotential"
        if self.H is None or self.R is None:
            raise ValueError(f"{name}: H (the observation matrix) and R (the observation covariance) are required")
        H = np.asarray(self.H, np.float64)
        if H.ndim != 2 or H.shape[0] < 1 or H.shape[1] < 1:
            raise ValueError(f"{name}: H must be a (dy, dx) matrix (got shape {np.shape(self.H)})")
        dy, dx = H.shape
        if dx > 32:
            raise ValueError(f"{name}: dx = {dx}: the cSMC kernels cover dx <= 32")
        if dy > dx:
            raise NotImplementedError(f"{name}: dy = {dy} > dx = {dx}: the potential covers 1 <= dy <= dx (more observations than state components "
                                      "would need a reduction to dx sufficient statistics per step, which is not done)")
        Rm = np.asarray(self.R, np.float64)
        if Rm.ndim == 0 and dy == 1:
            Rm = Rm.reshape(1, 1)
        if Rm.shape != (dy, dy):
            raise ValueError(f"{name}: R must be ({dy}, {dy}) for H of shape {H.shape} (got shape {np.shape(self.R)})")
        if not np.all(np.isfinite(H)):
            raise ValueError(f"{name}: H must be finite")
        if not np.all(np.isfinite(Rm)) or np.max(np.abs(Rm - Rm.T)) > 1e-12 * np.max(np.abs(Rm)):
            raise ValueError(f"{name}: R must be finite and symmetric (to 1e-12 relative)")
        Rm = 0.5 * (Rm + Rm.T)
        try:
            np.linalg.cholesky(Rm)
        except np.linalg.LinAlgError:
            raise ValueError(f"{name}: R must be positive definite") from None
        c = np.zeros(dy) if self.c is None else np.asarray(self.c, np.float64)
        if c.shape != (dy,) or not np.all(np.isfinite(c)):
            raise ValueError(f"{name}: c must be a finite vector of shape ({dy},) (got shape {np.shape(self.c)})")
        if self.y is not None and np.size(self.y) != dy:
            raise ValueError(f"{name}: y has shape {np.shape(self.y)}, H has {dy} rows")
        if self.params is not None and (np.shape(self.params)[-1] if np.ndim(self.params) >= 2 else (dy if dy == 1 else -1)) != dy:
            raise ValueError(f"{name}: params has shape {np.shape(self.params)}, expected (T - 1, {dy})")
        self.H, self.R, self.c = H, Rm, c

    @property
    def dx(self):
        return self.H.shape[1]

    @property
    def dy(self):
        return self.H.shape[0]

    def whitened(self, ys):
        """(Hw zero-padded to (dx, dx), yw zero-padded to (T, dx), c_lin) of the observations ys (T, dy): L = chol R, Hw = L^-1 H, yw_t = L^-1 (y_t - c),
        c_lin = -sum_k log L_kk - (dy / 2) log 2 pi; a row of ys with any NaN becomes an all-NaN row of yw.  float64."""
        dy, dx = self.H.shape
        ys = np.asarray(ys, np.float64).reshape(-1, dy)
        L = np.linalg.cholesky(self.R)
        Hw = np.zeros((dx, dx))
        Hw[:dy] = np.linalg.solve(L, self.H)
        yw = np.zeros((ys.shape[0], dx))
        miss = np.isnan(ys).any(axis=1)
        yw[:, :dy] = np.linalg.solve(L, (np.where(miss[:, None], 0.0, ys) - self.c).T).T
        yw[miss] = np.nan
        c_lin = -float(np.sum(np.log(np.diag(L)))) - 0.5 * dy * float(np.log(2.0 * np.pi))
        return Hw, yw, c_lin

    def __call__(self, x, y):
        """the NumPy formula (batched over the leading axes of x): solve + slogdet on the unwhitened residual, NaN -> 0"""
        x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
        with np.errstate(invalid="ignore"):
            r = y - (x @ self.H.T + self.c)
            q = np.sum(r * np.linalg.solve(self.R, r[..., None])[..., 0], axis=-1)
            v = -0.5 * q - 0.5 * np.linalg.slogdet(self.R)[1] - 0.5 * self.dy * np.log(2.0 * np.pi)
        return np.where(np.isnan(v), 0.0, v)


@dataclass
class PoissonPotential(UnivariatePotential, Potential):
    """Counts with a log link, y_{t,k} ~ Poisson(exp(x_{t,k})), independent over the components (AUXSSM_POT_POISSON):
        log g_t(x) = sum_k [ y_{t,k} x_k - exp(x_k) ]   over the components whose y_{t,k} is finite
    -- a NaN y_{t,k} drops component k of step t (per component, as SVPotential; not the whole-step rule of the coupled potentials).  Unnormalised: the
    constant -sum_k log y_{t,k}! is left out (it does not depend on x and cancels in every normalisation of the weights).  Non-integer values >= 0 are accepted,
    the formula is the same; a finite negative entry raises ValueError at construction.  An offset (a log-exposure o_{t,k}: y ~ Poisson(exp(o + x))) needs no
    field: it is a shift of the state, z = x + o, through m0 and b.  As G0 give y = ys[0]; as Gt give params = ys[1:].
    The auxiliary Kalman sampler's twin is kalman.PoissonModel: same density, same conventions (constant, missing counts, validation)."""
    y: Optional[Any] = None
    params: Optional[Any] = None

    @staticmethod
    def check_counts(a):
        a = np.asarray(a, np.float64)
        if np.any(a[np.isfinite(a)] < 0):
            raise ValueError(f"PoissonPotential: counts must be >= 0 or NaN (missing); got a minimum of {float(np.nanmin(a))}")

    def __post_init__(self):
        for a in (self.y, self.params):
            if a is not None:
                self.check_counts(a)

    def __call__(self, x, y):
        """the NumPy formula (batched over the leading axes of x); a non-finite y_k drops its component"""
        x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            v = y * x - np.exp(x)
        return np.sum(np.where(np.isfinite(y), v, 0.0), axis=-1)


class _LogisticPotential(UnivariatePotential, Potential):
    """What BinomialPotential and NegBinomialPotential share (AUXSSM_POT_LOGISTIC): one potential with a logit link and a SIZE m beside every observation,
        log g_t(x) = sum_k [ y_{t,k} x_k - m_{t,k} softplus(x_k) ]   over the components whose y_{t,k} is finite
    -- a NaN y_{t,k} drops component k of step t whatever its size is.  A subclass names its parameter (trials / r), whose (n, dx) form `sizes(ys)` validates
    against the data and turns into m (the data rules are the Kalman models', _logistic.py).  As G0 give y = ys[0] with a scalar or (dx,) parameter; as Gt give
    params = ys[1:] with a scalar, (dx,) or (T - 1, dx) parameter."""

    def _data(self):
        """the observations this object holds as (n, dx): y as one row, or params"""
        a = self.y if self.y is not None else self.params
        return None if a is None else np.atleast_2d(np.asarray(a, np.float64))

    def __post_init__(self):
        if self._data() is not None:
            self.sizes()

    def __call__(self, x, y, size=None):
        """the NumPy formula (batched over the leading axes of x); a non-finite y_k drops its component.  size: the sizes m beside y (same shape); by default
        those this object's parameter gives for y -- a scalar or (dx,) parameter, or y = all the rows this object holds"""
        if size is None:
            y2 = np.atleast_2d(np.asarray(y, np.float64))
            size = np.reshape(self._size_of(y2, self._parameter()), np.shape(y))
        return _logistic.log_g(x, y, size)

    def sizes(self):
        """the sizes m (n, dx) of the held observations, validated; 0 where the observation is missing"""
        ys = self._data()
        m = self._size_of(ys, self._parameter())
        return np.where(np.isfinite(ys), m, 0.0)


@dataclass
class BinomialPotential(_LogisticPotential):
    """Binomial data with a logit link, y_{t,k} ~ Binomial(trials_{t,k}, sigma(x_{t,k})), independent over the components (AUXSSM_POT_LOGISTIC with m = trials):
        log g_t(x) = sum_k [ y_{t,k} x_k - trials_{t,k} softplus(x_k) ]   over the components whose y_{t,k} is finite
    Binary data is trials = 1.  Unnormalised: the constant log C(trials, y) is left out; non-integers are accepted; a NaN y_{t,k} is a missing observation
    (its trials may be anything).  A finite y outside [0, trials], trials <= 0 or a non-finite trials under a finite y raises ValueError (kalman.BinomialModel's
    rules).  As G0: BinomialPotential(trials, y=ys[0]); as Gt: BinomialPotential(trials, params=ys[1:]), trials a scalar, (dx,) or (T - 1, dx)."""
    trials: Any = 1.0
    y: Optional[Any] = None
    params: Optional[Any] = None

    def _parameter(self):
        return self.trials

    @staticmethod
    def _size_of(ys, trials):
        return _logistic.binomial_size(ys, trials, "BinomialPotential")


@dataclass
class NegBinomialPotential(_LogisticPotential):
    """Overdispersed counts y_{t,k} ~ NB(r_{t,k}, p = sigma(x_{t,k})) (pmf proportional to p^y (1 - p)^r: mean r e^x), independent over the components
    (AUXSSM_POT_LOGISTIC with m = y + r):
        log g_t(x) = sum_k [ y_{t,k} x_k - (y_{t,k} + r_{t,k}) softplus(x_k) ]   over the components whose y_{t,k} is finite
    Unnormalised; non-integer counts are accepted; a NaN y_{t,k} is a missing observation.  A finite negative count, r <= 0 or a non-finite r under a finite y
    raises ValueError (kalman.NegBinomialModel's rules).  As G0: NegBinomialPotential(r, y=ys[0]); as Gt: NegBinomialPotential(r, params=ys[1:]), r a scalar,
    (dx,) or (T - 1, dx)."""
    r: Any = 1.0
    y: Optional[Any] = None
    params: Optional[Any] = None

    def _parameter(self):
        return self.r

    @staticmethod
    def _size_of(ys, r):
        return ys + _logistic.negbinomial_r(ys, r, "NegBinomialPotential")


# ---- user-defined models: device code compiled when the kernel is built (csrc/fk_program.hip, include/auxssm.h auxssm_fk_program_compile) ----------
@dataclass
class DevicePotential(UnivariatePotential, Potential):
    """A potential written as HIP device code, compiled into the sequential cSMC kernels at get_kernel time.  `source` defines
        template <typename R, int D> __device__ R log_g(int t, const R* x, const R* xprev, const R* y, const R* theta);
    and optionally  template <typename R, int D> __device__ R log_g_bound(int t, const R* y, const R* theta)  (sup_x log G_t, or +inf).
    t = the time index of x (0 for G0); xprev = x_{t-1} (nullptr at t = 0); y = row t of the (T, p) observations (nullptr without); theta = `theta`.
    As G0 give y = ys[0]; as Gt give params = ys[1:], like the built-in potentials; G0 and Gt carry the same source and theta.  p: the number of
    observation columns (default: inferred from y / params).  The code may call fma_, det_exp, det_log and the device math library (exp, log, lgamma, ...).
    Gradient-informed proposals (get_independent_kernel(..., gradient=True / "exact")) also need its partial derivatives:
        template <typename R, int D> __device__ void grad_log_g(int t, const R* x, const R* xprev, const R* y, const R* theta, R* gx, R* gxprev);
    gx (D) w.r.t. x, gxprev (D) w.r.t. xprev (nullptr at t = 0), both zero-filled by the caller."""
    source: str = ""
    y: Optional[Any] = None
    params: Optional[Any] = None
    theta: Optional[Any] = None
    p: Optional[int] = None


@dataclass
class DeviceGaussianDynamics(Dynamics, Potential):
    """x_t | x_{t-1} ~ N(mean(x_{t-1}), Q) with the mean written as HIP device code (compiled at get_kernel time):
        template <typename R, int D> __device__ void mean(int t, const R* xprev, const R* theta, R* mu);
    t = the time index of x_t.  Q (d, d) is time-invariant; the backward pass evaluates N(x_{t+1}; mean(x_t), Q) through the same code.
    Gradient-informed proposals also need the vector-Jacobian product of the mean, out = J^T v with J = d mean(t, xprev) / d xprev:
        template <typename R, int D> __device__ void mean_vjp(int t, const R* xprev, const R* theta, const R* v, R* out);"""
    source: str = ""
    Q: Any = None
    theta: Optional[Any] = None
    params: Optional[Any] = None

    def chol(self):
        return np.linalg.cholesky(np.atleast_2d(np.asarray(self.Q, np.float64)))
