"""Multi-dimensional user-defined Feynman-Kac models for the program path of the sequential cSMC sweep (helper module, not a test file).

Each model is a triple: HIP device source (log_g / log_g_bound / grad_log_g, mean / mean_vjp), the device-side model objects built from it, and the same model
written independently in NumPy for oracle/csmc_np.py's generic protocol (the "literal").  The sources deliberately differ from the built-in potentials' operation
order: they are compared with the literal to a tolerance, never bit for bit.

    RANGE                range observations of a planar position from p sensors (p read from theta[0]; NaN = sensor missing), dx = 2 (position, damped random walk)
                         or dx = 4 (position + velocity, constant-velocity mean), full Q; the mean once as built-in LinearGaussianDynamics, once as user source
    LORENZ_USER          the Euler-Maruyama Lorenz-63 step as a user mean + a user masked-Gaussian potential; also with either part built-in (three descriptions)
    INCREMENT_NONLINEAR  device_models.INCREMENT_OBS_GRAD (a potential of (x_t, x_{t-1})) on a nonlinear user mean with a non-symmetric Jacobian, dx = 2, full Q
    GROWTH_ND            the growth model componentwise at dx = 4 with a coupling term, one observation y ~ N(sum_k x_k^2 / 20, sig^2)

The sources use nothing of the device but its math library (no fma_, det_exp or det_log, which device_models.py's built-in-order sources are there to cover):
tests/test_user_model_literals.py compiles the very same text with the host's g++ (as tests/hostsim does for its checkers) to evaluate it on the CPU.

CASES is the one list of sweeps that tests/test_gpu_user_model_multidim.py compares with the literal and whose inputs tests/test_user_model_literals.py checks on the
CPU (derivatives, well-posedness of the exact ancestor comparison, underflow of the tightened inputs)."""
import dataclasses
import functools

import numpy as np

from oracle import csmc_np as L
from aux_ssm_samplers_amd.csmc import device_models as U
from tests import potential_np
from tests.test_gpu_user_model import _MeanDyn

HALF_LOG_2PI = 0.91893853320467274178

# ---- device sources -----------------------------------------------------------------------------------------------------------------------------------
# theta = [p, sig, s_1x, s_1y, ..., s_px, s_py]; y_j ~ N(|pos - s_j|, sig^2), pos = (x[0], x[1]); a NaN y_j is a missing sensor
_RANGE_LOG_G = r"""
template <typename R, int D> __device__ R log_g(int t, const R* x, const R* xprev, const R* y, const R* theta) {
    const int p = (int)theta[0];
    const R sig = theta[1];
    R acc = 0;
    for (int j = 0; j < p; ++j) {
        const R v = y[j];
        if (v == v) {
            const R a = x[0] - theta[2 + 2 * j], b = x[1] - theta[3 + 2 * j];
            const R z = (v - sqrt(a * a + b * b)) / sig;
            acc += (R)-0.5 * (z * z) - log(sig) - (R)0.91893853320467274178;
        }
    }
    return acc;
}
template <typename R, int D> __device__ void grad_log_g(int t, const R* x, const R* xprev, const R* y, const R* theta, R* gx, R* gxprev) {
    const int p = (int)theta[0];
    const R sig = theta[1];
    for (int j = 0; j < p; ++j) {
        const R v = y[j];
        if (v == v) {
            const R a = x[0] - theta[2 + 2 * j], b = x[1] - theta[3 + 2 * j];
            const R r = sqrt(a * a + b * b);
            const R z = (v - r) / sig;
            gx[0] += z / sig * (a / r);
            gx[1] += z / sig * (b / r);
        }
    }
}
"""
_RANGE_BOUND = r"""
template <typename R, int D> __device__ R log_g_bound(int t, const R* y, const R* theta) {
    const int p = (int)theta[0];
    int n = 0;
    for (int j = 0; j < p; ++j) n += (y[j] == y[j]) ? 1 : 0;
    return -(R)n * (log(theta[1]) + (R)0.91893853320467274178)%s;
}
"""
# theta = [dt, a]; D = 4: (pos + dt vel, a vel); D = 2: a pos
RANGE_CV_MEAN = r"""
template <typename R, int D> __device__ void mean(int t, const R* xprev, const R* theta, R* mu) {
    if constexpr (D == 4) {
        mu[0] = xprev[0] + theta[0] * xprev[2];
        mu[1] = xprev[1] + theta[0] * xprev[3];
        mu[2] = theta[1] * xprev[2];
        mu[3] = theta[1] * xprev[3];
    } else {
        for (int k = 0; k < D; ++k) mu[k] = theta[1] * xprev[k];
    }
}
template <typename R, int D> __device__ void mean_vjp(int t, const R* xprev, const R* theta, const R* v, R* out) {
    if constexpr (D == 4) {
        out[0] = v[0];
        out[1] = v[1];
        out[2] = theta[0] * v[0] + theta[1] * v[2];
        out[3] = theta[0] * v[1] + theta[1] * v[3];
    } else {
        for (int k = 0; k < D; ++k) out[k] = theta[1] * v[k];
    }
}
"""

# theta = [sig]; y_k ~ N(x_k, sig^2) for the finite y_k (p = D)
MASKED_OBS = r"""
template <typename R, int D> __device__ R log_g(int t, const R* x, const R* xprev, const R* y, const R* theta) {
    const R sig = theta[0];
    R acc = 0;
    for (int k = 0; k < D; ++k) {
        const R z = (y[k] - x[k]) / sig;
        const R v = (R)-0.5 * (z * z) - log(sig) - (R)0.91893853320467274178;
        acc += (v == v) ? v : (R)0;
    }
    return acc;
}
template <typename R, int D> __device__ void grad_log_g(int t, const R* x, const R* xprev, const R* y, const R* theta, R* gx, R* gxprev) {
    const R sig = theta[0];
    for (int k = 0; k < D; ++k) {
        const R g = (y[k] - x[k]) / (sig * sig);
        gx[k] = (g == g) ? g : (R)0;
    }
}
template <typename R, int D> __device__ R log_g_bound(int t, const R* y, const R* theta) {
    int n = 0;
    for (int k = 0; k < D; ++k) n += (y[k] == y[k]) ? 1 : 0;
    return -(R)n * (log(theta[0]) + (R)0.91893853320467274178);
}
"""
# theta = [sigma, rho, beta, dt]: x + dt f(x), f = (sigma (x2 - x1), rho x1 - x2 - x1 x3, x1 x2 - beta x3); J = I + dt Df
LORENZ_MEAN = r"""
template <typename R, int D> __device__ void mean(int t, const R* xprev, const R* theta, R* mu) {
    const R a = xprev[0], b = xprev[1], c = xprev[2], dt = theta[3];
    mu[0] = a + dt * (theta[0] * (b - a));
    mu[1] = b + dt * (theta[1] * a - b - a * c);
    mu[2] = c + dt * (a * b - theta[2] * c);
}
template <typename R, int D> __device__ void mean_vjp(int t, const R* xprev, const R* theta, const R* v, R* out) {
    const R a = xprev[0], b = xprev[1], c = xprev[2], dt = theta[3];
    out[0] = v[0] + dt * (-theta[0] * v[0] + (theta[1] - c) * v[1] + b * v[2]);
    out[1] = v[1] + dt * (theta[0] * v[0] - v[1] + a * v[2]);
    out[2] = v[2] + dt * (-a * v[1] - theta[2] * v[2]);
}
"""

# theta = [a, c]: mu = (a x0 + c sin x1, a x1 + c x0 x1 / (1 + x0^2))
NONLINEAR_MEAN_2D = r"""
template <typename R, int D> __device__ void mean(int t, const R* xprev, const R* theta, R* mu) {
    const R a = theta[0], c = theta[1], u = xprev[0], w = xprev[1];
    mu[0] = a * u + c * sin(w);
    mu[1] = a * w + c * u * w / ((R)1 + u * u);
}
template <typename R, int D> __device__ void mean_vjp(int t, const R* xprev, const R* theta, const R* v, R* out) {
    const R a = theta[0], c = theta[1], u = xprev[0], w = xprev[1], q = (R)1 + u * u;
    out[0] = a * v[0] + c * w * ((R)1 - u * u) / (q * q) * v[1];
    out[1] = c * cos(w) * v[0] + (a + c * u / q) * v[1];
}
"""

# theta_g = [sig]: y ~ N(sum_k x_k^2 / 20, sig^2) (p = 1);  theta_m = [kappa]: mu_k = x_k / 2 + 25 x_k / (1 + x_k^2) + 8 cos(1.2 t) + kappa x_{k+1 mod D}
_GROWTH_ND = r"""
template <typename R, int D> __device__ R log_g(int t, const R* x, const R* xprev, const R* y, const R* theta) {
    R s = 0;
    for (int k = 0; k < D; ++k) s += x[k] * x[k];
    const R z = (y[0] - s / (R)20) / theta[0];
    return (R)-0.5 * (z * z) - log(theta[0]) - (R)0.91893853320467274178;
}
template <typename R, int D> __device__ void grad_log_g(int t, const R* x, const R* xprev, const R* y, const R* theta, R* gx, R* gxprev) {
    R s = 0;
    for (int k = 0; k < D; ++k) s += x[k] * x[k];
    const R z = (y[0] - s / (R)20) / theta[0];
    for (int k = 0; k < D; ++k) gx[k] = z * x[k] / ((R)10 * theta[0]);
}
template <typename R, int D> __device__ void mean(int t, const R* xprev, const R* theta, R* mu) {
    for (int k = 0; k < D; ++k) {
        const R v = xprev[k];
        mu[k] = v / (R)2 + (R)25 * v / ((R)1 + v * v) + (R)8 * cos((R)1.2 * (R)t) + theta[0] * xprev[(k + 1) % D];
    }
}
template <typename R, int D> __device__ void mean_vjp(int t, const R* xprev, const R* theta, const R* v, R* out) {
    for (int k = 0; k < D; ++k) {
        const R a = xprev[k], q = (R)1 + a * a;
        out[k] = ((R)0.5 + (R)25 * ((R)1 - a * a) / (q * q)) * v[k] + theta[0] * v[(k + D - 1) % D];
    }
}
"""
_GROWTH_BOUND = r"""
template <typename R, int D> __device__ R log_g_bound(int t, const R* y, const R* theta) {
    return -log(theta[0]) - (R)0.91893853320467274178%s;
}
"""
_INF_BOUND = r"""
template <typename R, int D> __device__ R log_g_bound(int t, const R* y, const R* theta) { return (R)INFINITY; }
"""

BOUNDS = ("exact", "loose", "inf", "none")  # the exact supremum, the supremum + 50, +inf, no log_g_bound in the source


def _with_bound(body, bound_tpl, bound):
    if bound == "none":
        return body
    if bound == "inf":
        return body + _INF_BOUND
    return body + bound_tpl % ("" if bound == "exact" else " + (R)50")


def range_source(bound="exact"):
    return _with_bound(_RANGE_LOG_G, _RANGE_BOUND, bound)


def growth_nd_source(bound="exact"):
    return _with_bound(_GROWTH_ND, _GROWTH_BOUND, bound)


RANGE = range_source()
GROWTH_ND = growth_nd_source()

# ---- literal (NumPy) model parts: written from the model definitions, not from the device sources ---------------------------------------------------------
class _YPot:
    """G_t(x_t, x_{t-1}) = g(x_t, x_{t-1}, y_t); params = y[1:] (G0: g(x_0, None, y_0))"""

    def __init__(self, g, y, first=False):
        self.g, self.y, self.first = g, y, first
        self.params = None if first else y[1:]

    def __call__(self, x, x_prev=None, params=None):
        return self.g(x, None, self.y[0]) if self.first else self.g(x, x_prev, params)


def range_log_g(S, sig):
    """sum over the sensors with a finite reading of log N(y_j; |pos - s_j|, sig^2); S (p, 2)"""
    def g(x, xprev, y):
        r = np.sqrt(np.sum((x[..., None, :2] - S) ** 2, axis=-1))
        z = (y - r) / sig
        return np.nansum(-0.5 * z * z - np.log(sig) - x.dtype.type(HALF_LOG_2PI), axis=-1).astype(x.dtype)
    return g


def increments_log_g(s):
    def g(x, xprev, y):
        z = (y - (x if xprev is None else x - xprev)) / s
        return np.sum(-0.5 * z * z - np.log(s) - x.dtype.type(HALF_LOG_2PI), axis=-1).astype(x.dtype)
    return g


def growth_nd_log_g(sig):
    def g(x, xprev, y):
        z = (y[0] - np.sum(x * x, axis=-1) / 20) / sig
        return (-0.5 * z * z - np.log(sig) - x.dtype.type(HALF_LOG_2PI)).astype(x.dtype)
    return g


def nonlinear_mean_2d(a, c):
    def mean(x, t):
        u, w = x[..., 0], x[..., 1]
        return np.stack([a * u + c * np.sin(w), a * w + c * u * w / (1 + u * u)], axis=-1)
    return mean


def growth_nd_mean(kappa):
    def mean(x, t):
        R = x.dtype.type   # (the forcing term in the precision of x as well: an fp32 evaluation of the literal is fp32 throughout)
        return x / 2 + 25 * x / (1 + x * x) + 8 * np.cos(R(1.2) * R(t)) + kappa * np.roll(x, -1, axis=-1)
    return mean


# ---- the models ---------------------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Spec:
    """one model instance: which model, its shape and variant, the length and the seed of its simulated data"""
    model: str                 # "range" | "lorenz" | "increments" | "growth_nd"
    dx: int = 2
    p: int = 1
    parts: str = "user"        # range: the mean as "user" source or "builtin" LinearGaussianDynamics; lorenz: "user" | "potential" (user potential on the
    #                            built-in Lorenz63Dynamics) | "mean" (user mean under the built-in masked potential) | "builtin" (no program at all)
    bound: str = "exact"       # one of BOUNDS (range, growth_nd)
    tight: bool = False        # the tightened observation noise whose shifted weights underflow (range, growth_nd)
    T: int = 24
    seed: int = 0

    @property
    def name(self):
        s = f"{self.model}-d{self.dx}-p{self.p}-{self.parts}"
        return s + ("" if self.bound == "exact" else f"-{self.bound}") + ("-tight" if self.tight else "")

    def data_key(self):
        """the fields that decide the literal model and its data (the device description and the bound variant do not)"""
        return (self.model, self.dx, self.p, self.tight, self.T, self.seed)


_SENSORS = np.array([[4.0, 0.5], [-3.0, 2.5], [0.5, -5.0], [6.0, 6.0], [-5.5, -4.0], [1.5, 7.0]])
_LORENZ_THETA, _LORENZ_DT, _LORENZ_SIGX, _LORENZ_SIGY, _LORENZ_EVERY = (10.0, 28.0, 8.0 / 3.0), 0.02, 1.0, 0.5, 4


def _sim(mean, LQ, x_init, T, rng):
    x = np.zeros((T, x_init.shape[0]))
    x[0] = x_init
    for t in range(1, T):
        x[t] = mean(x[t - 1], t) + LQ @ rng.standard_normal(x_init.shape[0])
    return x


@functools.lru_cache(maxsize=None)
def _data(key):
    """the simulated trajectory, observations and parameters of a model instance (fp64, a function of Spec.data_key() only)"""
    model, dx, p, tight, T, seed = key
    rng = np.random.default_rng([seed, dx, p, T, len(model)])
    d = dict(T=T)
    if model == "range":
        dt, a = 0.5, 0.9
        F = a * np.eye(2) if dx == 2 else np.block([[np.eye(2), dt * np.eye(2)], [np.zeros((2, 2)), a * np.eye(2)]])
        A = 0.3 * np.eye(dx) + 0.1 * np.tril(np.ones((dx, dx)))
        Q = A @ A.T                                            # full
        sig = 0.02 if tight else 1.0
        x = _sim(lambda v, t: F @ v, np.linalg.cholesky(Q), np.concatenate([[1.0, -1.0], 0.3 * np.ones(dx - 2)]), T, rng)
        S = _SENSORS[:p]
        y = np.sqrt(np.sum((x[:, None, :2] - S) ** 2, axis=-1)) + sig * rng.standard_normal((T, p))
        if T > 4:
            y[rng.integers(1, T - 1, size=max(T // 6, 1)), rng.integers(0, p, size=max(T // 6, 1))] = np.nan   # single sensors missing
        d.update(F=F, Q=Q, sig=sig, S=S, dt=dt, a=a, x=x, y=y, m0=np.concatenate([[1.0, -1.0], np.zeros(dx - 2)]), P0=np.eye(dx))
    elif model == "lorenz":
        th, dt = np.array(_LORENZ_THETA), _LORENZ_DT
        LQ = _LORENZ_SIGX * np.sqrt(dt) * np.eye(3)
        mean = lambda v, t: v + dt * np.array([th[0] * (v[1] - v[0]), th[1] * v[0] - v[1] - v[0] * v[2], v[0] * v[1] - th[2] * v[2]])
        x = _sim(mean, LQ, np.array([1.5, -1.5, 25.0]), T, rng)
        y = x + _LORENZ_SIGY * rng.standard_normal((T, 3))
        keep = np.arange(T) % _LORENZ_EVERY == 0
        y[~keep, 1:] = np.nan                                  # x2, x3 every 4th step
        if T > 6:
            y[5] = np.nan                                      # one step without any observation
        d.update(theta=th, dt=dt, LQ=LQ, sig=_LORENZ_SIGY, x=x, y=y, m0=np.array([1.5, -1.5, 25.0]), P0=np.eye(3))
    elif model == "increments":
        a, c, s = 0.8, 0.7, 1.0
        Q = np.array([[0.5, 0.2], [0.2, 0.4]])
        x = _sim(nonlinear_mean_2d(a, c), np.linalg.cholesky(Q), rng.standard_normal(2), T, rng)
        y = np.diff(x, axis=0, prepend=0.0) + s * rng.standard_normal((T, 2))
        d.update(a=a, c=c, s=s, Q=Q, x=x, y=y, m0=np.zeros(2), P0=np.eye(2))
    elif model == "growth_nd":
        kappa, sig = 0.1, (0.02 if tight else 2.0)
        Q = np.eye(4)
        x = _sim(growth_nd_mean(kappa), np.linalg.cholesky(Q), rng.standard_normal(4), T, rng)
        y = np.sum(x * x, axis=-1, keepdims=True) / 20 + sig * rng.standard_normal((T, 1))
        d.update(kappa=kappa, sig=sig, Q=Q, x=x, y=y, m0=np.zeros(4), P0=np.eye(4))
    else:
        raise ValueError(model)
    return d


def data(spec):
    return _data(spec.data_key())


def literal(spec, dtype=np.float64):
    """(M0, G0, Mt, Gt) for oracle/csmc_np.py, every parameter in `dtype`"""
    d, T, R = data(spec), spec.T, np.dtype(dtype).type
    A = lambda a: np.asarray(a, dtype)
    y = A(d["y"])
    M0 = L.GaussianInit(A(d["m0"]), A(np.linalg.cholesky(d["P0"])))
    if spec.model == "range":
        g = range_log_g(A(d["S"]), R(d["sig"]))
        return M0, _YPot(g, y, True), L.LinearGaussianDynamics(A(d["F"]), A(np.zeros(spec.dx)), A(np.linalg.cholesky(d["Q"])), T), _YPot(g, y)
    if spec.model == "lorenz":
        return (M0, L.ObsPotential("masked", y[0], d["sig"], first=True), L.Lorenz63EM(A(d["theta"]), d["dt"], A(d["LQ"]), T),
                L.ObsPotential("masked", y[1:], d["sig"]))
    if spec.model == "increments":
        g = increments_log_g(R(d["s"]))
        return M0, _YPot(g, y, True), _MeanDyn(nonlinear_mean_2d(R(d["a"]), R(d["c"])), A(np.linalg.cholesky(d["Q"])), T), _YPot(g, y)
    g = growth_nd_log_g(R(d["sig"]))
    return M0, _YPot(g, y, True), _MeanDyn(growth_nd_mean(R(d["kappa"])), A(np.linalg.cholesky(d["Q"])), T), _YPot(g, y)


def device(spec, infer_p=False):
    """(M0, G0, Mt, Gt) of aux_ssm_samplers_amd.csmc; infer_p: leave DevicePotential.p to be inferred from the shapes of y / params"""
    from aux_ssm_samplers_amd.csmc import (GaussianInit, LinearGaussianDynamics, Lorenz63Dynamics, MaskedGaussianObsPotential, DevicePotential,
                                           DeviceGaussianDynamics)
    d = data(spec)
    y = d["y"]
    M0 = GaussianInit(m0=d["m0"], P0=d["P0"])
    pk = {} if infer_p else dict(p=y.shape[1])

    def pots(src, theta):
        return DevicePotential(src, y=y[0], theta=theta, **pk), DevicePotential(src, params=y[1:], theta=theta, **pk)
    if spec.model == "range":
        theta = np.concatenate([[spec.p, d["sig"]], d["S"].reshape(-1)])
        src = range_source(spec.bound)
        G0, Gt = pots(src, theta)
        if spec.parts == "builtin":
            Mt = LinearGaussianDynamics(F=d["F"], b=np.zeros(spec.dx), Q=d["Q"])
        else:
            Mt = DeviceGaussianDynamics(src + RANGE_CV_MEAN, Q=d["Q"], theta=[d["dt"], d["a"]])
            G0, Gt = (dataclasses.replace(g, source=src + RANGE_CV_MEAN) for g in (G0, Gt))
        return M0, G0, Mt, Gt
    if spec.model == "lorenz":
        up, um = spec.parts in ("user", "potential"), spec.parts in ("user", "mean")
        src = (MASKED_OBS if up else "") + (LORENZ_MEAN if um else "")
        G0, Gt = pots(src, [d["sig"]]) if up else (MaskedGaussianObsPotential(sig=d["sig"], y=y[0]), MaskedGaussianObsPotential(sig=d["sig"], params=y[1:]))
        Q = d["LQ"] @ d["LQ"].T
        Mt = (DeviceGaussianDynamics(src, Q=Q, theta=np.concatenate([d["theta"], [d["dt"]]])) if um
              else Lorenz63Dynamics(theta=d["theta"], sigma_x=_LORENZ_SIGX, dt=d["dt"]))
        return M0, G0, Mt, Gt
    if spec.model == "increments":
        src = U.INCREMENT_OBS_GRAD + NONLINEAR_MEAN_2D
        G0, Gt = pots(src, [d["s"]])
        return M0, G0, DeviceGaussianDynamics(src, Q=d["Q"], theta=[d["a"], d["c"]]), Gt
    src = growth_nd_source(spec.bound)
    G0, Gt = pots(src, [d["sig"]])
    return M0, G0, DeviceGaussianDynamics(src, Q=d["Q"], theta=[d["kappa"]]), Gt


# ---- the sweeps -------------------------------------------------------------------------------------------------------------------------------------------
# step sizes delta_t of the auxiliary proposals N(u_t, delta_t / 2 I), of the order of the models' transition variances; the tightened inputs use proposals much
# narrower than their observation noise, so that all particles miss the observation by about the same many standard deviations: every shifted weight
# underflows, yet the weights stay comparable (tests/test_user_model_literals.py checks both)
_DELTA = {"range": 0.03, "lorenz": 0.003, "increments": 0.1, "growth_nd": 0.001}
_DELTA_TIGHT = 5e-7
_START = {"range": 0.1, "lorenz": 0.05, "increments": 0.1, "growth_nd": 0.1}   # the reference trajectory: the simulated one + this much noise
_START_TIGHT = 0.3


@dataclasses.dataclass(frozen=True)
class Case:
    spec: Spec
    proposal: str = "independent"       # | "bootstrap"
    backward: bool = True
    gradient: object = None             # None | True (the reference's correction) | "exact"
    N: int = 128
    seed: int = 0
    group: str = "grid"

    @property
    def key(self):
        g = {None: "", True: "-gradref", "exact": "-gradexact"}[self.gradient]
        return f"{self.spec.name}-T{self.spec.T}-N{self.N}-{self.proposal}-{'bs' if self.backward else 'trace'}{g}"

    @property
    def id(self):
        return f"{self.key}-s{self.seed}"

    def literal_key(self):
        return (self.spec.data_key(), self.proposal, self.backward, self.gradient, self.N, self.seed)


def inputs(case, C=None):
    """(x0, delta, noise dict) of a case, fp64; one chain (T, d) / (T, N, d) ..., or C chains with a leading axis"""
    sp = case.spec
    d = data(sp)
    T, dx = sp.T, sp.dx
    rng = np.random.default_rng([case.seed, case.N, T, dx, 7])
    lead = () if C is None else (C,)
    x0 = d["x"] + (_START_TIGHT if sp.tight else _START[sp.model]) * rng.standard_normal(lead + (T, dx))
    delta = (_DELTA_TIGHT if sp.tight else _DELTA[sp.model]) * (0.75 + 0.5 * rng.random(T))
    nz = dict(eps_aux=rng.standard_normal(lead + (T, dx)), eps_prop=rng.standard_normal(lead + (T, case.N, dx)), u_res=rng.random(lead + (T - 1, case.N)),
              u_bwd=rng.random(lead + (T,)))
    return x0, delta, nz


_literal_runs = {}


def literal_sweep(case, grad_h=None):
    """the literal's sweep of a case: (x, ancestors, history), cached; grad_h: the step of the literal's central differences (default: csmc_np.grad_fd's)"""
    key = (case.literal_key(), grad_h)
    if key in _literal_runs:
        return _literal_runs[key]
    lit = literal(case.spec)
    x0, delta, nz = inputs(case)
    fd = L.grad_fd
    if grad_h is not None:
        L.grad_fd = lambda fn, u: fd(fn, u, h=grad_h)
    try:
        if case.proposal == "independent":
            _, kern = L.get_independent_kernel(lit[0], lit[1], lit[2], lit[3], case.N, backward=case.backward, Pt=lit[2], gradient=case.gradient is not None,
                                               exact_gradient=case.gradient == "exact")
            out = kern(L.Noise(**nz), x0, delta)
        else:
            _, kern = L.get_kernel(lit[0], lit[1], lit[2], lit[3], case.N, backward=case.backward, Pt=lit[2])
            out = kern(L.Noise(**nz), x0)
    finally:
        L.grad_fd = fd
    _literal_runs[key] = out
    return out


def _cases():
    out = []
    ranges = [Spec("range", 2, 1, "builtin"), Spec("range", 2, 3, "user"), Spec("range", 4, 3, "builtin"), Spec("range", 4, 6, "user")]
    lorenz = [Spec("lorenz", 3, 3, parts) for parts in ("user", "potential", "mean")]
    others = [Spec("increments", 2, 2), Spec("growth_nd", 4, 1)]
    # every model x {independent, bootstrap} x {backward sampling, ancestor tracing} and x gradient in {reference, exact} x the two backward modes; the other
    # shapes and descriptions of a model (p < dx, p = dx - 1, one part built-in) run two of each four
    for sp in ranges + lorenz + others:
        full = sp in (ranges[3], lorenz[0]) + tuple(others)
        for proposal in ("independent", "bootstrap"):
            for backward in (True, False):
                if full or backward == (proposal == "independent"):
                    out.append(Case(sp, proposal, backward, None, 128, 1 + backward))
        for gradient in (True, "exact"):
            for backward in (True, False):
                if full or backward == (gradient is True):
                    out.append(Case(sp, "independent", backward, gradient, 128, 3 + backward, "gradient"))
    # particle counts: two and three particles, a ragged last wave, the 8- and 16-wave kernels (and with dx = 4, fp64, N = 1024 the > 64 KB LDS launch)
    for sp in (Spec("range", 4, 6, "user"), Spec("lorenz", 3, 3, "user")):
        for N in (2, 3, 65, 512, 1000, 1024):
            out.append(Case(sp, "independent", True, None, N, 5, "N"))
            out.append(Case(sp, "independent", True, "exact", N, 6, "N"))
    # T = 1 (no transition), T = 2 (one)
    for sp in (ranges[0], ranges[3], lorenz[0], lorenz[1], lorenz[2]) + tuple(others):
        for T in (1, 2):
            spT = dataclasses.replace(sp, T=T)
            out.append(Case(spT, "independent", True, None, 128, 7, "T"))
            out.append(Case(spT, "independent", True, "exact", 128, 8, "T"))
            out.append(Case(spT, "bootstrap", False, None, 128, 9, "T"))
    # the potential's bound: exact, loose, +inf, none; the ordinary and the tightened inputs
    for sp in (Spec("range", 4, 6, "user"), Spec("growth_nd", 4, 1)):
        for tight in (False, True):
            for bound in BOUNDS:
                spb = dataclasses.replace(sp, bound=bound, tight=tight)
                out.append(Case(spb, "independent", True, None, 256, 10, "bound"))
                if bound in ("exact", "none") and not tight:   # (the tightened inputs collapse onto one particle under the prior's proposals)
                    out.append(Case(spb, "bootstrap", False, None, 256, 11, "bound"))
    return out


def requirements(case, w):
    """what wellposedness(case) = w has to satisfy (tests/test_user_model_literals.py asserts it; the seeds of _SEEDS were searched with it)"""
    ok = w["gap"] >= 1e-8
    if case.N >= 64:
        ok = ok and w["ess"] >= 2 and w["moved"] > 0.1
    if case.spec.tight:   # (the fp64 sweeps reach the fallback too)
        ok = ok and w["underflow32"] >= 1 and w["underflow64"] >= 1
    return ok


# the noise seed of a case, where the default one (the group's) does not meet `requirements`: the first of default + 100 k that does
_SEEDS = {
    "range-d4-p3-builtin-T24-N128-bootstrap-trace": 101,
    "range-d4-p6-user-T24-N128-independent-trace": 101,
    "range-d4-p6-user-T24-N128-bootstrap-trace": 101,
    "growth_nd-d4-p1-user-T24-N128-independent-trace": 101,
    "growth_nd-d4-p1-user-T24-N128-bootstrap-trace": 101,
    "range-d4-p6-user-T24-N512-independent-bs-gradexact": 106,
    "range-d4-p6-user-T24-N1000-independent-bs-gradexact": 206,
    "range-d4-p6-user-T24-N1024-independent-bs": 105,
    "lorenz-d3-p3-user-T24-N512-independent-bs-gradexact": 106,
}
CASES = [dataclasses.replace(c, seed=_SEEDS.get(c.key, c.seed)) for c in _cases()]
assert set(_SEEDS) <= {c.key for c in CASES}
assert len({c.key for c in CASES}) == len(CASES)


def sources():
    """every program source the cases compile, as csmc/_device.py joins it: (name, source, dx, flags of _lib.FK_USER_*, whether it defines log_g_bound)"""
    from aux_ssm_samplers_amd import _lib
    from aux_ssm_samplers_amd.csmc import DevicePotential, DeviceGaussianDynamics
    out = {}
    for sp in sorted({c.spec for c in CASES} | set(FP32_SPECS), key=lambda s: s.name):
        _, _, Mt, Gt = device(sp)
        ug, um = isinstance(Gt, DevicePotential), isinstance(Mt, DeviceGaussianDynamics)
        src = ([Gt.source] if ug else []) + ([Mt.source] if um and not (ug and Mt.source == Gt.source) else [])
        if src:
            flags = (_lib.FK_USER_POTENTIAL if ug else 0) | (_lib.FK_USER_MEAN if um else 0)
            out.setdefault(("\n".join(src), sp.dx, flags), (sp.name, "\n".join(src), sp.dx, flags, ug and " log_g_bound(" in Gt.source))
    return list(out.values())


def cases(group=None, **spec_fields):
    return [c for c in CASES if (group is None or c.group == group) and all(getattr(c.spec, k) == v for k, v in spec_fields.items())]


# fp32 against fp64 truth (section 5 of the tests): the sweeps whose stored particles and log-weights are re-evaluated by the literal
FP32_SPECS = [Spec("range", 4, 6, "user", T=60, seed=3), Spec("lorenz", 3, 3, "user", T=60, seed=3)]
FP32_N, FP32_C = 1024, 4


def fp32_chains(spec):
    """the FP32_C chains of the fp32 sweep of a spec, one Case (one set of inputs) per chain"""
    return [Case(spec, "independent", True, None, FP32_N, 20 + c, "fp32") for c in range(FP32_C)]


def teacher_forced_log_ws(spec, xs, As, dtype):
    """the literal's log-weights of the auxiliary independent sweep (AuxiliaryG0 / AuxiliaryGt: potential + prior / transition density) evaluated in `dtype` at
    given particles xs (T, N, d) and resampling ancestors As (T - 1, N)"""
    M0, G0, Mt, Gt = literal(spec, dtype)
    xs = np.asarray(xs, dtype)
    out = np.zeros(xs.shape[:2], dtype)
    out[0] = G0(xs[0]) + M0.logpdf(xs[0])
    for t in range(1, xs.shape[0]):
        xp = xs[t - 1][As[t - 1]]
        out[t] = Mt.logpdf(xs[t], xp, L._tree_index(Mt.params, t - 1)) + Gt(xs[t], xp, L._tree_index(Gt.params, t - 1))
    assert out.dtype == np.dtype(dtype)
    return out


# ---- what the exact comparison with the literal presupposes (asserted by tests/test_user_model_literals.py for every case) ---------------------------------
def exact_bound(spec):
    """sup_x log G_t per time step, (T,): what the sources' log_g_bound returns for bound == "exact" """
    d = data(spec)
    n = np.sum(np.isfinite(d["y"]), axis=1) if spec.model in ("range", "lorenz") else (np.full(spec.T, spec.dx) if spec.model == "increments" else np.ones(spec.T))
    sig = d["s"] if spec.model == "increments" else d["sig"]
    return -n * (np.log(sig) + HALF_LOG_2PI)


def wellposedness(case):
    """of the literal sweep of a case: gap = the smallest distance of a resampling / backward draw r = c[-1] (1 - u) from a cumulative-weight boundary c[j] (weights
    normalised to sum 1: tests/potential_np.py::draw_gap); ess = the smallest effective sample size over t; moved = the share of time steps whose new ancestor is not the reference particle;
    underflow32 / underflow64 = the number of steps 1 <= t < T - 1 at which every weight shifted by the exact bound (+ the transition density's log-normaliser for the
    auxiliary proposals), exp(log_w - bound), is zero in that precision"""
    sp, T = case.spec, case.spec.T
    x, B, h = literal_sweep(case)
    lit = literal(sp)
    _, _, nz = inputs(case)

    ess = [1 / np.sum(w * w) for w in map(L.normalize, h["log_ws"])]
    out = dict(gap=potential_np.draw_gap((x, B, h), nz, lit[2], case.backward), ess=float(min(ess)), moved=float(np.mean(B != 0)))
    if T > 2:
        LQ = L._tree_index(lit[2].params, 0)[2] if isinstance(lit[2].params, tuple) else lit[2].L
        c_trans = -np.sum(np.log(np.diag(LQ))) - 0.5 * sp.dx * L.LOG_2PI if case.proposal == "independent" else 0.0
        sh = h["log_ws"][1:T - 1] - (exact_bound(sp)[1:T - 1, None] + c_trans)
        with np.errstate(under="ignore"):
            out["underflow32"] = int(np.sum(np.all(np.exp(sh.astype(np.float32)) == 0, axis=1)))
            out["underflow64"] = int(np.sum(np.all(np.exp(sh) == 0, axis=1)))
        out["bound_excess"] = float(np.max(sh))   # (<= 0 up to rounding: the bound is one)
    return out


def fp32_bound_chains(case):
    """the FP32_C chains of the fp32 sweep of a bound case: the case's own inputs and three more seeds"""
    return [dataclasses.replace(case, seed=case.seed + 1000 * c) for c in range(FP32_C)]


def compare_log_ws(case, log_ws):
    """log-weights in the form in which device and literal are comparable: with the reference's gradient correction (gradient=True) the literal adds the correction
    summed over ALL particles, a constant of the step the device leaves out (csrc/csmc_sweep.h) -- there the weights relative to particle 0, for t >= 1"""
    log_ws = np.asarray(log_ws)
    if case.gradient is True:
        out = log_ws - log_ws[:, :1]
        out[0] = log_ws[0]
        return out
    return log_ws


def literal_log_ws_uncertainty(case):
    """how much the literal's own log-weights move when its central differences (csmc_np.grad_fd, h = 1e-5) take half the step: the largest change"""
    _, _, h1 = literal_sweep(case)
    _, _, h2 = literal_sweep(case, grad_h=5e-6)
    assert np.array_equal(h1["As"], h2["As"])
    return float(np.max(np.abs(compare_log_ws(case, h1["log_ws"]) - compare_log_ws(case, h2["log_ws"]))))
