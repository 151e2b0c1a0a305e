"""Example models written as device code for DevicePotential / DeviceGaussianDynamics (csmc.models; contract in csrc/fk_user_pre.h).

BUILTIN_*: the built-in potentials (Gaussian, stochastic volatility, multivariate Student-t, linear-Gaussian observation, Poisson counts, logistic counts) / bounds / linear mean of csrc/csmc_sweep.h + csrc/csmc_host.h::k_csmc_potbound written as user source, in the
built-in operation order (fma_, det_exp, det_log), so that a program sweep reproduces the closed-family sweep bit for bit (the tests and
tools/fk_program_bench.py use them).  The constants the host computes for the built-ins (csmc_host.h::fk_model) are formed the same way on
the device from theta = [sig].  RARE_EVENT, STUDENT_T, GROWTH: models the closed family cannot express.

*_GRAD / *_VJP: the same sources with the derivatives that gradient-informed proposals need (grad_log_g for a potential, mean_vjp for a mean;
csrc/fk_user_pre.h).  BUILTIN_GAUSS_OBS_GRAD, BUILTIN_SV_GRAD and BUILTIN_LINEAR_MEAN_VJP follow csrc/csmc_sweep.h::k_csmc_grad's operation
order, so that their gradient sweep is the closed family's bit for bit.  INCREMENT_OBS_GRAD: a potential that reads x_{t-1}."""

HALF_LOG_2PI = "(R)0.91893853320467274178"

# y ~ N(x, sig^2 I): theta = [sig]
BUILTIN_GAUSS_OBS = r"""
template <typename R, int D> __device__ R log_g(int t, const R* x, const R* xprev, const R* y, const R* theta) {
    const R inv = (R)1 / theta[0];
    const R c_obs = -(R)D * det_log(theta[0]) - (R)D * (R)0.91893853320467274178;
    R q = 0;
    for (int k = 0; k < D; ++k) {
        const R z = (y[k] - x[k]) * inv;
        q = fma_(z, z, q);
    }
    return fma_((R)-0.5, q, c_obs);
}
template <typename R, int D> __device__ R log_g_bound(int t, const R* y, const R* theta) {
    return -(R)D * det_log(theta[0]) - (R)D * (R)0.91893853320467274178;
}
"""

# stochastic volatility y_k ~ N(0, exp(x_k)), NaN terms -> 0; the bound of k_csmc_potbound
BUILTIN_SV = r"""
template <typename R, int D> __device__ R log_g(int t, const R* x, const R* xprev, const R* y, const R* theta) {
    const R c_obs = -(R)0.91893853320467274178;
    R acc = 0;
    for (int k = 0; k < D; ++k) {
        const R e = det_exp(-x[k]);
        const R s = fma_(y[k] * y[k], e, x[k]);
        const R v = fma_((R)-0.5, s, c_obs);
        acc += (v == v) ? v : (R)0;
    }
    return acc;
}
template <typename R, int D> __device__ R log_g_bound(int t, const R* y, const R* theta) {
    const R c_obs = -(R)0.91893853320467274178;
    R b = 0;
    for (int k = 0; k < D; ++k) {
        const R yk = y[k], y2 = yk * yk;
        R v = (R)0;
        if (y2 - y2 == 0) v = y2 > (R)0 ? fma_((R)-0.5, (R)1 + det_log(y2), c_obs) : (R)INFINITY;
        b += v > (R)0 ? v : (R)0;
    }
    return b;
}
"""

# multivariate Student-t with a precision matrix (AUXSSM_POT_MVT): theta = [nu | prec (D x D, row-major)]; csrc/csmc_sweep.h::coupled_resid / mvt_value in their order,
# the two constants formed as csmc_host.h::fk_model forms them; sup_x log g = 0
BUILTIN_MVT = r"""
template <typename R, int D> __device__ R mvt_s_(const R* x, const R* y, const R* theta, R* z) {
    const R inv_nu = (R)1 / theta[0];
    const R* P = theta + 1;
    R r[D];
    for (int k = 0; k < D; ++k) r[k] = x[k] - y[k];
    R q = 0;
    for (int k = 0; k < D; ++k) {
        R acc = 0;
        for (int j = 0; j < D; ++j) acc = fma_(P[k * D + j], r[j], acc);
        z[k] = acc;
    }
    for (int k = 0; k < D; ++k) q = fma_(z[k], r[k], q);
    return (R)1 + q * inv_nu;
}
template <typename R, int D> __device__ R log_g(int t, const R* x, const R* xprev, const R* y, const R* theta) {
    R z[D];
    const R hc = (theta[0] + (R)D) / (R)2;
    const R v = -hc * det_log(mvt_s_<R, D>(x, y, theta, z));
    return (v == v) ? v : (R)0;
}
template <typename R, int D> __device__ R log_g_bound(int t, const R* y, const R* theta) { return (R)0; }
"""

# linear-Gaussian observation y ~ N(H x + c, R) in the whitened residual form (AUXSSM_POT_LIN_GAUSS): theta = [c_lin | Hw (D x D, row-major, rows beyond dy zero)],
# observations = the whitened rows yw (T, D); csrc/csmc_sweep.h::coupled_resid / lin_value in their order; the bound of k_csmc_potbound (c_lin, 0 on a NaN row)
BUILTIN_LINGAUSS = r"""
template <typename R, int D> __device__ R lin_q_(const R* x, const R* y, const R* theta, R* z) {
    const R* H = theta + 1;
    for (int k = 0; k < D; ++k) {
        R acc = 0;
        for (int j = 0; j < D; ++j) acc = fma_(H[k * D + j], x[j], acc);
        z[k] = y[k] - acc;
    }
    R q = 0;
    for (int k = 0; k < D; ++k) q = fma_(z[k], z[k], q);
    return q;
}
template <typename R, int D> __device__ R log_g(int t, const R* x, const R* xprev, const R* y, const R* theta) {
    R z[D];
    const R v = fma_((R)-0.5, lin_q_<R, D>(x, y, theta, z), theta[0]);
    return (v == v) ? v : (R)0;
}
template <typename R, int D> __device__ R log_g_bound(int t, const R* y, const R* theta) {
    bool obs = true;
    for (int k = 0; k < D; ++k) obs = obs && (y[k] - y[k] == 0);
    return obs ? theta[0] : (R)0;
}
"""

# Poisson counts with a log link y_k ~ Poisson(exp(x_k)) (AUXSSM_POT_POISSON), the -log y_k! constant left out; no theta.  The order of include/auxssm.h, restated:
# e_k = det_exp(x_k);  v_k = fma_(y_k, x_k, -e_k);  v_k counts only if y_k - y_k == 0;  accumulated over k ascending from 0.  Gradient y_k - det_exp(x_k), 0 for a
# missing component.  Bound (k_csmc_potbound): sum_k (y_k > 0 ? y_k (det_log(y_k) - 1) : 0).  One source with the derivative: it serves plain and gradient programs.
BUILTIN_POISSON = r"""
template <typename R, int D> __device__ R log_g(int t, const R* x, const R* xprev, const R* y, const R* theta) {
    R acc = 0;
    for (int k = 0; k < D; ++k) {
        const R e = det_exp(x[k]);
        const R v = fma_(y[k], x[k], -e);
        acc += (y[k] - y[k] == 0) ? v : (R)0;
    }
    return acc;
}
template <typename R, int D> __device__ R log_g_bound(int t, const R* y, const R* theta) {
    R b = 0;
    for (int k = 0; k < D; ++k) b += y[k] > (R)0 ? y[k] * (det_log(y[k]) - (R)1) : (R)0;
    return b;
}
template <typename R, int D> __device__ void grad_log_g(int t, const R* x, const R* xprev, const R* y, const R* theta, R* gx, R* gxprev) {
    for (int k = 0; k < D; ++k) gx[k] = (y[k] - y[k] == 0) ? y[k] - det_exp(x[k]) : (R)0;
}
"""

# Binomial / negative-binomial counts with a logit link (AUXSSM_POT_LOGISTIC), the combinatorial constant left out; no theta.  The observation rows are
# [y (D) | m (D)], p = 2 D: the data, then the sizes (the built-in kind reads the sizes from plane 1 of its (2, T, D) array).  The order of include/auxssm.h,
# restated:  e = det_exp(-|x_k|);  l = det_log(1 + e);  sp = max(x_k, 0) + l;  v_k = fma_(y_k, x_k, -(m_k sp)), counted only if y_k - y_k == 0, accumulated over
# k ascending from 0.  Gradient: r = 1 / (1 + e), s = x_k >= 0 ? r : e r, fma_(-m_k, s, y_k), 0 for a missing component.  Bound (k_csmc_potbound): the binomial
# log-likelihood at p = y / m without cancellation.  One source with the derivative: it serves plain and gradient programs.
BUILTIN_LOGISTIC = r"""
template <typename R, int D> __device__ R log_g(int t, const R* x, const R* xprev, const R* y, const R* theta) {
    R acc = 0;
    for (int k = 0; k < D; ++k) {
        const R e = det_exp(-(x[k] < (R)0 ? -x[k] : x[k]));
        const R l = det_log((R)1 + e);
        const R sp = (x[k] > (R)0 ? x[k] : (R)0) + l;
        const R v = fma_(y[k], x[k], -(y[D + k] * sp));
        acc += (y[k] - y[k] == 0) ? v : (R)0;
    }
    return acc;
}
template <typename R, int D> __device__ R log_g_bound(int t, const R* y, const R* theta) {
    R b = 0;
    for (int k = 0; k < D; ++k) {
        const R yk = y[k], mk = y[D + k], nk = mk - yk;
        const R v = (yk > (R)0 ? yk * det_log(yk / mk) : (R)0) + (nk > (R)0 ? nk * det_log(nk / mk) : (R)0);
        b += (yk - yk == 0) ? v : (R)0;
    }
    return b;
}
template <typename R, int D> __device__ void grad_log_g(int t, const R* x, const R* xprev, const R* y, const R* theta, R* gx, R* gxprev) {
    for (int k = 0; k < D; ++k) {
        const R e = det_exp(-(x[k] < (R)0 ? -x[k] : x[k]));
        const R r = (R)1 / ((R)1 + e);
        const R s = x[k] >= (R)0 ? r : e * r;
        gx[k] = (y[k] - y[k] == 0) ? fma_(-y[D + k], s, y[k]) : (R)0;
    }
}
"""

# mean F x + b: theta = [F (D x D, row-major) | b (D)]
BUILTIN_LINEAR_MEAN = r"""
template <typename R, int D> __device__ void mean(int t, const R* xprev, const R* theta, R* mu) {
    for (int k = 0; k < D; ++k) {
        R acc = theta[D * D + k];
        for (int j = 0; j < D; ++j) acc = fma_(theta[k * D + j], xprev[j], acc);
        mu[k] = acc;
    }
}
"""

# the reference's rare-event example (examples/rare_event/auxiliary_csmc.py): AR(1) x_t = rho x_{t-1} + sqrt(1 - rho^2) eps, and a potential that is
# zero except at t = T - 1, log N(y; x, r^2).  theta_g = [T, y, r], theta_m = [rho]
RARE_EVENT = r"""
template <typename R, int D> __device__ R log_g(int t, const R* x, const R* xprev, const R* y, const R* theta) {
    if (t != (int)theta[0] - 1) return (R)0;
    const R z = (theta[1] - x[0]) / theta[2];
    return (R)-0.5 * (z * z) - log(theta[2]) - (R)0.91893853320467274178;
}
template <typename R, int D> __device__ R log_g_bound(int t, const R* y, const R* theta) {
    return t == (int)theta[0] - 1 ? -log(theta[2]) - (R)0.91893853320467274178 : (R)0;
}
template <typename R, int D> __device__ void mean(int t, const R* xprev, const R* theta, R* mu) {
    mu[0] = theta[0] * xprev[0];
}
"""

# Student-t observations y_k ~ x_k + s t_nu: theta = [nu, s]
STUDENT_T = r"""
template <typename R, int D> __device__ R log_g(int t, const R* x, const R* xprev, const R* y, const R* theta) {
    const R nu = theta[0], s = theta[1];
    const R c = lgamma((nu + (R)1) / (R)2) - lgamma(nu / (R)2) - (R)0.5 * log(nu * (R)3.14159265358979323846 * s * s);
    R acc = 0;
    for (int k = 0; k < D; ++k) {
        const R z = (y[k] - x[k]) / s;
        acc += c - (nu + (R)1) / (R)2 * log1p(z * z / nu);
    }
    return acc;
}
"""

# the classic nonlinear growth model: x_t = x/2 + 25 x / (1 + x^2) + 8 cos(1.2 t) + noise, y_t ~ N(x_t^2 / 20, sig^2): theta_g = [sig]
GROWTH = r"""
template <typename R, int D> __device__ R log_g(int t, const R* x, const R* xprev, const R* y, const R* theta) {
    const R z = (y[0] - x[0] * x[0] / (R)20) / theta[0];
    return (R)-0.5 * (z * z) - log(theta[0]) - (R)0.91893853320467274178;
}
template <typename R, int D> __device__ void mean(int t, const R* xprev, const R* theta, R* mu) {
    const R v = xprev[0];
    mu[0] = v / (R)2 + (R)25 * v / ((R)1 + v * v) + (R)8 * cos((R)1.2 * (R)t);
}
"""


# ---- with derivatives (gradient-informed proposals) -----------------------------------------------------------------------------------------------
# d/dx log N(y; x, sig^2 I) = (y - x) / sig^2, as ((y - x) inv) inv
BUILTIN_GAUSS_OBS_GRAD = BUILTIN_GAUSS_OBS + r"""
template <typename R, int D> __device__ void grad_log_g(int t, const R* x, const R* xprev, const R* y, const R* theta, R* gx, R* gxprev) {
    const R inv = (R)1 / theta[0];
    for (int k = 0; k < D; ++k) gx[k] = ((y[k] - x[k]) * inv) * inv;
}
"""

# d/dx log g = (-(hc + hc) / nu / s) z with s = 1 + q / nu, z = prec (x - y); every component 0 where s is NaN (csrc/csmc_sweep.h::coupled_grad)
BUILTIN_MVT_GRAD = BUILTIN_MVT + r"""
template <typename R, int D> __device__ void grad_log_g(int t, const R* x, const R* xprev, const R* y, const R* theta, R* gx, R* gxprev) {
    R z[D];
    const R hc = (theta[0] + (R)D) / (R)2, inv_nu = (R)1 / theta[0];
    const R s = mvt_s_<R, D>(x, y, theta, z);
    const R c = -((hc + hc) * inv_nu) / s;
    for (int k = 0; k < D; ++k) gx[k] = (s == s) ? c * z[k] : (R)0;
}
"""

# d/dx log g = Hw^T z with z = yw - Hw x (component j: fma over k ascending); every component 0 where the value is NaN (csrc/csmc_sweep.h::coupled_grad)
BUILTIN_LINGAUSS_GRAD = BUILTIN_LINGAUSS + r"""
template <typename R, int D> __device__ void grad_log_g(int t, const R* x, const R* xprev, const R* y, const R* theta, R* gx, R* gxprev) {
    R z[D];
    const R* H = theta + 1;
    const R v = fma_((R)-0.5, lin_q_<R, D>(x, y, theta, z), theta[0]);
    for (int j = 0; j < D; ++j) {
        R acc = 0;
        for (int k = 0; k < D; ++k) acc = fma_(H[k * D + j], z[k], acc);
        gx[j] = (v == v) ? acc : (R)0;
    }
}
"""

# d/dx_k of -0.5 (y_k^2 e^{-x_k} + x_k) = 0.5 (y_k^2 e^{-x_k} - 1), NaN -> 0
BUILTIN_SV_GRAD = BUILTIN_SV + r"""
template <typename R, int D> __device__ void grad_log_g(int t, const R* x, const R* xprev, const R* y, const R* theta, R* gx, R* gxprev) {
    for (int k = 0; k < D; ++k) {
        const R e = det_exp(-x[k]);
        const R v = (R)0.5 * fma_(y[k] * y[k], e, (R)-1);
        gx[k] = (v == v) ? v : (R)0;
    }
}
"""

# J = F: out = F^T v
BUILTIN_LINEAR_MEAN_VJP = BUILTIN_LINEAR_MEAN + r"""
template <typename R, int D> __device__ void mean_vjp(int t, const R* xprev, const R* theta, const R* v, R* out) {
    for (int k = 0; k < D; ++k) {
        R acc = 0;
        for (int j = 0; j < D; ++j) acc = fma_(theta[j * D + k], v[j], acc);
        out[k] = acc;
    }
}
"""

RARE_EVENT_GRAD = RARE_EVENT + r"""
template <typename R, int D> __device__ void grad_log_g(int t, const R* x, const R* xprev, const R* y, const R* theta, R* gx, R* gxprev) {
    if (t == (int)theta[0] - 1) gx[0] = (theta[1] - x[0]) / (theta[2] * theta[2]);
}
template <typename R, int D> __device__ void mean_vjp(int t, const R* xprev, const R* theta, const R* v, R* out) {
    out[0] = theta[0] * v[0];
}
"""

# d/dx_k [-(nu + 1) / 2 log1p(z^2 / nu)], z = (y_k - x_k) / s:  (nu + 1) z / (s (nu + z^2))
STUDENT_T_GRAD = STUDENT_T + r"""
template <typename R, int D> __device__ void grad_log_g(int t, const R* x, const R* xprev, const R* y, const R* theta, R* gx, R* gxprev) {
    const R nu = theta[0], s = theta[1];
    for (int k = 0; k < D; ++k) {
        const R z = (y[k] - x[k]) / s;
        gx[k] = (nu + (R)1) * z / (s * (nu + z * z));
    }
}
"""

# potential: z x / (10 sig) with z = (y - x^2 / 20) / sig;  mean: d/dv [v / 2 + 25 v / (1 + v^2)] = 1 / 2 + 25 (1 - v^2) / (1 + v^2)^2
GROWTH_GRAD = GROWTH + r"""
template <typename R, int D> __device__ void grad_log_g(int t, const R* x, const R* xprev, const R* y, const R* theta, R* gx, R* gxprev) {
    const R z = (y[0] - x[0] * x[0] / (R)20) / theta[0];
    gx[0] = z * x[0] / ((R)10 * theta[0]);
}
template <typename R, int D> __device__ void mean_vjp(int t, const R* xprev, const R* theta, const R* v, R* out) {
    const R a = xprev[0], q = (R)1 + a * a;
    out[0] = ((R)0.5 + (R)25 * ((R)1 - a * a) / (q * q)) * v[0];
}
"""

# observed increments: y_t ~ N(x_t - x_{t-1}, s^2 I) (y_0 ~ N(x_0, s^2 I)), a potential of (x_t, x_{t-1}): theta = [s]
INCREMENT_OBS_GRAD = r"""
template <typename R, int D> __device__ R log_g(int t, const R* x, const R* xprev, const R* y, const R* theta) {
    const R s = theta[0];
    R acc = 0;
    for (int k = 0; k < D; ++k) {
        const R z = (y[k] - (xprev ? x[k] - xprev[k] : x[k])) / s;
        acc += (R)-0.5 * (z * z) - log(s) - (R)0.91893853320467274178;
    }
    return acc;
}
template <typename R, int D> __device__ R log_g_bound(int t, const R* y, const R* theta) {
    return (R)D * (-log(theta[0]) - (R)0.91893853320467274178);
}
template <typename R, int D> __device__ void grad_log_g(int t, const R* x, const R* xprev, const R* y, const R* theta, R* gx, R* gxprev) {
    const R s = theta[0];
    for (int k = 0; k < D; ++k) {
        const R z = (y[k] - (xprev ? x[k] - xprev[k] : x[k])) / s;
        gx[k] = z / s;
        if (gxprev) gxprev[k] = -z / s;
    }
}
"""
