"""Built-in device model factories for the auxiliary Kalman sampler.

The reference's factories are JAX closures traced into the sweep; a Python callable cannot run inside a HIP
kernel, so models whose factories are known in closed form are provided as device factories and the whole sweep
(auxssm_kalman_sweep) stays in HBM.  Arbitrary NumPy factories still work through the generic host path of
kalman.get_kernel.
"""
import numpy as np

from .. import _lib, _logistic
from .._primitives.kalman.base import DeviceLGSSM, _upload_arr


class _BuiltinModel:
    """What the built-in device models have in common, and what kalman.get_kernel knows one by (generic._same_device_model): the model kind `kmodel` of
    include/auxssm.h, the sizes T, dx, p_obs, the data yobs (T, p_obs), and the uploads, made once per (handle, dtype): a subclass gives _upload(handle, dtype)
    -> the model's C struct with the buffers it points at; the data is uploaded here."""
    dense_only = False  # >= 32 chains run chain-minor (lanes over chains)
    _yname = "ys"

    def device(self, handle, dtype):
        """-> (model, data buffer, data array descriptor) on the handle's device"""
        key = (id(handle), np.dtype(dtype).str)
        dev = self._dev.get(key)
        if dev is None:
            dl = self._upload(handle, dtype)
            ybuf, yarr = _upload_arr(handle, self.yobs, (self.p_obs,), 1, self.T, 1, False, False, np.dtype(dtype), self._yname)
            dev = self._dev[key] = (dl, ybuf, yarr)
        return dev


def _state_space_observations(order, x, u, delta, grad, lam):
    """The auxiliary observation set of examples/stochastic_volatility/auxiliary_kalman.py:28-46 for a potential with gradient grad (T, d) and lam = -hess at x,
    diagonal (T, d) or dense (T, d, d); it lives in the state space, H = I, c = 0:
        order 1: ys = u + delta/2 grad,                               R = delta/2 I
        order 2: Om = (lam + 2/delta I)^-1 (a dense one symmetrised), ys = Om (2u/delta + grad + lam x), R = Om
    -> ys, Hs, Rs, cs in u's dtype"""
    T, d = u.shape
    dt = u.dtype
    eyes = np.broadcast_to(np.eye(d, dtype=dt), (T, d, d))
    zeros = np.zeros((T, d), dt)
    if order == 1:
        return (u + 0.5 * delta * grad).astype(dt), eyes, (0.5 * delta * eyes).astype(dt), zeros
    hess = -lam  # (the reference's own terms, -hess + 2/delta and grad - hess x: the same numbers, and for SVModel's missing data the same NaN to the bit)
    if lam.ndim == 2:
        om = 1.0 / (-hess + 2.0 / delta)
        ys = om * (2.0 * u / delta + grad - hess * x)
        Rs = np.zeros((T, d, d), dt)
        Rs[:, np.arange(d), np.arange(d)] = om
    else:
        om = np.linalg.inv(-hess + (2.0 / delta) * np.eye(d))
        om = 0.5 * (om + np.swapaxes(om, -1, -2))
        ys = np.einsum("tkl,tl->tk", om, 2.0 * u / delta + grad - np.einsum("tkl,tl->tk", hess, x))
        Rs = om.astype(dt)
    return ys.astype(dt), eyes, Rs, zeros


class LGConcatModel(_BuiltinModel):
    """Linear-Gaussian SSM with the auxiliary observations concatenated to the real ones
    (the observation-factory pattern of examples/lorenz/auxiliary_kalman.py:26-35):

        dynamics_factory(x)            -> m0, P0, Fs, Qs, bs                       (independent of x)
        observations_factory(x, u, d)  -> ys=[u; y], Hs=[I; Hobs], Rs=blkdiag(d/2 I, Robs), cs=[0; cobs]
        log_likelihood_fn(x)           -> prior_logpdf(x) + sum_t log N(y_t; Hobs_t x_t + cobs_t, Robs_t)

    Pass the three bound methods to kalman.get_kernel; it recognises them and runs the fused device sweep.
    The same methods are plain NumPy factories, so they also drive the generic host path (and the oracle)."""

    kmodel = _lib.KMODEL_LG_CONCAT
    _yname = "yobs"

    def __init__(self, m0, P0, Fs, Qs, bs, Hobs, Robs, cobs, yobs):
        self.m0, self.P0, self.Fs, self.Qs, self.bs = m0, P0, Fs, Qs, bs
        self.Hobs, self.Robs, self.cobs, self.yobs = Hobs, Robs, cobs, yobs
        self.T = np.shape(yobs)[0]
        self.dx = np.shape(m0)[-1]
        self.p_obs = np.shape(yobs)[-1]
        self._dev = {}

    # ---- NumPy factories (reference call signatures: kalman/generic.py:80-81,89) ----
    def dynamics_factory(self, x):
        return self.m0, self.P0, self.Fs, self.Qs, self.bs

    def observations_factory(self, x, u, delta):
        T, d, po = self.T, self.dx, self.p_obs
        dt = np.asarray(u).dtype
        P = d + po
        ys = np.concatenate([u, np.asarray(self.yobs, dt)], axis=-1)
        Hs = np.concatenate([np.broadcast_to(np.eye(d, dtype=dt), (T, d, d)), np.asarray(self.Hobs, dt)], axis=1)
        Rs = np.zeros((T, P, P), dt)
        Rs[:, :d, :d] = 0.5 * delta * np.eye(d)
        Rs[:, d:, d:] = self.Robs
        cs = np.concatenate([np.zeros((T, d), dt), np.asarray(self.cobs, dt)], axis=-1)
        return ys, Hs, Rs, cs

    def log_likelihood_fn(self, x):
        from .._primitives.kalman.base import joint_logpdf, LGSSM
        return joint_logpdf(self.yobs, x, LGSSM(self.m0, self.P0, self.Fs, self.Qs, self.bs, self.Hobs, self.Robs, self.cobs))

    # ---- device side ----
    def _upload(self, handle, dtype):
        lg = (self.m0, self.P0, self.Fs, self.Qs, self.bs, self.Hobs, self.Robs, self.cobs)
        return DeviceLGSSM(handle, lg, 1, self.T, 1, self.dx, self.p_obs, False, dtype)


class _StateSpaceModel(_BuiltinModel):
    """What SVModel, PoissonModel and PoissonLinearModel share: data ys (T, p_obs), time-invariant linear-Gaussian dynamics (m0, P0, F, Q, b) on a state of dx
    components (ys's width unless said) and a potential whose first- or second-order auxiliary observation set lives in the state space
    (_state_space_observations).  A subclass sets KMODELS = (first-order kind, second-order kind) and gives log_potential(x) and grad_lam(x) -> (grad (T, dx),
    lam = -hess: (T, dx) where the potential is a sum over the components, else (T, dx, dx))."""
    KMODELS = None

    def __init__(self, ys, m0, P0, F, Q, b, order=1, dx=None):
        if order not in (1, 2):
            raise ValueError("order must be 1 or 2")
        self.yobs = np.asarray(ys)
        self.T, self.p_obs = self.yobs.shape
        self.dx = self.p_obs if dx is None else dx
        self.m0, self.P0 = np.asarray(m0), np.asarray(P0)
        self.F, self.Q, self.b = np.asarray(F), np.asarray(Q), np.asarray(b)
        self.order = order
        self.kmodel = self.KMODELS[order - 1]
        n = self.T - 1
        self.Fs = np.broadcast_to(self.F, (n,) + self.F.shape)
        self.Qs = np.broadcast_to(self.Q, (n,) + self.Q.shape)
        self.bs = np.broadcast_to(self.b, (n,) + self.b.shape)
        self._dev = {}

    def dynamics_factory(self, x):
        return self.m0, self.P0, self.Fs, self.Qs, self.bs

    def log_likelihood_fn(self, x):
        from .._primitives.kalman.base import prior_logpdf, LGSSM
        x = np.asarray(x)
        prior = prior_logpdf(x, LGSSM(self.m0, self.P0, self.Fs, self.Qs, self.bs, None, None, None))
        return prior + self.log_potential(x)

    def observations_factory(self, x, u, delta):
        x, u = np.asarray(x), np.asarray(u)
        with np.errstate(all="ignore"):
            return _state_space_observations(self.order, x, u, delta, *self.grad_lam(x))

    def _upload(self, handle, dtype):
        lg = (self.m0, self.P0, self.Fs, self.Qs, self.bs, None, None, None)
        return DeviceLGSSM(handle, lg, 1, self.T, 1, self.dx, self.dx, False, dtype)


class SVModel(_StateSpaceModel):
    """Multivariate stochastic volatility  y_{t,k} ~ N(0, exp(x_{t,k}))  on linear-Gaussian dynamics
    x_{t+1} = F x_t + b + N(0, Q), with the first- or second-order auxiliary observation factories of
    examples/stochastic_volatility/auxiliary_kalman.py:22-48 (closed-form gradient / Hessian of the potential,
    model.py:56-82, instead of jax.grad):

        dynamics_factory(x)           -> m0, P0, tile(F), tile(Q), tile(b)                        (:22-26)
        observations_factory(x, u, d) -> order 1: ys = u + d/2 grad(x), H = I, R = d/2 I, c = 0     (:28-35)
                                         order 2: Om = (-hess + 2/d I)^-1, ys = Om (2u/d + grad - hess x), H = I, R = Om (:37-46)
        log_likelihood_fn(x)          -> log N(x_0; m0, P0) + sum_t log N(x_t; F x_{t-1} + b, Q) + sum log g   (:48-52)

    Pass the three bound methods to kalman.get_kernel: it runs the device sweep (auxssm_kalman_sweep, model kind SV_FIRST /
    SV_SECOND).  The same methods are NumPy factories for the host path and the oracle."""
    KMODELS = (_lib.KMODEL_SV_FIRST, _lib.KMODEL_SV_SECOND)

    # potential and its derivatives (model.py:56-82), NaN -> 0 as jnp.nan_to_num
    def _w(self, x):
        return self.yobs.astype(x.dtype) ** 2 * np.exp(-x)

    def log_potential(self, x):
        x = np.asarray(x)
        with np.errstate(all="ignore"):
            val = -0.5 * np.log(2 * np.pi) - 0.5 * x - 0.5 * self._w(x)
        return float(np.sum(np.nan_to_num(val)))

    def grad_lam(self, x):
        """(grad, lam) of log g, both (T, dx): grad NaN -> 0, lam = -hess NaN where y is"""
        with np.errstate(all="ignore"):
            w = self._w(np.asarray(x))
            return np.nan_to_num(0.5 * (w - 1.0)), -(-0.5 * w)   # (hess negated, as the reference writes it: w / 2, and the same NaN where y is missing)


class PoissonModel(_StateSpaceModel):
    """Multivariate counts with a log link  y_{t,k} ~ Poisson(exp(x_{t,k}))  on linear-Gaussian dynamics x_{t+1} = F x_t + b + N(0, Q), x_0 ~ N(m0, P0),
    under the first- or second-order auxiliary observation factories of examples/stochastic_volatility/auxiliary_kalman.py:22-48.  Arguments and shapes
    are SVModel's: ys (T, dx), F and Q dense (dx, dx), order 1 or 2.  With mask = isfinite(y), per component

        log g = where(mask, y x - e^x, 0)      grad = where(mask, y - e^x, 0)      lam = -hess = where(mask, e^x, 0)

        dynamics_factory(x)           -> m0, P0, tile(F), tile(Q), tile(b)
        observations_factory(x, u, d) -> order 1: ys = u + d/2 grad, H = I, R = d/2 I, c = 0
                                         order 2: Om = 1 / (lam + 2/d) (diagonal), ys = Om (2u/d + grad + lam x), H = I, R = diag(Om), c = 0
        log_likelihood_fn(x)          -> prior_logpdf(x) + sum log g

    The conventions are csmc.PoissonPotential's, so both samplers target one density: the constant -log y! is left out, non-integer y >= 0 is accepted, a
    finite negative entry raises ValueError, a NaN y_{t,k} drops that component's term alone, and a log-exposure is a shift of the state through m0 and b (no
    field).  The potential is concave and -hess = e^x > 0, so the second-order factory is always well defined.  Unlike SVModel's, no pseudo-observation is
    ever NaN: a missing count leaves its component observed through u with variance d/2, in both orders.  exp overflow (|x| beyond ~88 in float32, ~709 in
    float64) is not guarded.

    Pass the three bound methods to kalman.get_kernel: it runs the device sweep (model kind POISSON_FIRST / POISSON_SECOND: the SV sweep's kernels
    instantiated for this potential, every layout and width SVModel has).  The same methods are NumPy factories for the host path and the oracle."""
    KMODELS = (_lib.KMODEL_POISSON_FIRST, _lib.KMODEL_POISSON_SECOND)

    def __init__(self, ys, m0, P0, F, Q, b, order=1):
        ys = np.asarray(ys)
        if ys.ndim != 2:
            raise ValueError(f"PoissonModel: ys must be (T, dx), got shape {ys.shape}")
        from ..csmc.models import PoissonPotential
        PoissonPotential.check_counts(ys)
        super().__init__(ys, m0, P0, F, Q, b, order)

    def _terms(self, x):
        """(mask, e^x) at x (T, dx)"""
        with np.errstate(over="ignore"):
            return np.isfinite(self.yobs), np.exp(x)

    def log_potential(self, x):
        x = np.asarray(x)
        mask, e = self._terms(x)
        with np.errstate(invalid="ignore"):
            return float(np.sum(np.where(mask, self.yobs.astype(x.dtype) * x - e, 0.0)))

    def grad_lam(self, x):
        """(grad, lam) of log g, both (T, dx) and 0 where the count is missing"""
        x = np.asarray(x)
        mask, e = self._terms(x)
        with np.errstate(invalid="ignore"):
            return np.where(mask, self.yobs.astype(x.dtype) - e, 0.0), np.where(mask, e, 0.0)


def _loading_arguments(who, ys, H, c, order, max_dx, max_dy):
    """What the models behind a loading matrix check first: order, ys (T, dy), H (dy, dx) finite, c a finite scalar or (dy,), 1 <= dx <= max_dx, 1 <= dy <= max_dy
    -> ys as an array, H and c (dy,) in float64; who: the class named in the messages"""
    if order not in (1, 2):
        raise ValueError("order must be 1 or 2")
    ys = np.asarray(ys)
    if ys.ndim != 2:
        raise ValueError(f"{who}: ys must be (T, dy), got shape {ys.shape}")
    H = np.asarray(H, np.float64)
    if H.ndim != 2 or H.shape[0] != ys.shape[1]:
        raise ValueError(f"{who}: H must be (dy, dx) = ({ys.shape[1]}, dx), got shape {H.shape}")
    T, dy = ys.shape
    dx = H.shape[1]
    if not 1 <= dx <= max_dx:
        raise NotImplementedError(f"{who}: dx = {dx}: the sweep covers 1 <= dx <= {max_dx}")
    if not 1 <= dy <= max_dy:
        raise NotImplementedError(f"{who}: dy = {dy}: the sweep covers 1 <= dy <= {max_dy}")
    if not np.all(np.isfinite(H)):
        raise ValueError(f"{who}: H must be finite")
    c = np.asarray(c, np.float64)
    if c.ndim == 0:
        c = np.full(dy, float(c))
    if c.shape != (dy,) or not np.all(np.isfinite(c)):
        raise ValueError(f"{who}: c must be a finite scalar or ({dy},) vector, got shape {c.shape}")
    return ys, H, c


def _check_dynamics_shapes(who, model):
    dx = model.dx
    if model.m0.shape != (dx,) or model.b.shape != (dx,) or any(a.shape != (dx, dx) for a in (model.P0, model.F, model.Q)):
        raise ValueError(f"{who}: m0, b must be ({dx},) and P0, F, Q ({dx}, {dx})")


class PoissonLinearModel(_StateSpaceModel):
    """Poisson counts through a loading matrix (the Poisson linear dynamical system, a dynamic Poisson factor model): a low-dimensional linear-Gaussian state
    drives many count channels,

        x_0 ~ N(m0, P0),   x_{t+1} = F x_t + b + N(0, Q),   y_{t,j} ~ Poisson(exp(h_j' x_t + c_j)),   j = 1..dy,

    under the first- or second-order auxiliary observation factories of examples/stochastic_volatility/auxiliary_kalman.py:22-48.  ys (T, dy): counts >= 0, NaN =
    missing; H (dy, dx) dense and finite; c (dy,) or a scalar; the dynamics arguments are SVModel's; 1 <= dx <= MAX_DX = 4, 1 <= dy <= MAX_DY = 1024.  With
    mask = isfinite(y), eta_t = H x_t + c, e = where(mask, exp(eta), 0), yy = where(mask, y, 0):

        log g_t = sum_j yy_j eta_j - e_j       grad_t = H' (yy - e)  (dx)       Lam_t = H' diag(e) H = -hess  (dx x dx, symmetric PSD)

        dynamics_factory(x)           -> m0, P0, tile(F), tile(Q), tile(b)
        observations_factory(x, u, d) -> order 1: ys = u + d/2 grad,                                            H_obs = I, R = d/2 I, c_obs = 0
                                         order 2: Om = sym((Lam + 2/d I)^-1), ys = Om (2u/d + grad + Lam x),    H_obs = I, R = Om,    c_obs = 0
        log_likelihood_fn(x)          -> prior_logpdf(x) + sum_t log g_t

    The pseudo-observation of both orders lives in the state space, so the filter and the pathwise sampler are the dx <= 4 register kernels however large dy is;
    the dy-dependent work is a reduction over the channels per (chain, step) (csrc/kalman_plin.hip).  The conventions are PoissonModel's, so the samplers share
    one density: the constant -log y! is left out, non-integer y >= 0 is accepted, a finite negative entry raises ValueError, a NaN y_{t,j} drops that channel's
    term alone.  Lam is PSD, so order 2 is always defined.  With H = I, c = 0, dy = dx the model is PoissonModel.  exp overflow (|eta| beyond ~88 in float32,
    ~709 in float64) is not guarded.

    The first-order proposal is only usable for delta * lambda_max(Lam_t) of order 1: at dy >= 65 with delta = 0.05 the oracle's own log alpha was -1e3 to
    -1e70.  That is the linearisation, not a defect; the second order has no such limit.

    Pass the three bound methods to kalman.get_kernel: it runs the device sweep (model kind POISSON_LIN_FIRST / _SECOND) on host states (T, dx) or (C, T, dx),
    or on resident DeviceChains(handle, x (C, T, dx), chain_minor=False): the dense layout only.  The same methods are NumPy factories for the host path and
    the oracle."""
    KMODELS = (_lib.KMODEL_POISSON_LIN_FIRST, _lib.KMODEL_POISSON_LIN_SECOND)
    dense_only = True
    MAX_DX = 4
    MAX_DY = 1024

    def __init__(self, ys, H, c, m0, P0, F, Q, b, order=1):
        ys, H, c = _loading_arguments("PoissonLinearModel", ys, H, c, order, self.MAX_DX, self.MAX_DY)
        from ..csmc.models import PoissonPotential
        PoissonPotential.check_counts(ys)
        super().__init__(ys, m0, P0, F, Q, b, order, dx=H.shape[1])
        self.H, self.c = H, c
        _check_dynamics_shapes("PoissonLinearModel", self)

    def _terms(self, x):
        """(mask, eta, e, yy) at x (T, dx), each (T, dy)"""
        x = np.asarray(x)
        eta = x @ self.H.astype(x.dtype).T + self.c.astype(x.dtype)
        mask = np.isfinite(self.yobs)
        with np.errstate(over="ignore"):
            e = np.where(mask, np.exp(eta), 0.0)
        return mask, eta, e, np.where(mask, self.yobs, 0.0).astype(x.dtype)

    def log_potential(self, x):
        _, eta, e, yy = self._terms(x)
        return float(np.sum(yy * eta - e))

    def grad_lam(self, x):
        """(grad (T, dx), Lam (T, dx, dx)) of log g: H' (yy - e) and H' diag(e) H"""
        _, _, e, yy = self._terms(x)
        H = self.H.astype(e.dtype)
        lam = np.einsum("tj,jk,jl->tkl", e, H, H)
        return (yy - e) @ H, 0.5 * (lam + np.swapaxes(lam, -1, -2))   # (symmetric to the last bit)

    def _upload(self, handle, dtype):
        dl = super()._upload(handle, dtype)
        # include/auxssm.h, POISSON_LIN_FIRST / _SECOND: the loading matrix (dy, dx) row-major rides in the Hs slot, the offsets (dy) in the cs slot
        for name, a in (("Hs", self.H), ("cs", self.c)):
            buf = dl.bufs["plin_" + name] = handle.to_device(np.ascontiguousarray(a, np.float64), dtype)
            setattr(dl.c, name, buf.arr(0, 0, 0))
        return dl


class _LogisticModel(_StateSpaceModel):
    """What BinomialModel and NegBinomialModel share: one potential with a logit link and a SIZE m (T, dx) beside the data.  With mask = isfinite(y),
    e = exp(-|x|), r = 1 / (1 + e), sigma = where(x >= 0, r, e r) and 1 - sigma its mirror image (never a subtraction), per component

        log g = where(mask, y x - m softplus(x), 0)      grad = where(mask, y - m sigma, 0)      lam = -hess = where(mask, m (e r) r, 0) >= 0

    with softplus(x) = max(x, 0) + log1p(e): the device's form (csrc/kalman_bodies.h, Pointwise<R, PW_LOGISTIC>), finite at every x.  A subclass validates its
    data and hands in m; where y is missing, m is never looked at."""
    KMODELS = (_lib.KMODEL_LOGISTIC_FIRST, _lib.KMODEL_LOGISTIC_SECOND)

    def __init__(self, ys, size, m0, P0, F, Q, b, order):
        super().__init__(ys, m0, P0, F, Q, b, order)
        self.size = np.asarray(size, np.float64)

    def _terms(self, x):
        """(mask, y, m, e, r) at x (T, dx), the data in x's dtype"""
        e = np.exp(-np.abs(x))
        return np.isfinite(self.yobs), self.yobs.astype(x.dtype), self.size.astype(x.dtype), e, 1.0 / (1.0 + e)

    def log_potential(self, x):
        x = np.asarray(x)
        mask, y, m, e, _ = self._terms(x)
        with np.errstate(invalid="ignore"):
            return float(np.sum(np.where(mask, y * x - m * (np.maximum(x, 0.0) + np.log1p(e)), 0.0)))

    def grad_lam(self, x):
        """(grad, lam) of log g, both (T, dx) and 0 where the observation is missing"""
        x = np.asarray(x)
        mask, y, m, e, r = self._terms(x)
        with np.errstate(invalid="ignore"):
            return np.where(mask, y - m * np.where(x >= 0, r, e * r), 0.0), np.where(mask, m * ((e * r) * r), 0.0)

    def _upload(self, handle, dtype):
        dl = super()._upload(handle, dtype)
        # include/auxssm.h, LOGISTIC_FIRST / _SECOND: the size array (T, dx), laid out as the data is (time stride dx), rides in the cs slot
        buf = dl.bufs["logistic_size"] = handle.to_device(np.ascontiguousarray(self.size, np.float64), dtype)
        dl.c.cs = buf.arr(0, self.dx, 0)
        return dl


class BinomialModel(_LogisticModel):
    """Binomial data with a logit link  y_{t,k} ~ Binomial(trials_{t,k}, sigma(x_{t,k}))  on linear-Gaussian dynamics x_{t+1} = F x_t + b + N(0, Q),
    x_0 ~ N(m0, P0), under the first- or second-order auxiliary observation factories of examples/stochastic_volatility/auxiliary_kalman.py:22-48.  ys (T, dx):
    successes; trials: a scalar, (dx,) or (T, dx), > 0; binary data (spike / no spike, rain / no rain) is trials = 1.  The other arguments are SVModel's.

        log g = where(mask, y x - trials softplus(x), 0)   grad = where(mask, y - trials sigma(x), 0)   lam = -hess = where(mask, trials sigma (1 - sigma), 0)

        dynamics_factory(x)           -> m0, P0, tile(F), tile(Q), tile(b)
        observations_factory(x, u, d) -> order 1: ys = u + d/2 grad, H = I, R = d/2 I, c = 0
                                         order 2: Om = 1 / (lam + 2/d) (diagonal), ys = Om (2u/d + grad + lam x), H = I, R = diag(Om), c = 0
        log_likelihood_fn(x)          -> prior_logpdf(x) + sum log g

    The conventions are PoissonModel's: the constant log C(trials, y) is left out, non-integer values are accepted, a NaN y_{t,k} drops that component's term
    alone (trials may then be anything), and no pseudo-observation is ever NaN.  A finite y outside [0, trials], trials <= 0, or a non-finite trials under a
    finite y raises ValueError.  The potential is concave and evaluated through exp(-|x|), so both orders are defined and finite at every x.

    Pass the three bound methods to kalman.get_kernel: it runs the device sweep (model kind LOGISTIC_FIRST / LOGISTIC_SECOND: the SV sweep's kernels
    instantiated for this potential, every layout and width SVModel has).  The same methods are NumPy factories for the host path and the oracle."""

    def __init__(self, ys, trials, m0, P0, F, Q, b, order=1):
        ys = np.asarray(ys)
        if ys.ndim != 2:
            raise ValueError(f"BinomialModel: ys must be (T, dx), got shape {ys.shape}")
        n = _logistic.binomial_size(ys, trials, "BinomialModel")
        super().__init__(ys, n, m0, P0, F, Q, b, order)
        self.trials = n


class NegBinomialModel(_LogisticModel):
    """Overdispersed counts  y_{t,k} ~ NB(r_{t,k}, p = sigma(x_{t,k})),  pmf proportional to p^y (1 - p)^r: mean r e^x, variance mean (1 + e^x), on
    linear-Gaussian dynamics x_{t+1} = F x_t + b + N(0, Q), x_0 ~ N(m0, P0), under the first- or second-order auxiliary observation factories of
    examples/stochastic_volatility/auxiliary_kalman.py:22-48.  ys (T, dx): counts >= 0; r: a scalar, (dx,) or (T, dx), > 0.  The other arguments are SVModel's.

        log g = where(mask, y x - (y + r) softplus(x), 0)   grad = where(mask, y - (y + r) sigma(x), 0)   lam = -hess = where(mask, (y + r) sigma (1 - sigma), 0)

    and the factories are BinomialModel's with trials = y + r: on the device the two families are one model kind.  The state is the log-odds; the log-mean is
    x + log r, so a log-mean parametrisation (or an exposure) is a shift of the state by log r through m0 and b -- there is no field for it.  The conventions are
    PoissonModel's: the constant log Gamma(y + r) - log Gamma(r) - log y! is left out, non-integer counts are accepted, a finite negative count raises
    ValueError, as does r <= 0 or a non-finite r under a finite y; a NaN y_{t,k} drops that component's term alone; no pseudo-observation is ever NaN.

    Pass the three bound methods to kalman.get_kernel: it runs the device sweep (model kind LOGISTIC_FIRST / LOGISTIC_SECOND).  The same methods are NumPy
    factories for the host path and the oracle."""

    def __init__(self, ys, r, m0, P0, F, Q, b, order=1):
        ys = np.asarray(ys)
        if ys.ndim != 2:
            raise ValueError(f"NegBinomialModel: ys must be (T, dx), got shape {ys.shape}")
        rr = _logistic.negbinomial_r(ys, r, "NegBinomialModel")
        super().__init__(ys, np.asarray(ys, np.float64) + rr, m0, P0, F, Q, b, order)
        self.r = rr


class _LogisticLinearModel(_StateSpaceModel):
    """What BinomialLinearModel and NegBinomialLinearModel share: the logit link behind a loading matrix, PoissonLinearModel's twin.  A latent of dx <= MAX_DX = 4
    components drives dy <= MAX_DY = 1024 channels with a SIZE m_{t,j} = s_j + w_j yy_{t,j} beside the data (binomial: s = trials, w = 0; negative binomial:
    s = r, w = 1).  With mask = isfinite(y), eta_t = H x_t + c, yy = where(mask, y, 0), e = exp(-|eta|), r = 1 / (1 + e), sigma = where(eta >= 0, r, e r) and
    s1 = (e r) r = sigma (1 - sigma) (never a subtraction):

        log g_t = sum_j mask (yy eta - m (max(eta, 0) + log1p(e)))      grad_t = H' (mask (yy - m sigma))  (dx)      Lam_t = H' diag(mask m s1) H = -hess  (dx x dx, PSD)

        dynamics_factory(x)           -> m0, P0, tile(F), tile(Q), tile(b)
        observations_factory(x, u, d) -> order 1: ys = u + d/2 grad,                                            H_obs = I, R = d/2 I, c_obs = 0
                                         order 2: Om = sym((Lam + 2/d I)^-1), ys = Om (2u/d + grad + Lam x),    H_obs = I, R = Om,    c_obs = 0
        log_likelihood_fn(x)          -> prior_logpdf(x) + sum_t log g_t

    These are _LogisticModel's formulas and conventions: the combinatorial constants are left out, non-integers are accepted, a NaN y_{t,j} drops that channel's
    term alone (its size is never looked at), and everything goes through the one exp(-|eta|), so nothing overflows at any eta.  With H = I, c = 0, dy = dx the
    models are BinomialModel / NegBinomialModel.  Lam is PSD, so order 2 is always defined.

    Unlike the Poisson twin's, the curvature is bounded before any sweep: s1 <= 1/4, so Lam_t <= H' diag(m_t / 4) H at every x and
    delta <= 4 / lambda_max(H' diag(m) H) (the largest over t: first_order_delta()) is the a-priori step size of the first order, for which delta lambda_max(Lam_t)
    <= 1 wherever the chain is.  The second order has no such limit.

    The size is per channel: a scalar or (dy,).  A (T, dy) size is refused (NotImplementedError): the factory kernel stages the step's data as an fp64 tile that
    already takes 133 of the 160 KB of LDS, and a second staged tile would not fit beside it.

    Pass the three bound methods to kalman.get_kernel: it runs the device sweep (model kind LOGISTIC_LIN_FIRST / _SECOND: both families are one device kind) on
    host states (T, dx) or (C, T, dx), or on resident DeviceChains(handle, x (C, T, dx), chain_minor=False): the dense layout only.  The same methods are NumPy
    factories for the host path and the oracle."""
    KMODELS = (_lib.KMODEL_LOGISTIC_LIN_FIRST, _lib.KMODEL_LOGISTIC_LIN_SECOND)
    dense_only = True
    MAX_DX = 4
    MAX_DY = 1024

    def __init__(self, who, ys, H, c, s, w, m0, P0, F, Q, b, order):
        super().__init__(ys, m0, P0, F, Q, b, order, dx=H.shape[1])
        self.H, self.c = H, c
        self.size_s, self.size_w = np.asarray(s, np.float64), np.full(self.p_obs, float(w))
        _check_dynamics_shapes(who, self)

    @staticmethod
    def _per_channel(who, name, ys, a):
        """the (T, dy) form refused with its reason, before the shared data rules see the parameter"""
        if np.ndim(a) == 2:
            raise NotImplementedError(f"{who}: {name} must be a scalar or ({np.shape(ys)[1]},), one per channel: a (T, dy) size is not covered -- the factory "
                                      f"kernel stages the step's data as an fp64 tile that already takes 133 of the 160 KB of LDS, and a second staged tile "
                                      f"would not fit beside it")

    @property
    def size(self):
        """m (T, dy) = s + w yy (yy = 0 where y is missing: the size there is never looked at)"""
        return self.size_s + self.size_w * np.where(np.isfinite(self.yobs), self.yobs, 0.0)

    def first_order_delta(self):
        """4 / max_t lambda_max(H' diag(m_t) H): the a-priori step size of the first order (Lam_t <= H' diag(m_t / 4) H at every x)"""
        m = np.where(np.isfinite(self.yobs), self.size, 0.0)
        lam = np.einsum("tj,jk,jl->tkl", m, self.H, self.H)
        return 4.0 / float(np.max(np.linalg.eigvalsh(0.5 * (lam + np.swapaxes(lam, -1, -2)))))

    def _terms(self, x):
        """(mask, eta, yy, m, e, r) at x (T, dx), each (T, dy), m = 0 where y is missing"""
        x = np.asarray(x)
        eta = x @ self.H.astype(x.dtype).T + self.c.astype(x.dtype)
        mask = np.isfinite(self.yobs)
        yy = np.where(mask, self.yobs, 0.0).astype(x.dtype)
        with np.errstate(invalid="ignore"):
            m = np.where(mask, self.size_s.astype(x.dtype) + self.size_w.astype(x.dtype) * yy, 0.0).astype(x.dtype)
        e = np.exp(-np.abs(eta))
        return mask, eta, yy, m, e, 1.0 / (1.0 + e)

    def log_potential(self, x):
        _, eta, yy, m, e, _ = self._terms(x)
        return float(np.sum(yy * eta - m * (np.maximum(eta, 0.0) + np.log1p(e))))

    def grad_lam(self, x):
        """(grad (T, dx), Lam (T, dx, dx)) of log g: H' (yy - m sigma) and H' diag(m sigma (1 - sigma)) H"""
        _, eta, yy, m, e, r = self._terms(x)
        H = self.H.astype(e.dtype)
        lam = np.einsum("tj,jk,jl->tkl", m * ((e * r) * r), H, H)
        return (yy - m * np.where(eta >= 0, r, e * r)) @ H, 0.5 * (lam + np.swapaxes(lam, -1, -2))   # (symmetric to the last bit)

    def _upload(self, handle, dtype):
        dl = super()._upload(handle, dtype)
        # include/auxssm.h, LOGISTIC_LIN_FIRST / _SECOND: the loading matrix (dy, dx) row-major rides in the Hs slot, [c; s; w] (3, dy) in the cs slot
        for name, a in (("Hs", self.H), ("cs", np.stack([self.c, self.size_s, self.size_w]))):
            buf = dl.bufs["llin_" + name] = handle.to_device(np.ascontiguousarray(a, np.float64), dtype)
            setattr(dl.c, name, buf.arr(0, 0, 0))
        return dl


class BinomialLinearModel(_LogisticLinearModel):
    """Binomial channels through a loading matrix: a low-dimensional linear-Gaussian state drives many binary or binomial channels,

        x_0 ~ N(m0, P0),   x_{t+1} = F x_t + b + N(0, Q),   y_{t,j} ~ Binomial(trials_j, sigma(h_j' x_t + c_j)),   j = 1..dy,

    (spike / no-spike bins of many neurons on a few latents, item-response panels, multi-site presence / absence: binary data is trials = 1).  ys (T, dy):
    successes, NaN = missing; trials: a scalar or (dy,), > 0; H (dy, dx) dense and finite; c (dy,) or a scalar; the dynamics arguments are SVModel's;
    1 <= dx <= 4, 1 <= dy <= 1024.  The potential, the factories, the conventions and the a-priori first-order step size delta <= 4 / lambda_max(H' diag(trials) H)
    are _LogisticLinearModel's with m = trials; the data rules are BinomialModel's (a finite y outside [0, trials], trials <= 0 or a (T, dy) trials are refused).
    With H = I, c = 0, dy = dx the model is BinomialModel."""

    def __init__(self, ys, trials, H, c, m0, P0, F, Q, b, order=1):
        who = "BinomialLinearModel"
        ys, H, c = _loading_arguments(who, ys, H, c, order, self.MAX_DX, self.MAX_DY)
        self._per_channel(who, "trials", ys, trials)
        n = _logistic.binomial_size(ys, trials, who)
        super().__init__(who, ys, H, c, n[0], 0.0, m0, P0, F, Q, b, order)
        self.trials = n[0]


class NegBinomialLinearModel(_LogisticLinearModel):
    """Overdispersed counts through a loading matrix:  y_{t,j} ~ NB(r_j, p = sigma(h_j' x_t + c_j)),  mean r_j e^eta and variance mean (1 + e^eta), on the
    dynamics of BinomialLinearModel.  ys (T, dy): counts >= 0, NaN = missing; r: a scalar or (dy,), > 0.  The potential, the factories and the conventions are
    _LogisticLinearModel's with m = y + r (so the a-priori first-order step size is delta <= 4 / max_t lambda_max(H' diag(y_t + r) H)); the data rules are
    NegBinomialModel's (a finite negative count, r <= 0 or a (T, dy) r are refused).  The log-mean of channel j is eta_j + log r_j: a log-mean parametrisation
    or an exposure is a shift of c.  With H = I, c = 0, dy = dx the model is NegBinomialModel."""

    def __init__(self, ys, r, H, c, m0, P0, F, Q, b, order=1):
        who = "NegBinomialLinearModel"
        ys, H, c = _loading_arguments(who, ys, H, c, order, self.MAX_DX, self.MAX_DY)
        self._per_channel(who, "r", ys, r)
        rr = _logistic.negbinomial_r(ys, r, who)
        super().__init__(who, ys, H, c, rr[0], 1.0, m0, P0, F, Q, b, order)
        self.r = rr[0]


class LorenzModel(_BuiltinModel):
    """Stochastic Lorenz-63 with Euler-Maruyama dynamics and sparse linear-Gaussian observations,
    examples/lorenz/auxiliary_kalman.py:14-52 (model.py:10-25; linearisation.py:11-44 with the analytic Jacobian in place of jacfwd):

        dynamics_factory(x)           -> m0, P0, F_t = I + dt J(x_t), tile(Q), b_t = mean(x_t) - F_t x_t       (:27-29)
        observations_factory(x, u, d) -> ys = [u; y], Hs = [I; H], Rs = blkdiag(d/2 I, R), cs = [0; c]        (:31-36)
        log_likelihood_fn(x)          -> log N(x_0; m0, P0) + sum log N(x_{t+1}; mean(x_t), Q) + nansum_t log N(y_t; H_t x_t + c_t, R_t)

    ys (T, po) with NaN rows where nothing is observed; Hs (T, po, 3) may carry NaN rows there too (model.py:43-56).
    Pass the three bound methods to kalman.get_kernel: it runs the device sweep (model kind LORENZ63_EXT)."""
    kmodel = _lib.KMODEL_LORENZ63_EXT

    def __init__(self, ys, Hs, Rs, cs, m0, P0, theta, sigma_x, dt):
        self.yobs, self.Hobs, self.Robs, self.cobs = np.asarray(ys), np.asarray(Hs), np.asarray(Rs), np.asarray(cs)
        self.T, self.p_obs = self.yobs.shape
        self.dx = 3
        self.m0, self.P0 = np.asarray(m0, np.float64), np.asarray(P0, np.float64)
        # theta (3,): one parameter vector for all chains; (C, 3): one per chain (the Gibbs sampler over (x, theta), loop.LorenzThetaStep).
        # The NumPy methods below (host path / oracle) use chain 0's.
        self.theta_rows = np.asarray(theta, np.float64).reshape(-1, 3)
        self.theta = self.theta_rows[0].copy()
        self.sigma_x, self.dt = float(sigma_x), float(dt)
        self.Q = self.dt * self.sigma_x ** 2 * np.eye(3)
        self.Qs = np.broadcast_to(self.Q, (self.T - 1, 3, 3))
        self._dev = {}

    def mean(self, x):
        x = np.asarray(x)
        th, dt = self.theta, self.dt
        x1, x2, x3 = x[..., 0], x[..., 1], x[..., 2]
        return x + dt * np.stack([th[0] * (x2 - x1), th[1] * x1 - x2 - x1 * x3, x1 * x2 - th[2] * x3], axis=-1)

    def dynamics_factory(self, x):
        x = np.asarray(x)
        xl = x[:-1]
        th, dt = self.theta, self.dt
        n = xl.shape[0]
        J = np.zeros((n, 3, 3), x.dtype)
        J[:, 0, 0], J[:, 0, 1] = -th[0], th[0]
        J[:, 1, 0], J[:, 1, 1], J[:, 1, 2] = th[1] - xl[:, 2], -1.0, -xl[:, 0]
        J[:, 2, 0], J[:, 2, 1], J[:, 2, 2] = xl[:, 1], xl[:, 0], -th[2]
        Fs = np.eye(3, dtype=x.dtype) + dt * J
        bs = self.mean(xl) - np.einsum("tij,tj->ti", Fs, xl)
        return self.m0.astype(x.dtype), self.P0.astype(x.dtype), Fs, self.Qs.astype(x.dtype), bs

    def observations_factory(self, x, u, delta):
        return LGConcatModel.observations_factory(self, x, u, delta)

    def log_likelihood_fn(self, x):
        """NumPy (host path / oracle): the same nansum-over-steps semantics as the reference (:38-46)."""
        x = np.asarray(x, np.float64)

        def mvn(r, cov):
            L = np.linalg.cholesky(cov)
            z = np.linalg.solve(L, r[..., None])[..., 0]
            return -0.5 * np.sum(z * z, -1) - np.sum(np.log(np.diagonal(L, axis1=-2, axis2=-1)), -1) - 0.5 * r.shape[-1] * np.log(2 * np.pi)

        out = mvn(x[0] - self.m0, self.P0)
        out += np.sum(mvn(x[1:] - self.mean(x[:-1]), self.Q))
        with np.errstate(all="ignore"):
            pred = np.einsum("tij,tj->ti", self.Hobs, x) + self.cobs
            ll = mvn(np.asarray(self.yobs, np.float64) - pred, np.asarray(self.Robs, np.float64))
        return float(out + np.nansum(ll))

    def _upload(self, handle, dtype):
        # rides in the Fs slot of the C struct (include/auxssm.h, LORENZ63_EXT): rows [theta1, theta2, theta3, dt]
        par = np.concatenate([self.theta_rows, np.full((self.theta_rows.shape[0], 1), self.dt)], axis=1)
        n = self.T - 1
        lg = (self.m0, self.P0, np.broadcast_to(np.eye(3), (n, 3, 3)), self.Qs, np.broadcast_to(np.zeros(3), (n, 3)),
              self.Hobs, self.Robs, self.cobs)
        dl = DeviceLGSSM(handle, lg, 1, self.T, 1, 3, self.p_obs, False, dtype)
        pbuf = handle.to_device(par, dtype)
        dl.bufs["lorenz_par"] = pbuf
        dl.c.Fs = pbuf.arr(4 if par.shape[0] > 1 else 0, 0, 0)
        return dl

    def par_device(self, handle, dtype, C):
        """the device rows [theta, dt] the sweep reads, one per chain (C, 4): a single theta is replicated on first use, so that a theta
        step can then write each chain's own"""
        dl = self.device(handle, dtype)[0]
        pbuf = dl.bufs["lorenz_par"]
        if pbuf.shape[0] != C:
            if pbuf.shape[0] != 1:
                raise ValueError(f"the model holds {pbuf.shape[0]} theta rows, the chains are {C}")
            pbuf = dl.bufs["lorenz_par"] = handle.to_device(np.repeat(pbuf.to_host(), C, axis=0), dtype)
            dl.c.Fs = pbuf.arr(4 if C > 1 else 0, 0, 0)
        return pbuf


class _DeviceModel:
    """the C struct of a device model whose arrays do not have the LGSSM's shapes, with the buffers it points at"""

    def __init__(self):
        self.c = _lib.Lgssm()
        self.bufs = {}


class MVTModel(_BuiltinModel):
    """The spatial example's batched model (examples/spatial/auxiliary_kalman.py:10-66, model.py:103-124): d independent scalar LGSSMs
    x_{t+1,k} = F_k x_{t,k} + b_k + N(0, Q_k), x_{0,k} ~ N(m0_k, P0_k), coupled only through the multivariate Student-t potential
    log g_t(x) = -(nu + d) / 2 log(1 + (y_t - x)^T prec (y_t - x) / nu) (NaN -> 0), in the reference's batched shapes: the state is (T, d, 1),

        dynamics_factory(x)           -> m0 (d, 1), P0 (d, 1, 1), tile(F), tile(Q) (T - 1, d, 1, 1), tile(b) (T - 1, d, 1)                    (:24-28)
        observations_factory(x, u, d) -> order 1: ys = u + d/2 nan_to_num(grad(x)), H = 1, R = d/2, c = 0                                       (:30-38)
                                         order 2: h = -nu diag(prec) / (nu - 2), Om = 1 / (-h + 2/d), ys = Om (2u/d + grad - h x), R = Om       (:40-48)
        log_likelihood_fn(x)          -> sum_k [log N(x_0k; m0_k, P0_k) + sum_t log N(x_tk; F_k x_{t-1,k} + b_k, Q_k)] + sum_t log g_t(x_t)      (:50-54)

    with the closed-form gradient grad_x log g_t = (nu + d) prec (y_t - x_t) / (nu + q_t), q_t = (y_t - x_t)^T prec (y_t - x_t), in place of jax.grad.
    ys (T, d) (a NaN anywhere in y_t makes the step's potential flat); m0, b (d,) or (d, 1); P0, F, Q (d,) or (d, 1, 1); prec dense (d, d), symmetric positive
    definite; nu > 0 (order 2: nu != 2); 1 <= d <= 64.  Pass the three bound methods to kalman.get_kernel: it runs the device sweep (model kind MVT_FIRST /
    MVT_SECOND, csrc/kalman_mvt.hip: C * d scalar recursions) on host states of shape (T, d, 1), (T, d), either with a leading chain axis, or on resident
    DeviceChains(handle, x (C, T, d), chain_minor=False).  Order 2 needs -h_k + 2/delta > 0 for every component: checked for a host step size (ValueError), a
    precondition for a device-resident one.  The same methods are NumPy factories for the host path and the oracle."""
    dense_only = True
    batched_state = True  # the reference's state carries a trailing axis of 1 (kalman.generic strips and restores it around the device sweep)
    MAX_D = 64

    def __init__(self, ys, m0, P0, F, Q, b, nu, prec, order=1):
        if order not in (1, 2):
            raise ValueError("order must be 1 or 2")
        self.yobs = np.asarray(ys)
        if self.yobs.ndim != 2:
            raise ValueError(f"MVTModel: ys must be (T, d), got shape {self.yobs.shape}")
        self.T, self.dx = self.yobs.shape
        d = self.dx
        if not 1 <= d <= self.MAX_D:
            raise ValueError(f"MVTModel: d = {d}: the batched sweep covers 1 <= d <= {self.MAX_D}")
        if not (np.ndim(nu) == 0 and np.isfinite(float(nu)) and float(nu) > 0):
            raise ValueError(f"MVTModel: nu must be a finite scalar > 0 (got {nu!r})")
        if order == 2 and float(nu) == 2.0:
            raise ValueError("MVTModel: order=2 divides by nu - 2: nu == 2 is refused")
        P = np.asarray(prec, np.float64)
        if P.ndim != 2 or P.shape != (d, d):
            raise ValueError(f"MVTModel: prec must be a dense ({d}, {d}) matrix (got shape {np.shape(prec)})")
        if not np.all(np.isfinite(P)) or np.max(np.abs(P - P.T)) > 1e-12 * np.max(np.abs(P)):
            raise ValueError("MVTModel: prec must be finite and symmetric (to 1e-12 relative)")
        try:
            np.linalg.cholesky(P)
        except np.linalg.LinAlgError:
            raise ValueError("MVTModel: prec must be positive definite") from None

        def diag(a, name, shapes):
            a = np.asarray(a, np.float64)
            if a.shape not in shapes:
                raise ValueError(f"MVTModel: {name} must have shape {' or '.join(map(str, shapes))}, got {a.shape}")
            return a.reshape(d)

        self.p_obs = d
        self.nu, self.prec, self.order = float(nu), 0.5 * (P + P.T), order
        self.m0v, self.bv = diag(m0, "m0", ((d,), (d, 1))), diag(b, "b", ((d,), (d, 1)))
        self.P0v, self.Fv, self.Qv = (diag(a, n, ((d,), (d, 1, 1))) for a, n in ((P0, "P0"), (F, "F"), (Q, "Q")))
        if np.any(self.P0v <= 0) or np.any(self.Qv <= 0):
            raise ValueError("MVTModel: P0 and Q must be positive")
        self.hess_diag = -self.nu * np.diagonal(self.prec) / (self.nu - 2.0) if order == 2 else np.zeros(d)
        self.kmodel = _lib.KMODEL_MVT_FIRST if order == 1 else _lib.KMODEL_MVT_SECOND
        self._dev = {}

    def check_delta(self, delta):
        """order 2: Omega_k^-1 = -h_k + 2/delta must be positive for every component (it is a variance's inverse)"""
        if self.order == 2 and not np.all(2.0 / float(delta) + (-self.hess_diag) > 0):
            raise ValueError(f"MVTModel: order=2 needs 2/delta + nu prec_kk / (nu - 2) > 0 for every component: delta = {float(delta)!r} gives "
                             f"min {float(np.min(2.0 / float(delta) - self.hess_diag)):.3g}")

    # ---- the potential (t_distribution.py:98-104, model.py:116-124) and its gradient ----
    def _rz(self, x):
        x = np.asarray(x)
        x = x.reshape(-1, self.dx)
        r = self.yobs.astype(x.dtype) - x
        return r, r @ self.prec.astype(x.dtype).T

    def log_potential(self, x):
        """sum_t nan_to_num(log g_t(x_t)), x (T, d) or (T, d, 1)"""
        r, z = self._rz(x)
        with np.errstate(all="ignore"):
            q = np.sum(z * r, -1)
            val = -(0.5 * (self.nu + self.dx)) * np.log1p(q / self.nu)
        return float(np.sum(np.nan_to_num(val)))

    def grad_log_potential(self, x):
        """(T, d): (nu + d) prec (y_t - x_t) / (nu + q_t); NaN where y_t has a NaN (the factories decide what to do with it)"""
        r, z = self._rz(x)
        with np.errstate(all="ignore"):
            q = np.sum(z * r, -1, keepdims=True)
            return (self.nu + self.dx) * z / (self.nu + q)

    # ---- NumPy factories in the reference's batched shapes ----
    def dynamics_factory(self, x):
        dt = np.asarray(x).dtype
        T, d = self.T, self.dx
        Fs = np.tile(self.Fv.astype(dt).reshape(1, d, 1, 1), (T - 1, 1, 1, 1))
        Qs = np.tile(self.Qv.astype(dt).reshape(1, d, 1, 1), (T - 1, 1, 1, 1))
        bs = np.tile(self.bv.astype(dt).reshape(1, d, 1), (T - 1, 1, 1))
        return self.m0v.astype(dt).reshape(d, 1), self.P0v.astype(dt).reshape(d, 1, 1), Fs, Qs, bs

    def observations_factory(self, x, u, delta):
        x, u = np.asarray(x), np.asarray(u)
        T, d = self.T, self.dx
        dt = u.dtype
        x, u = x.reshape(T, d, 1), u.reshape(T, d, 1)
        eyes, zeros = np.ones((T, d, 1, 1), dt), np.zeros((T, d, 1), dt)
        grad = self.grad_log_potential(x).reshape(T, d, 1)
        with np.errstate(all="ignore"):
            if self.order == 1:
                grad = np.nan_to_num(grad)
                return (u + 0.5 * delta * grad).astype(dt), eyes, (0.5 * delta * eyes).astype(dt), zeros
            h = self.hess_diag.astype(dt)
            om = 1.0 / (-h[None, :, None, None] + 2 * eyes / delta)
            ys = om[..., 0] * (2 * u / delta + grad - h[None, :, None] * x)
        return ys.astype(dt), eyes, om.astype(dt), zeros

    def log_likelihood_fn(self, x):
        x = np.asarray(x)
        x = x.reshape(self.T, self.dx)

        def norm(v, loc, var):
            return -0.5 * (v - loc) ** 2 / var - 0.5 * np.log(var) - 0.5 * np.log(2 * np.pi)

        with np.errstate(all="ignore"):
            out = np.nansum(norm(x[0], self.m0v, self.P0v))
            out += np.nansum(norm(x[1:], self.Fv * x[:-1] + self.bv, self.Qv))
        return float(out) + self.log_potential(x)

    # ---- device side ----
    def _upload(self, handle, dtype):
        dl = _DeviceModel()
        # include/auxssm.h, MVT_FIRST / MVT_SECOND: the diagonal model as (d) vectors; prec rides in the Rs slot, [nu] in the cs slot
        for name, a in (("m0", self.m0v), ("P0", self.P0v), ("Fs", self.Fv), ("Qs", self.Qv), ("bs", self.bv), ("Rs", self.prec), ("cs", [self.nu])):
            buf = dl.bufs[name] = handle.to_device(np.asarray(a, np.float64), dtype)
            setattr(dl.c, name, buf.arr(0, 0, 0))
        return dl
