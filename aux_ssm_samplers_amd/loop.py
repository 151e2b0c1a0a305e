"""The MCMC loop around the sweeps, on the device (reference: `loop` of examples/stochastic_volatility/experiment.py:88-128 and
examples/lorenz/experiment.py:120-169; `gibbs_step` :106-115; `theta_posterior_mean_and_chol` examples/lorenz/model.py:59-79).

    loop(key, init_delta, init_state, kernel_fn, delta_fn, n_iter, ...) ->
        (n_iter, (sq_jump, mean, sq_mean), state, delta, window_avg_acceptance, avg_acceptance)

same argument order and return order as the reference.  The chains stay resident in HBM (`state.x` a kalman.DeviceChains or a
csmc.CsmcChains); per sweep the loop enqueues: the sweep, the running squared-jump / first / second moments (folded into the Kalman
sweep's accept step, a separate pass for cSMC), the acceptance averages and, while adapting, the step-size rule -- all HIP kernels on
the handle's stream (include/auxssm.h, "the MCMC loop around the sweeps").  A sampling run (delta_fn None) never synchronises with
the host.  While adapting with the reference's rule the Kalman step size is a device scalar as well (auxssm_kalman_sweep_dd): no read-back per sweep;
a user-supplied rule runs on the host and reads the C windowed acceptances back each burn-in sweep.

Chains of one call share delta: the adaptation rule sees the chain-mean of the windowed acceptance (one chain: the reference exactly).
"""
import functools

import numpy as np

from . import _lib, random as _random
from .common import delta_adaptation


def _is_reference_rule(delta_fn):
    """-> (min_delta, max_delta) if delta_fn is common.delta_adaptation (or a functools.partial of it fixing only the bounds)"""
    if delta_fn is delta_adaptation:
        return 1e-20, 1e20
    if isinstance(delta_fn, functools.partial) and delta_fn.func is delta_adaptation and not delta_fn.args and \
            set(delta_fn.keywords) <= {"min_delta", "max_delta"}:
        return delta_fn.keywords.get("min_delta", 1e-20), delta_fn.keywords.get("max_delta", 1e20)
    return None


class LorenzThetaStep:
    """theta | x of the stochastic Lorenz-63 Gibbs sampler (experiment.py:106-115), one theta per chain, drawn and written on the device
    into the parameter rows the LORENZ63_EXT sweep reads (`model` a kalman.LorenzModel built with theta of shape (C, 3))."""

    def __init__(self, model, sigma_theta):
        self.model, self.sigma_theta = model, float(sigma_theta)
        self._eps = None

    def __call__(self, key, chains):
        from .kalman.generic import DeviceChains
        if not isinstance(chains, DeviceChains):
            raise ValueError("LorenzThetaStep: the step writes the parameter rows of the Kalman sampler's LORENZ63_EXT sweep; it needs kalman.DeviceChains")
        handle = chains.handle
        par = self.model.par_device(handle, chains.dtype, chains.C)
        if self._eps is None or self._eps.handle is not handle or self._eps.shape != (chains.C, 3) or self._eps.dtype != chains.dtype:
            self._eps = handle.empty((chains.C, 3), chains.dtype)
        if _random.compat() == "jax":   # examples/lorenz/experiment.py:115: jax.random.normal(key_theta, (3,)) -- one key per chain (`key` (C, 2) or split(key, C))
            kk = np.asarray(key, np.uint32)
            keys = kk if kk.ndim == 2 else (_random.as_key(key)[None] if chains.C == 1 else _random.jax_split(_random.as_key(key), chains.C))
            self._eps.copy_from_host(_random.jax_normal(keys, (3,), chains.dtype, handle))
        else:
            handle.rng_normal_into(key, 0, self._eps)
        handle.lorenz_theta_update(chains.x, self.sigma_theta, self.model.sigma_x, self._eps, par, layout=chains.layout)

    def theta(self, chains):
        return self.model.par_device(chains.handle, chains.dtype, chains.C).to_host()[:, :3]


class MNIWPrior:
    """The conjugate prior of linear-Gaussian dynamics x_{t+1} = F x_t + b + N(0, Q), with A = [F b] (d, d + 1):
        Q ~ IW(nu0, Psi0),   A | Q ~ MN(M0, Q, K0^-1)
    M0 (d, d + 1), K0 (d + 1, d + 1) symmetric positive definite (a precision: the rows of A have covariance K0^-1 up to Q), nu0 > d - 1, Psi0 (d, d)
    symmetric positive definite.  Validated here, so that a DynamicsThetaStep never meets an inadmissible prior on the device."""

    def __init__(self, M0, K0, nu0, Psi0):
        M0, K0, Psi0 = (np.array(a, np.float64, ndmin=2) for a in (M0, K0, Psi0))
        d = Psi0.shape[0]
        if Psi0.shape != (d, d) or M0.shape != (d, d + 1) or K0.shape != (d + 1, d + 1):
            raise ValueError(f"MNIWPrior: need M0 (d, d + 1), K0 (d + 1, d + 1), Psi0 (d, d); got {M0.shape}, {K0.shape}, {Psi0.shape}")
        nu0 = float(nu0)
        if not (np.all(np.isfinite(M0)) and np.all(np.isfinite(K0)) and np.all(np.isfinite(Psi0)) and np.isfinite(nu0)):
            raise ValueError("MNIWPrior: M0, K0, nu0 and Psi0 must be finite")
        if not nu0 > d - 1:
            raise ValueError(f"MNIWPrior: nu0 must exceed d - 1 = {d - 1} (got {nu0})")
        for name, a in (("K0", K0), ("Psi0", Psi0)):
            dg = np.abs(np.diag(a))
            if not np.all(np.abs(a - a.T) <= 1e-12 * (dg[:, None] + dg[None, :])):
                raise ValueError(f"MNIWPrior: {name} must be symmetric")
            try:
                np.linalg.cholesky(0.5 * (a + a.T))
            except np.linalg.LinAlgError:
                raise ValueError(f"MNIWPrior: {name} must be positive definite") from None
        self.d, self.M0, self.K0, self.nu0, self.Psi0 = d, M0, 0.5 * (K0 + K0.T), nu0, 0.5 * (Psi0 + Psi0.T)

    def struct(self, chi_scale=2.0):
        """-> _lib.MniwPrior (auxssm_mniw_prior); chi_scale 2: the chi buffer holds Gamma((nu_n - i) / 2, 1) draws"""
        if self.d > 4:
            raise ValueError(f"the device step covers dx <= 4 (this prior has d = {self.d})")
        p = _lib.MniwPrior()
        for name in ("M0", "K0", "Psi0"):
            flat = getattr(self, name).ravel()
            arr = getattr(p, name)
            for k, v in enumerate(flat):
                arr[k] = float(v)
        p.nu0, p.chi_scale = self.nu0, float(chi_scale)
        return p


def _time_invariant(a):
    a = np.asarray(a)
    return a.shape[0] <= 1 or a.strides[0] == 0 or bool(np.all(a == a[:1]))


class DynamicsThetaStep:
    """(F, b, Q) | x for the linear-Gaussian dynamics of a Kalman-sampler model: one conjugate matrix-normal inverse-Wishart draw per chain and sweep, on the
    device (auxssm_dynamics_theta_update), written into per-chain parameter buffers the next sweep reads:

        step = DynamicsThetaStep(model, MNIWPrior(M0, K0, nu0, Psi0));   loop(key, delta, state, kernel, None, n_iter, theta_step=step)

    model: LGConcatModel, SVModel, PoissonModel, BinomialModel, NegBinomialModel, PoissonLinearModel, BinomialLinearModel or NegBinomialLinearModel with
    time-invariant Fs / Qs / bs (a broadcast view, or equal rows) and dx <= 4.  On its first call the step replaces the device model's Fs, Qs, bs with per-chain
    buffers (C, d, d), (C, d, d), (C, d) of time stride 0 that start as copies of the model's values (LorenzModel.par_device's pattern); from then on the model
    serves chains of that count only (a sweep with another count is refused, kalman/generic.py::_check_per_chain_dynamics).  With per-chain parameters an LGConcatModel leaves the fused chain-shared sweep (and its memoised model stage) for the general
    path.  x_0's prior (m0, P0) takes no part and stationarity is not imposed.  Every call: the key is split in three, chi <- auxssm_rng_gamma at shapes
    (nu_n - i) / 2 (the update doubles them to chi-squares), the two normal buffers are filled, the update runs on chains.x in chains.layout; no host synchronisation.
    A chain whose posterior cannot be factorised keeps its parameters and raises its flag (flags(chains)).
    Keys: the call's key is split by random.split, which is jax.random.split under random.set_compat("jax") -- as loop() splits its own; the three fills are the
    package's Threefry streams in either mode (the reference has no such step, so there are no jax.random draws to reproduce).

    Particle Gibbs: model may instead be the csmc.LinearGaussianDynamics of a conditional-SMC kernel (time-invariant, dx <= 4) -- the step then serves
    csmc.CsmcChains, and loop(..., theta_step=step) alternates x | theta, y by cSMC with theta | x by this draw:

        Mt = csmc.LinearGaussianDynamics(F, b, Q);   init, kernel = csmc.get_independent_kernel(M0, G0, Mt, Gt, N=..., backward=True, Pt=Mt)
        step = DynamicsThetaStep(Mt, MNIWPrior(M0, K0, nu0, Psi0));   loop(key, delta, state, kernel, None, n_iter, theta_step=step)

    On its first call it attaches per-chain buffers to the chains (chains.dynamics, a csmc._device.ChainDynamics: the live F, b, Q, chol_Q, staging copies and
    flags, all starting from the model's values); from then on the sequential sweep reads chain c's own transition (auxssm_csmc_sweep_chain_dynamics; kernels that
    cannot -- guided, parallel in time, user programs, dx > 4 -- refuse such chains).  Every call: the same three key splits and fills, the update on chains.x into
    the STAGING buffers, then auxssm_csmc_dynamics_commit, which factors each chain's new Q as rounded to the chains' dtype and moves the whole quadruple into the live
    buffers, or leaves it and raises the chain's flag (1 - 4 the update's codes, 5: Q is not positive definite once rounded).  No host synchronisation."""

    def __init__(self, model, prior):
        from .kalman import models as M
        from .csmc import models as CM
        self._csmc = isinstance(model, (CM.LinearGaussianDynamics, CM.Lorenz63Dynamics, CM.DeviceGaussianDynamics))
        if self._csmc:
            self._init_csmc(model, prior)
            return
        who = type(model).__name__
        if isinstance(model, M.LorenzModel):
            raise ValueError("DynamicsThetaStep: LorenzModel is parameterised by its drift (theta, dt), not by (F, b, Q): use LorenzThetaStep")
        if isinstance(model, M.MVTModel):
            raise ValueError("DynamicsThetaStep: MVTModel holds d independent scalar dynamics (diagonal F, Q): a dense (F, b, Q) draw would leave its "
                             "parameterisation")
        if not isinstance(model, (M.LGConcatModel, M._StateSpaceModel)):
            raise ValueError(f"DynamicsThetaStep: {who} is not a model with linear-Gaussian dynamics (Fs, Qs, bs) the Kalman sampler runs on the device")
        if not isinstance(prior, MNIWPrior):
            raise ValueError("DynamicsThetaStep: prior must be an MNIWPrior")
        if model.dx > 4:
            raise ValueError(f"DynamicsThetaStep: the device step covers dx <= 4 (the model has dx = {model.dx})")
        if prior.d != model.dx:
            raise ValueError(f"DynamicsThetaStep: the prior is for d = {prior.d}, the model has dx = {model.dx}")
        if model.T < 2:
            raise ValueError("DynamicsThetaStep: the model has no transition (T < 2)")
        for name in ("Fs", "Qs", "bs"):
            if not _time_invariant(getattr(model, name)):
                raise ValueError(f"DynamicsThetaStep: the model's {name} varies in time; the step draws ONE (F, b, Q) per chain")
        self.model, self.prior = model, prior
        self._prior_c = prior.struct(2.0)
        self._shapes = [0.5 * (prior.nu0 + model.T - 1 - i) for i in range(model.dx)]
        self._work = {}

    def _init_csmc(self, model, prior):
        from .csmc import models as CM
        if isinstance(model, CM.Lorenz63Dynamics):
            raise ValueError("DynamicsThetaStep: Lorenz63Dynamics is parameterised by its drift (theta, dt), not by (F, b, Q): there is nothing for the step to draw")
        if isinstance(model, CM.DeviceGaussianDynamics):
            raise ValueError("DynamicsThetaStep: DeviceGaussianDynamics has a user-defined transition mean (device code), not (F, b): the step covers "
                             "csmc.LinearGaussianDynamics")
        if not isinstance(prior, MNIWPrior):
            raise ValueError("DynamicsThetaStep: prior must be an MNIWPrior")
        if model.time_varying:
            raise ValueError("DynamicsThetaStep: the LinearGaussianDynamics varies in time (F is (T - 1, d, d)); the step draws ONE (F, b, Q) per chain")
        F, Q = (np.atleast_2d(np.asarray(a, np.float64)) for a in (model.F, model.Q))
        d = F.shape[0]
        if d > 4:
            raise ValueError(f"DynamicsThetaStep: per-chain dynamics run the cSMC kernels of dx <= 4 (the model has dx = {d})")
        if F.shape != (d, d) or Q.shape != (d, d) or np.size(model.b) != d:
            raise ValueError(f"DynamicsThetaStep: need F (d, d), b (d,), Q (d, d); got {F.shape}, {np.shape(model.b)}, {Q.shape}")
        if prior.d != d:
            raise ValueError(f"DynamicsThetaStep: the prior is for d = {prior.d}, the model has dx = {d}")
        self.model, self.prior, self.dx = model, prior, d
        self._prior_c = prior.struct(2.0)
        self._work = {}

    def _dynamics(self, chains):
        """-> the chains' ChainDynamics, attached (from the model's F, b, Q) on first use"""
        from .csmc._device import ChainDynamics
        if chains.dynamics is None:
            chains.dynamics = ChainDynamics(chains.handle, chains.dtype, chains.C, self.model.F, self.model.b, self.model.Q)
        dyn = chains.dynamics
        if (dyn.C, dyn.dx) != (chains.C, self.dx):
            raise ValueError(f"DynamicsThetaStep: the chains hold per-chain parameters of {dyn.C} chains of dx = {dyn.dx}, the step is for {chains.C} of dx = {self.dx}")
        return dyn

    def _call_csmc(self, key, chains):
        handle, dtype, Cn, d = chains.handle, chains.dtype, chains.C, self.dx
        dyn = self._dynamics(chains)
        wk = (id(handle), np.dtype(dtype).str, Cn)
        work = self._work.get(wk)
        if work is None:
            self._work.clear()
            work = self._work[wk] = (handle.empty((Cn, d), dtype), handle.empty((Cn, d, d), dtype), handle.empty((Cn, d, d + 1), dtype))
        chi, eps_w, eps_a = work
        k_chi, k_w, k_a = _random.split(key, 3)
        handle.rng_gamma_into(k_chi, 0, [0.5 * (self.prior.nu0 + chains.T - 1 - i) for i in range(d)], chi)
        handle.rng_normal_into(k_w, 0, eps_w)
        handle.rng_normal_into(k_a, 0, eps_a)
        sc = 1 if Cn > 1 else 0
        handle.dynamics_theta_update(chains.x, self._prior_c, chi, eps_w, eps_a, dyn.F_new.arr(sc * d * d, 0, 0), dyn.b_new.arr(sc * d, 0, 0),
                                     dyn.Q_new.arr(sc * d * d, 0, 0), dyn.step_flags)
        dyn.commit()

    # ---- the model's per-chain parameter buffers ----
    def _params(self, handle, dtype, C):
        """-> (F (C, d, d), b (C, d), Q (C, d, d)) DeviceArrays the device model points at, made per-chain on first use"""
        dl = self.model.device(handle, dtype)[0]
        d = self.model.dx
        own = dl.bufs.get("dynamics_theta")
        if own is None:
            host = [np.repeat(np.asarray(getattr(self.model, n))[:1], C, axis=0) for n in ("Fs", "bs", "Qs")]
            own = dl.bufs["dynamics_theta"] = tuple(handle.to_device(a, dtype) for a in host)
            F, b, Q = own
            sc = 1 if C > 1 else 0
            dl.c.Fs, dl.c.bs, dl.c.Qs = F.arr(sc * d * d, 0, 0), b.arr(sc * d, 0, 0), Q.arr(sc * d * d, 0, 0)
            dl.bufs["Fs"], dl.bufs["bs"], dl.bufs["Qs"] = F, b, Q
        if own[0].shape[0] != C:
            raise ValueError(f"DynamicsThetaStep: the model holds per-chain parameters of {own[0].shape[0]} chains, the chains are {C}")
        return own

    def _check_chains(self, chains):
        from .kalman.generic import DeviceChains
        if self._csmc:
            from .csmc._device import CsmcChains
            if not isinstance(chains, CsmcChains):
                raise ValueError("DynamicsThetaStep: the step was built on a csmc.LinearGaussianDynamics and needs csmc.CsmcChains; for kalman.DeviceChains build "
                                 "it on the Kalman-sampler model")
            if chains.dx != self.dx:
                raise ValueError(f"DynamicsThetaStep: the chains have dx = {chains.dx}, the model {self.dx}")
            if chains.T < 2:
                raise ValueError("DynamicsThetaStep: the chains have no transition (T < 2)")
            return
        if not isinstance(chains, DeviceChains):
            raise ValueError("DynamicsThetaStep: cSMC chains carry their transition parameters in the Feynman-Kac model; the step needs kalman.DeviceChains "
                             "(for csmc.CsmcChains build it on the kernel's csmc.LinearGaussianDynamics)")
        if (chains.T, chains.dx) != (self.model.T, self.model.dx):
            raise ValueError(f"DynamicsThetaStep: the chains are (T, dx) = ({chains.T}, {chains.dx}), the model ({self.model.T}, {self.model.dx})")

    def __call__(self, key, chains):
        self._check_chains(chains)
        if self._csmc:
            return self._call_csmc(key, chains)
        handle, dtype, Cn, d = chains.handle, chains.dtype, chains.C, self.model.dx
        F, b, Q = self._params(handle, dtype, Cn)
        wk = (id(handle), np.dtype(dtype).str, Cn)
        work = self._work.get(wk)
        if work is None:
            self._work.clear()
            work = self._work[wk] = (handle.empty((Cn, d), dtype), handle.empty((Cn, d, d), dtype), handle.empty((Cn, d, d + 1), dtype),
                                     handle.zeros((Cn,), np.int32))
        chi, eps_w, eps_a, flags = work
        chains.disable_fused()   # per-chain parameters: the fused chain-shared sweep no longer applies
        k_chi, k_w, k_a = _random.split(key, 3)
        handle.rng_gamma_into(k_chi, 0, self._shapes, chi)
        handle.rng_normal_into(k_w, 0, eps_w)
        handle.rng_normal_into(k_a, 0, eps_a)
        sc = 1 if Cn > 1 else 0
        handle.dynamics_theta_update(chains.x, self._prior_c, chi, eps_w, eps_a, F.arr(sc * d * d, 0, 0), b.arr(sc * d, 0, 0), Q.arr(sc * d * d, 0, 0), flags,
                                     layout=chains.layout)

    def params(self, chains):
        """-> (F (C, d, d), b (C, d), Q (C, d, d)) as host arrays (synchronises)"""
        self._check_chains(chains)
        if self._csmc:
            dyn = self._dynamics(chains)
            return dyn.F.to_host(), dyn.b.to_host(), dyn.Q.to_host()
        F, b, Q = self._params(chains.handle, chains.dtype, chains.C)
        return F.to_host(), b.to_host(), Q.to_host()

    def flags(self, chains):
        """-> (C,) int32: 0, or why the last call left chain c unchanged (include/auxssm.h: auxssm_dynamics_theta_update; cSMC chains: auxssm_csmc_dynamics_commit,
        which adds 5 -- Q not positive definite once rounded to the chains' dtype)"""
        if self._csmc:
            return chains.dynamics.flags.to_host() if getattr(chains, "dynamics", None) is not None else np.zeros(chains.C, np.int32)
        work = self._work.get((id(chains.handle), np.dtype(chains.dtype).str, chains.C))
        return work[3].to_host() if work is not None else np.zeros(chains.C, np.int32)


class ObsMNIWPrior:
    """The conjugate prior of a linear-Gaussian observation model y_t = H x_t + c + N(0, R), with A = [H c] (dy, dx + 1):
        R ~ IW(nu0, Psi0),   A | R ~ MN(M0, R, K0^-1)
    M0 (dy, dx + 1), K0 (dx + 1, dx + 1) symmetric positive definite (a precision: the rows of A have covariance K0^-1 up to R), nu0 > dy - 1, Psi0 (dy, dy)
    symmetric positive definite.  Validated here as MNIWPrior validates its own, so that an ObservationThetaStep never meets an inadmissible prior on the device."""

    def __init__(self, M0, K0, nu0, Psi0):
        M0, K0, Psi0 = (np.array(a, np.float64, ndmin=2) for a in (M0, K0, Psi0))
        dy, n = Psi0.shape[0], K0.shape[0]
        if Psi0.shape != (dy, dy) or K0.shape != (n, n) or n < 2 or M0.shape != (dy, n):
            raise ValueError(f"ObsMNIWPrior: need M0 (dy, dx + 1), K0 (dx + 1, dx + 1), Psi0 (dy, dy); got {M0.shape}, {K0.shape}, {Psi0.shape}")
        nu0 = float(nu0)
        if not (np.all(np.isfinite(M0)) and np.all(np.isfinite(K0)) and np.all(np.isfinite(Psi0)) and np.isfinite(nu0)):
            raise ValueError("ObsMNIWPrior: M0, K0, nu0 and Psi0 must be finite")
        if not nu0 > dy - 1:
            raise ValueError(f"ObsMNIWPrior: nu0 must exceed dy - 1 = {dy - 1} (got {nu0})")
        for name, a in (("K0", K0), ("Psi0", Psi0)):
            dg = np.abs(np.diag(a))
            if not np.all(np.abs(a - a.T) <= 1e-12 * (dg[:, None] + dg[None, :])):
                raise ValueError(f"ObsMNIWPrior: {name} must be symmetric")
            try:
                np.linalg.cholesky(0.5 * (a + a.T))
            except np.linalg.LinAlgError:
                raise ValueError(f"ObsMNIWPrior: {name} must be positive definite") from None
        self.dx, self.dy, self.M0, self.K0, self.nu0, self.Psi0 = n - 1, dy, M0, 0.5 * (K0 + K0.T), nu0, 0.5 * (Psi0 + Psi0.T)

    def struct(self, chi_scale=2.0):
        """-> _lib.MniwPrior (auxssm_mniw_prior, its arrays holding (dy, dx + 1), (dx + 1, dx + 1), (dy, dy)); chi_scale 2: the chi buffer holds
        Gamma((nu_n - i) / 2, 1) draws"""
        if self.dx > 4 or self.dy > 4:
            raise ValueError(f"the device step covers dx <= 4 and dy <= 4 (this prior has dx = {self.dx}, dy = {self.dy})")
        p = _lib.MniwPrior()
        for name in ("M0", "K0", "Psi0"):
            arr = getattr(p, name)
            for k, v in enumerate(getattr(self, name).ravel()):
                arr[k] = float(v)
        p.nu0, p.chi_scale = self.nu0, float(chi_scale)
        return p


class ObservationThetaStep:
    """(H, c, R) | x, y for the observation model y_t = H x_t + c + N(0, R) of an LGConcatModel: one conjugate matrix-normal inverse-Wishart draw per chain and
    sweep, on the device (auxssm_observation_theta_update), written into per-chain parameter buffers the next sweep reads:

        step = ObservationThetaStep(model, ObsMNIWPrior(M0, K0, nu0, Psi0));   loop(key, delta, state, kernel, None, n_iter, theta_step=step)

    update=("H", "c", "R") draws the three jointly, update=("R",) draws R alone with every chain's H and c fixed (the prior's M0 and K0 are then not read); other
    subsets are not conjugate blocks and are refused.  model: an LGConcatModel with time-invariant Hobs / Robs / cobs (a broadcast view, or equal rows), dx <= 4,
    dy <= 4, T >= 2.  Rows of yobs that are wholly NaN are missing and skipped; a partly missing row is refused (under a dense R it is not conjugate, as in fit_em).
    On its first call the step replaces the device model's Hs, cs, Rs with per-chain buffers (C, dy, dx), (C, dy), (C, dy, dy) of time stride 0 that start as copies
    of the model's values; from then on the model serves chains of that count only (kalman/generic.py::_check_per_chain_params).  The LG_CONCAT sweep reads a
    per-chain observation model in the DENSE layout only (the chain-minor filter forms the concatenated observations from one chain-shared table): the step refuses
    chain-minor chains -- build them with DeviceChains(handle, x, chain_minor=False).  Every call: chains.disable_fused(), the key is split in three by
    random.split, chi <- auxssm_rng_gamma at shapes (nu_n - i) / 2, two normal fills, the update on chains.x; no host synchronisation.  A chain whose posterior
    cannot be factorised keeps its parameters and raises its flag (flags(chains))."""

    def __init__(self, model, prior, update=("H", "c", "R")):
        from .kalman import models as M
        if not isinstance(model, M.LGConcatModel):
            raise ValueError(f"ObservationThetaStep: {type(model).__name__} has no linear-Gaussian observation model (Hobs, cobs, Robs) to draw: the step covers "
                             "LGConcatModel (the count, loading-matrix and Student-t models are not conjugate; LorenzModel rebuilds its model every sweep)")
        if not isinstance(prior, ObsMNIWPrior):
            raise ValueError("ObservationThetaStep: prior must be an ObsMNIWPrior")
        up = tuple(update) if not isinstance(update, str) else (update,)
        if sorted(up) == ["H", "R", "c"]:
            self.mask = 1
        elif up == ("R",):
            self.mask = 2
        else:
            raise ValueError(f"ObservationThetaStep: update must be ('H', 'c', 'R') (drawn jointly) or ('R',) (R alone); {up!r} is not a conjugate block")
        dx, dy = model.dx, model.p_obs
        if dx > 4 or dy > 4:
            raise ValueError(f"ObservationThetaStep: the device step covers dx <= 4 and dy <= 4 (the model has dx = {dx}, dy = {dy})")
        if (prior.dx, prior.dy) != (dx, dy):
            raise ValueError(f"ObservationThetaStep: the prior is for (dx, dy) = ({prior.dx}, {prior.dy}), the model has ({dx}, {dy})")
        if model.T < 2:
            raise ValueError("ObservationThetaStep: the model needs T >= 2")
        for name, core in (("Hobs", (dy, dx)), ("Robs", (dy, dy)), ("cobs", (dy,))):
            a = np.asarray(getattr(model, name))
            if a.ndim == len(core) + 1 and not _time_invariant(a):
                raise ValueError(f"ObservationThetaStep: the model's {name} varies in time; the step draws ONE (H, c, R) per chain")
        y = np.asarray(model.yobs, np.float64).reshape(model.T, dy)
        fin = np.isfinite(y)
        if np.any(fin.any(axis=1) & ~fin.all(axis=1)):
            raise ValueError("ObservationThetaStep: a row of yobs is partly missing; under a dense R only wholly missing (all-NaN) rows are conjugate")
        self.model, self.prior = model, prior
        self._prior_c = prior.struct(2.0)
        self._observed = fin.all(axis=1)
        self._shapes = [0.5 * (prior.nu0 + int(self._observed.sum()) - i) for i in range(dy)]
        self._syy = {}
        self._work = {}

    def _syy_nobs(self, dtype):
        """[S_yy | n_obs] in double from the data as the device holds it (rounded to the chains' dtype)"""
        k = np.dtype(dtype).str
        if k not in self._syy:
            y = np.asarray(self.model.yobs).reshape(self.model.T, self.model.p_obs).astype(dtype).astype(np.float64)[self._observed]
            self._syy[k] = np.concatenate([(y.T @ y).ravel(), [float(y.shape[0])]])
        return self._syy[k]

    # ---- the model's per-chain parameter buffers ----
    def _params(self, handle, dtype, C):
        """-> (H (C, dy, dx), c (C, dy), R (C, dy, dy)) DeviceArrays the device model points at, made per-chain on first use"""
        dl = self.model.device(handle, dtype)[0]
        dx, dy = self.model.dx, self.model.p_obs
        own = dl.bufs.get("observation_theta")
        if own is None:
            host = [np.repeat(np.asarray(getattr(self.model, n)).reshape((-1,) + core)[:1], C, axis=0)
                    for n, core in (("Hobs", (dy, dx)), ("cobs", (dy,)), ("Robs", (dy, dy)))]
            own = dl.bufs["observation_theta"] = tuple(handle.to_device(a, dtype) for a in host)
            H, c, R = own
            sc = 1 if C > 1 else 0
            dl.c.Hs, dl.c.cs, dl.c.Rs = H.arr(sc * dy * dx, 0, 0), c.arr(sc * dy, 0, 0), R.arr(sc * dy * dy, 0, 0)
            dl.bufs["Hs"], dl.bufs["cs"], dl.bufs["Rs"] = H, c, R
        if own[0].shape[0] != C:
            raise ValueError(f"ObservationThetaStep: the model holds per-chain parameters of {own[0].shape[0]} chains, the chains are {C}")
        return own

    def _check_chains(self, chains):
        from .kalman.generic import DeviceChains
        if not isinstance(chains, DeviceChains):
            raise ValueError("ObservationThetaStep: cSMC chains carry their potential in the Feynman-Kac model; the step needs kalman.DeviceChains")
        if (chains.T, chains.dx) != (self.model.T, self.model.dx):
            raise ValueError(f"ObservationThetaStep: the chains are (T, dx) = ({chains.T}, {chains.dx}), the model ({self.model.T}, {self.model.dx})")
        if chains.chain_minor and chains.C > 1:
            raise ValueError("ObservationThetaStep: the sweep reads a per-chain observation model in the dense layout only (the chain-minor filter forms the "
                             "concatenated observations from one chain-shared table): build the chains with DeviceChains(handle, x, chain_minor=False)")

    def __call__(self, key, chains):
        self._check_chains(chains)
        handle, dtype, Cn, dx, dy = chains.handle, chains.dtype, chains.C, self.model.dx, self.model.p_obs
        H, c, R = self._params(handle, dtype, Cn)
        wk = (id(handle), np.dtype(dtype).str, Cn)
        work = self._work.get(wk)
        if work is None:
            self._work.clear()
            work = self._work[wk] = (handle.empty((Cn, dy), dtype), handle.empty((Cn, dy, dy), dtype), handle.empty((Cn, dy, dx + 1), dtype),
                                     handle.zeros((Cn,), np.int32))
        chi, eps_w, eps_a, flags = work
        chains.disable_fused()   # per-chain parameters: the fused chain-shared sweep no longer applies
        k_chi, k_w, k_a = _random.split(key, 3)
        handle.rng_gamma_into(k_chi, 0, self._shapes, chi)
        handle.rng_normal_into(k_w, 0, eps_w)
        handle.rng_normal_into(k_a, 0, eps_a)
        sc = 1 if Cn > 1 else 0
        yarr = self.model.device(handle, dtype)[2]
        handle.observation_theta_update(chains.x, yarr, dy, self._syy_nobs(dtype), self._prior_c, self.mask, chi, eps_w, eps_a, H.arr(sc * dy * dx, 0, 0),
                                        c.arr(sc * dy, 0, 0), R.arr(sc * dy * dy, 0, 0), flags, layout=chains.layout)

    def params(self, chains):
        """-> (H (C, dy, dx), c (C, dy), R (C, dy, dy)) as host arrays (synchronises)"""
        self._check_chains(chains)
        H, c, R = self._params(chains.handle, chains.dtype, chains.C)
        return H.to_host(), c.to_host(), R.to_host()

    def flags(self, chains):
        """-> (C,) int32: 0, or why the last call left chain c unchanged (include/auxssm.h: auxssm_observation_theta_update)"""
        work = self._work.get((id(chains.handle), np.dtype(chains.dtype).str, chains.C))
        return work[3].to_host() if work is not None else np.zeros(chains.C, np.int32)


class ThetaSteps:
    """Several theta steps as one: ThetaSteps(step_a, step_b, ...)(key, chains) splits its key by random.split into one child per step and calls the steps in
    order, each with its own child.  loop(..., theta_step=ThetaSteps(DynamicsThetaStep(...), ObservationThetaStep(...))) is the Gibbs sampler over
    (x, F, b, Q, H, c, R) of an LGConcatModel."""

    def __init__(self, *steps):
        if not steps or not all(callable(s) for s in steps):
            raise ValueError("ThetaSteps: give at least one step, each callable as step(key, chains)")
        self.steps = tuple(steps)

    def __call__(self, key, chains):
        for k, step in zip(_random.split(key, len(self.steps)), self.steps):
            step(k, chains)


def loop(key, init_delta, init_state, kernel_fn, delta_fn, n_iter, target_alpha=None, lr=None, beta=0.01, theta_step=None,
         callback=None):
    """See module docstring.  init_state.x: DeviceChains (kernel_fn(key, state, delta) from kalman.get_kernel) or CsmcChains (from
    csmc.get_kernel / get_independent_kernel).  theta_step: called as theta_step(key, chains) after every sweep (and, on cSMC chains, after the sweep's moments are folded) with the second child of the sweep's key -- a LorenzThetaStep (the Lorenz drift
    parameters), a DynamicsThetaStep ((F, b, Q) of linear-Gaussian dynamics under an MNIWPrior: a Gibbs sampler over (x, F, b, Q)), an ObservationThetaStep
    ((H, c, R) of an LGConcatModel's observation model under an ObsMNIWPrior) or a ThetaSteps of several (both of the latter: a Gibbs sampler over
    (x, F, b, Q, H, c, R)); all write the model's device parameters in place, one set per chain, without a host synchronisation.  On cSMC chains: a
    DynamicsThetaStep built on the kernel's csmc.LinearGaussianDynamics (particle Gibbs over (x, F, b, Q)); a step built for the other kind of chains raises ValueError.
    callback(i, state) is called after every sweep (e.g. to keep thinned samples; it may synchronise).

    Returns (n_iter, stats, state, delta, window_avg_acceptance, avg_acceptance): stats = (sq_jump, mean, sq_mean) as DeviceArrays
    in the chains' resident layout (chains.stats_to_host(a) -> (C, T, dx)); the acceptance averages are DeviceArrays (C,) [Kalman] or
    (C, T) [cSMC]; delta a float [Kalman] or the chains' device array (T,) [cSMC]."""
    from .kalman.generic import DeviceChains
    from .csmc._device import CsmcChains

    chains = init_state.x
    kalman = isinstance(chains, DeviceChains)
    if not kalman and not isinstance(chains, CsmcChains):
        raise ValueError("loop() runs on resident chains: init_state.x must be a kalman.DeviceChains or a csmc.CsmcChains")
    if delta_fn is not None and (target_alpha is None or lr is None):
        raise ValueError("target_alpha and lr are required with delta_fn")
    handle, dtype = chains.handle, chains.dtype
    split = _random.jax_split if _random.compat() == "jax" else _random.split   # (experiment.py:90: keys = jax.random.split(key, n_iter))
    keys = split(key, n_iter)
    stats = tuple(handle.zeros(chains.x.shape, dtype) for _ in range(3))  # fold 0 overwrites: (0 u + v) / 1 = v, as stats_fn(x, x) would
    flags = chains.accepted if kalman else chains.ancestors
    m = 1 if kalman else chains.T
    upd = init_state.updated if init_state.updated is not None else True
    if hasattr(upd, "to_host"):  # the state a previous loop returned: flags still on the device
        upd = upd.to_host().reshape(chains.C, m) != 0
    upd0 = np.broadcast_to(np.asarray(upd, dtype), (chains.C, m))
    avg = handle.to_device(upd0, dtype)
    window = handle.to_device(upd0, dtype)
    rule = _is_reference_rule(delta_fn) if delta_fn is not None else None
    if kalman:
        delta = float(init_delta)
        # the reference's rule while adapting: delta stays on the DEVICE (one scalar, updated by auxssm_delta_adapt from the chain-mean of the
        # windowed acceptance and read by auxssm_kalman_sweep_dd) -- no host round trip per sweep.  A user rule still runs on the host.
        delta_dev = handle.to_device(np.full(1, delta, dtype), dtype) if rule is not None else None
    else:
        if init_delta is not None:
            chains.set_delta(init_delta)
        delta = None
        delta_dev = None
        x_prev = handle.empty(chains.x.shape, dtype)
    state = init_state
    if kalman:
        handle.stats_attach(stats, 0, chains.x)
    try:
        for i in range(n_iter):
            if kalman:
                k_sweep, k_theta = (keys[i], None) if theta_step is None else split(keys[i], 2)
                state = kernel_fn(k_sweep, state, delta if delta_dev is None else delta_dev)  # folds the moments in its accept step
                if theta_step is not None:
                    theta_step(k_theta, chains)
            else:
                k_sweep, k_theta = (keys[i], None) if theta_step is None else split(keys[i], 2)
                x_prev.copy_from(chains.x)
                state = kernel_fn(k_sweep, state, None)
                handle.stats_update(i, x_prev, chains.x, stats)
                if theta_step is not None:   # particle Gibbs: theta | x on the trajectory the sweep has just drawn
                    theta_step(k_theta, chains)
            handle.accept_update(i, beta, flags, avg, window)
            if delta_fn is not None:
                lr_i = (n_iter - i) * lr / n_iter
                if kalman and delta_dev is not None:
                    handle.delta_adapt(window, target_alpha, lr_i, delta_dev, None, rule[0], rule[1])
                elif kalman:
                    delta = float(delta_fn(delta, target_alpha, float(np.mean(window.to_host())), lr_i))
                elif rule is not None:
                    handle.delta_adapt(window, target_alpha, lr_i, chains.delta, chains.sqrt_half_delta, rule[0], rule[1])
                else:
                    chains.set_delta(delta_fn(chains.delta.to_host(), target_alpha, np.mean(window.to_host(), axis=0), lr_i))
            if callback is not None:
                callback(i, state)
    finally:
        if kalman:
            handle.stats_attach(None, 0)
    if kalman and delta_dev is not None:
        delta = float(delta_dev.to_host()[0])  # one read at the END of the run (the return value is a float, as the reference's)
    return n_iter, stats, state, (delta if kalman else chains.delta), window, avg
