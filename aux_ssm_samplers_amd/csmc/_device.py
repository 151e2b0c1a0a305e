"""Host driver of auxssm_csmc_sweep: model description, noise, buffers."""
import ctypes as C
import hashlib
import os

import numpy as np

from .. import _lib, random as _random
from .models import (GaussianInit, LinearGaussianDynamics, FlatPotential, GaussianObsPotential, SVPotential, Lorenz63Dynamics,
                     MaskedGaussianObsPotential, MultivariateTPotential, LinearGaussianPotential, PoissonPotential, BinomialPotential,
                     NegBinomialPotential, DevicePotential, DeviceGaussianDynamics)

_UNSUPPORTED = ("{what} is a Python object the HIP kernels cannot evaluate. The cSMC kernels run the closed model family "
                "of aux_ssm_samplers_amd.csmc.models (GaussianInit, LinearGaussianDynamics, Lorenz63Dynamics, FlatPotential, "
                "GaussianObsPotential, MaskedGaussianObsPotential, SVPotential, MultivariateTPotential, LinearGaussianPotential, PoissonPotential, BinomialPotential, NegBinomialPotential) in-kernel; there is no CPU fallback.")


class FkDesc:
    def __init__(self, proposal, pot, m0, chol_P0, F, b, chol_Q, transition=_lib.TRANS_LINEAR, gradient=_lib.GRAD_NONE):
        """pot: everything about the potential (_potential)"""
        self.proposal, self.transition, self.gradient = proposal, int(transition), int(gradient)
        self.m0 = np.ascontiguousarray(m0, np.float64).reshape(-1)
        self.dx = self.m0.shape[0]
        d = self.dx
        self.chol_P0 = np.ascontiguousarray(chol_P0, np.float64).reshape(d, d)
        F, b, chol_Q = np.asarray(F, np.float64), np.asarray(b, np.float64), np.asarray(chol_Q, np.float64)
        self.tv = None  # time-varying transitions: (F_t (T-1,d,d), b_t (T-1,d), chol_Q_t (T-1,d,d)), uploaded per handle / dtype
        if F.ndim == 3:
            n = F.shape[0]
            self.tv = (np.ascontiguousarray(F.reshape(n, d, d)), np.ascontiguousarray(np.broadcast_to(b, (n, d))),
                       np.ascontiguousarray(np.broadcast_to(chol_Q, (n, d, d))))
            F, b, chol_Q = self.tv[0][0], self.tv[1][0], self.tv[2][0]  # (the invariant slots are not read then)
        self.F = np.ascontiguousarray(F, np.float64).reshape(d, d)
        self.b = np.ascontiguousarray(b, np.float64).reshape(d)
        self.chol_Q = np.ascontiguousarray(chol_Q, np.float64).reshape(d, d)
        self._ydev = {}
        self._tvdev = {}
        self.user = None  # UserModel: the parts of the model compiled from device code (auxssm_csmc_sweep_program)
        mat = lambda a: None if a is None else np.ascontiguousarray(a, np.float64).reshape(d, d)  # noqa: E731 -- host (dx, dx), like F
        self.potential, self.sig_y = pot["kind"], float(pot.get("sig_y", 1.0))
        self.y = None if pot.get("y") is None else np.asarray(pot["y"])  # the device's observation array (POT_LIN_GAUSS: the whitened rows)
        self.nu, self.prec = float(pot.get("nu", 0.0)), mat(pot.get("prec"))  # POT_MVT: degrees of freedom and the precision matrix
        self.obs_H, self.obs_const = mat(pot.get("obs_H")), float(pot.get("obs_const", 0.0))  # POT_LIN_GAUSS: Hw zero-padded to (dx, dx), and c_lin

    def tvdev(self, handle, dtype, T):
        """device copies of the time-varying transition arrays (or None)"""
        if self.tv is None:
            return None
        if self.tv[0].shape[0] != T - 1:
            raise ValueError(f"time-varying dynamics have {self.tv[0].shape[0]} rows, the state has T - 1 = {T - 1} transitions")
        key = (id(handle), np.dtype(dtype).str)
        ent = self._tvdev.get(key)
        if ent is None or ent[0] is not handle:  # (the entry keeps its handle alive, so its id cannot pass to another handle: UserModel.struct)
            ent = self._tvdev[key] = (handle, tuple(handle.to_device(a, dtype) for a in self.tv))
        return ent[1]

    def struct(self, handle, dtype, T):
        """the auxssm_fk_model of this description on `handle` (keeps the device arrays alive through self)"""
        m = _lib.FkModelObs(self.proposal, self.potential, self.dx, self.transition, self.m0.ctypes.data, self.chol_P0.ctypes.data,
                         self.F.ctypes.data, self.b.ctypes.data, self.chol_Q.ctypes.data, None, self.sig_y, None, None, None, self.gradient, 0,
                         self.nu, None if self.prec is None else self.prec.ctypes.data,
                         None if self.obs_H is None else self.obs_H.ctypes.data, self.obs_const)
        yd = self.ydev(handle, dtype)
        if yd is not None:
            nt = yd.shape[1] if self.potential == _lib.POT_LOGISTIC else yd.shape[0]  # (POT_LOGISTIC: (2, T, dx), the data and the sizes)
            if nt != T:
                raise ValueError(f"observations have {nt} time steps, state has {T}")
            m.y = yd.ptr.value
        tv = self.tvdev(handle, dtype, T)
        if tv is not None:
            m.F_t, m.b_t, m.chol_Q_t = tv[0].ptr.value, tv[1].ptr.value, tv[2].ptr.value
        return m

    def ydev(self, handle, dtype):
        if self.y is None:
            return None
        key = (id(handle), np.dtype(dtype).str)
        ent = self._ydev.get(key)
        if ent is None or ent[0] is not handle:
            ent = self._ydev[key] = (handle, handle.to_device(self.y, dtype))
        return ent[1]


def _potential(G0, Gt, d):
    """everything FkDesc needs about the potential: dict(kind, y = the device's observation array (T, dx) -- (2, T, dx) for POT_LOGISTIC -- [, sig_y] [, the
    kind's own parameters])"""
    if type(G0) is not type(Gt) and not (isinstance(G0, GaussianInit) and isinstance(Gt, GaussianObsPotential)):
        raise NotImplementedError(_UNSUPPORTED.format(what=f"G0={type(G0).__name__} with Gt={type(Gt).__name__}"))
    if isinstance(Gt, FlatPotential):
        return dict(kind=_lib.POT_FLAT)
    if not isinstance(Gt, (MultivariateTPotential, LinearGaussianPotential, PoissonPotential, BinomialPotential, NegBinomialPotential, MaskedGaussianObsPotential, GaussianObsPotential, SVPotential)):
        raise NotImplementedError(_UNSUPPORTED.format(what=f"Gt={type(Gt).__name__}"))
    y0 = G0.m0 if isinstance(G0, GaussianInit) else G0.y
    if y0 is None or Gt.params is None:
        raise ValueError("the potential needs y (G0.y = ys[0]) and params (Gt.params = ys[1:])")
    dy = Gt.dy if isinstance(Gt, LinearGaussianPotential) else d
    ys = np.concatenate([np.reshape(y0, (1, dy)), np.reshape(Gt.params, (-1, dy))], axis=0)
    if isinstance(Gt, MultivariateTPotential):
        if G0.nu != Gt.nu or not np.array_equal(G0.prec, Gt.prec):
            raise ValueError("G0 and Gt must carry the same nu and prec")
        if Gt.dx != d:
            raise ValueError(f"the potential's precision matrix is {Gt.dx} x {Gt.dx}, the state has dimension {d}")
        return dict(kind=_lib.POT_MVT, y=ys, nu=Gt.nu, prec=Gt.prec)
    if isinstance(Gt, LinearGaussianPotential):
        if not (np.array_equal(G0.H, Gt.H) and np.array_equal(G0.R, Gt.R) and np.array_equal(G0.c, Gt.c)):
            raise ValueError("G0 and Gt must carry the same H, R and c")
        if Gt.dx != d:
            raise ValueError(f"the potential's observation matrix has {Gt.dx} columns, the state has dimension {d}")
        Hw, yw, c_lin = Gt.whitened(ys)  # whitened once, in float64, here at description time
        return dict(kind=_lib.POT_LIN_GAUSS, y=yw, obs_H=Hw, obs_const=c_lin)
    if isinstance(Gt, SVPotential):
        return dict(kind=_lib.POT_SV, y=ys)
    if isinstance(Gt, PoissonPotential):
        PoissonPotential.check_counts(ys)  # (G0.y / Gt.params may have been assigned after construction)
        return dict(kind=_lib.POT_POISSON, y=ys)
    if isinstance(Gt, (BinomialPotential, NegBinomialPotential)):
        # the one kind whose device array has two planes: [the data | the sizes], (2, T, dx); sizes() validates (y / params may have been assigned later)
        return dict(kind=_lib.POT_LOGISTIC, y=np.stack([ys, np.concatenate([G0.sizes(), Gt.sizes()], axis=0)]))
    masked = isinstance(Gt, MaskedGaussianObsPotential)
    s0 = G0.sig if masked else (float(np.sqrt(np.reshape(G0.P0, -1)[0])) if isinstance(G0, GaussianInit) else Gt.sig)
    if abs(s0 - Gt.sig) > 1e-12 * Gt.sig:
        raise NotImplementedError("G0 and Gt must share the observation noise scale")
    return dict(kind=_lib.POT_GAUSS_OBS_MASKED if masked else _lib.POT_GAUSS_OBS, y=ys, sig_y=Gt.sig)


def _dyn(M0, Mt):
    if not isinstance(M0, GaussianInit):
        raise NotImplementedError(_UNSUPPORTED.format(what=f"M0={type(M0).__name__}"))
    if not isinstance(Mt, (LinearGaussianDynamics, Lorenz63Dynamics)):
        raise NotImplementedError(_UNSUPPORTED.format(what=f"Mt={type(Mt).__name__}"))
    return M0, Mt


def _trans(Mt):
    """(transition kind, F, b) as the C ABI wants them (include/auxssm.h, auxssm_fk_transition)"""
    if isinstance(Mt, Lorenz63Dynamics):
        F = np.zeros((3, 3))
        F[0] = np.asarray(Mt.theta, np.float64).reshape(3)
        return _lib.TRANS_LORENZ63_EM, F, np.array([float(Mt.dt), 0.0, 0.0])
    return _lib.TRANS_LINEAR, Mt.F, Mt.b


# ---- user-defined models (models.DevicePotential / DeviceGaussianDynamics) ------------------------------------------------------------------------------
_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc")
_programs = {}         # (sha256 of the source, dtype, dx, flags) -> auxssm_fk_program, for the life of the process
_compiles = [0]


def program_compiles():
    """how many programs this process has compiled (a cached program is not compiled again)"""
    return _compiles[0]


def compile_program(source, dtype, dx, flags):
    """auxssm_fk_program_compile, cached in-process by source hash; a source hipRTC rejects raises AuxSSMError with hipRTC's log"""
    key = (hashlib.sha256(source.encode()).hexdigest(), np.dtype(dtype).str, int(dx), int(flags))
    prog = _programs.get(key)
    if prog is not None:
        return prog
    lib = _lib.load()
    log = C.create_string_buffer(1 << 16)
    out = C.c_void_p()
    rc = lib.auxssm_fk_program_compile(source.encode(), _CSRC.encode(), _lib.dtype_code(dtype), int(dx), int(flags), log, len(log), C.byref(out))
    if rc != 0:
        msg = lib.auxssm_last_error().decode(errors="replace")
        if rc == -1 and log.value:
            raise _lib.AuxSSMError(f"auxssm: {msg}\n{log.value.decode(errors='replace')}")
        if rc == -2:  # AUXSSM_ERR_UNSUPPORTED
            raise NotImplementedError(f"auxssm: {msg}")
        _lib.check(rc)
    _compiles[0] += 1
    _programs[key] = out
    return out


def program_info(prog):
    """dict(dtype code, dx, flags, has_bound) of a compiled program (auxssm_fk_program_info)"""
    v = [C.c_int32() for _ in range(4)]
    _lib.check(_lib.load().auxssm_fk_program_info(prog, *(C.byref(x) for x in v)))
    return dict(zip(("dtype", "dx", "flags", "has_bound"), (x.value for x in v)))


class UserModel:
    """the device-code parts of a model: the program source and flags, the user potential's observations (T, p) and the two parameter vectors"""

    def __init__(self, source, flags, dx, y=None, theta_g=None, theta_m=None):
        self.source, self.flags, self.dx = source, int(flags), int(dx)
        self.y = None if y is None else np.ascontiguousarray(y, np.float64)
        self.p = 0 if self.y is None else self.y.shape[1]
        self.theta_g = None if theta_g is None else np.ascontiguousarray(np.reshape(theta_g, -1), np.float64)
        self.theta_m = None if theta_m is None else np.ascontiguousarray(np.reshape(theta_m, -1), np.float64)
        self._dev = {}
        for dt in (np.float32, np.float64):  # compiled now (get_kernel time), not at the first sweep
            self.program(dt)

    def program(self, dtype):
        return compile_program(self.source, dtype, self.dx, self.flags)

    def struct(self, handle, dtype, T):
        # the entry keeps its handle: an id is only unique among live objects, so a cache keyed by id(handle) alone could hand a later handle
        # another one's device pointers
        key = (id(handle), np.dtype(dtype).str)
        ent = self._dev.get(key)
        if ent is None or ent[0] is not handle:
            ent = self._dev[key] = (handle, tuple(None if a is None else handle.to_device(a, dtype) for a in (self.y, self.theta_g, self.theta_m)))
        yd, tg, tm = ent[1]
        if yd is not None and yd.shape[0] != T:
            raise ValueError(f"observations have {yd.shape[0]} time steps, state has {T}")
        u = _lib.FkUser()
        u.y, u.theta_g, u.theta_m = (None if a is None else a.ptr.value for a in (yd, tg, tm))
        u.p = self.p
        return u


def _is_user(*objs):
    return any(isinstance(o, (DevicePotential, DeviceGaussianDynamics)) for o in objs)


def _describe_user(proposal, M0, G0, Mt, Gt, gradient, parallel):
    """the FkDesc of a model with device-code parts (the rest from the built-in family); every limit of the program path raises NotImplementedError"""
    if parallel:
        raise NotImplementedError("user-defined models (DevicePotential / DeviceGaussianDynamics) run the sequential cSMC sweep only: parallel=True "
                                  "(the parallel-in-time kernels) is not compiled for them")
    if not isinstance(M0, GaussianInit):
        raise NotImplementedError(f"a user-defined M0 ({type(M0).__name__}) is not supported: user-defined models keep the Gaussian initial "
                                  "distribution GaussianInit(m0, P0)")
    d = int(np.size(M0.m0))
    if d > 4:
        raise NotImplementedError(f"dx={d}: user-defined models run the sequential kernels of dx <= 4; the wide-state path (dx > 4) is not "
                                  "compiled for them")
    flags, src, theta_g, theta_m, yu = 0, [], None, None, None
    if isinstance(G0, DevicePotential) or isinstance(Gt, DevicePotential):
        if not (isinstance(G0, DevicePotential) and isinstance(Gt, DevicePotential)):
            raise NotImplementedError("G0 and Gt must both be DevicePotential (with the same source and theta)")
        if G0.source != Gt.source:
            raise ValueError("G0 and Gt must carry the same source")
        tg0, tgt = (None if th is None else np.asarray(th, np.float64).reshape(-1) for th in (G0.theta, Gt.theta))
        if (tg0 is None) != (tgt is None) or (tg0 is not None and not np.array_equal(tg0, tgt)):
            raise ValueError("G0 and Gt must carry the same theta")
        if (G0.y is None) != (Gt.params is None):
            raise ValueError("the potential's observations: give both G0.y = ys[0] and Gt.params = ys[1:], or neither")
        if G0.y is not None:
            p = G0.p or Gt.p or int(np.size(G0.y))
            yu = np.concatenate([np.reshape(G0.y, (1, p)), np.reshape(Gt.params, (-1, p))], axis=0)
        flags |= _lib.FK_USER_POTENTIAL
        src.append(Gt.source)
        theta_g = tgt
        pot = dict(kind=_lib.POT_FLAT)
    else:
        pot = _potential(G0, Gt, d)
    if isinstance(Mt, DeviceGaussianDynamics):
        Q = np.asarray(Mt.Q, np.float64)
        if Q.ndim == 3:
            raise NotImplementedError("DeviceGaussianDynamics: a time-varying Q together with a user mean is not supported (Q must be (d, d))")
        flags |= _lib.FK_USER_MEAN
        if Mt.source not in src:
            src.append(Mt.source)
        theta_m = Mt.theta
        tk, F, b, LQ = _lib.TRANS_LINEAR, np.zeros((d, d)), np.zeros(d), Mt.chol()
    elif isinstance(Mt, (LinearGaussianDynamics, Lorenz63Dynamics)):
        if isinstance(Mt, LinearGaussianDynamics) and Mt.time_varying:
            raise NotImplementedError("user-defined potentials run time-invariant transitions: time-varying LinearGaussianDynamics is not supported with them")
        tk, F, b = _trans(Mt)
        LQ = Mt.chol()
    else:
        raise NotImplementedError(f"Mt={type(Mt).__name__}: user-defined transitions are Gaussian, x_t ~ N(mean(x_{{t-1}}), Q) (DeviceGaussianDynamics); "
                                  "non-Gaussian transition noise is not supported")
    if gradient:  # the program also holds the gradient kernel, from the derivatives of the user-defined parts (grad_log_g / mean_vjp)
        flags |= _lib.FK_USER_GRADIENT
    fk = FkDesc(proposal, pot, M0.m0, M0.chol(), F, b, LQ, tk, gradient)
    fk.user = UserModel("\n".join(src), flags, d, yu, theta_g, theta_m)
    return fk


def _describe_builtin(proposal, M0, G0, Mt, Gt, gradient):
    """the FkDesc of a model of the closed family, once the proposal's own checks have passed"""
    d = np.size(M0.m0)
    tk, F, b = _trans(Mt)
    return FkDesc(proposal, _potential(G0, Gt, d), M0.m0, M0.chol(), F, b, Mt.chol(), tk, gradient)


def describe_bootstrap(M0, G0, Mt, Gt, Pt):
    """_primitives.csmc.get_kernel: M0/Mt are the proposals, G0/Gt the potentials."""
    if _is_user(M0, G0, Mt, Gt):
        if Pt is not None and Pt is not Mt:
            raise NotImplementedError("backward sampling with Pt != Mt is not supported by the bootstrap device kernel")
        return _describe_user(_lib.PROP_BOOTSTRAP_LG, M0, G0, Mt, Gt, _lib.GRAD_NONE, False)
    M0, Mt = _dyn(M0, Mt)
    if Pt is not None and Pt is not Mt and not (isinstance(Pt, LinearGaussianDynamics) and isinstance(Mt, LinearGaussianDynamics)
                                                   and np.array_equal(Pt.F, Mt.F) and np.array_equal(Pt.Q, Mt.Q) and np.array_equal(Pt.b, Mt.b)):
        raise NotImplementedError("backward sampling with Pt != Mt is not supported by the bootstrap device kernel")
    return _describe_builtin(_lib.PROP_BOOTSTRAP_LG, M0, G0, Mt, Gt, _lib.GRAD_NONE)


def describe_independent(M0, G0, Mt, Gt, Pt, gradient=_lib.GRAD_NONE, parallel=False):
    """csmc.get_independent_kernel (classical): proposals N(u_t [+ delta_t/2 grad_t], delta_t/2 I); M0/Mt enter the weights."""
    if _is_user(M0, G0, Mt, Gt):
        if Pt is not None and Pt is not Mt:
            raise NotImplementedError("Pt must be the model dynamics Mt")
        return _describe_user(_lib.PROP_AUX_INDEPENDENT, M0, G0, Mt, Gt, gradient, parallel)
    M0, Mt = _dyn(M0, Mt)
    if Pt is not None and Pt is not Mt:
        raise NotImplementedError("Pt must be the model dynamics Mt")
    return _describe_builtin(_lib.PROP_AUX_INDEPENDENT, M0, G0, Mt, Gt, gradient)


def describe_guided(M0, G0, Mt, Gt, Pt, gradient=_lib.GRAD_NONE):
    """csmc.get_guided_kernel: proposals N(pred + K_t (u_t - pred), P - K_t P) conditioned on the auxiliary variable AND the parent (pred = m0 / P = P0
    at t = 0, pred = the transition mean of the parent / P = Q after), K_t = P (P + delta_t/2 I)^-1; with a gradient, u_t is shifted by
    delta_t/2 grad log g_t(u_t) inside the proposal mean.  The closed model family with time-invariant transitions only."""
    if _is_user(M0, G0, Mt, Gt):
        raise NotImplementedError("guided proposals run the closed model family only: user-defined models (DevicePotential / DeviceGaussianDynamics) "
                                  "are not compiled into the guided kernels")
    M0, Mt = _dyn(M0, Mt)
    if isinstance(Mt, LinearGaussianDynamics) and Mt.time_varying:
        raise NotImplementedError("guided proposals run time-invariant transitions: time-varying LinearGaussianDynamics is not supported with them")
    if Pt is not None and Pt is not Mt:
        raise NotImplementedError("Pt must be the model dynamics Mt")
    if gradient not in (_lib.GRAD_NONE, _lib.GRAD_REFERENCE):
        raise NotImplementedError('guided proposals take gradient=False or True (the potential\'s gradient at u, as the reference has it): gradient="exact" '
                                  "is a weighting of the independent proposals")
    return _describe_builtin(_lib.PROP_AUX_GUIDED, M0, G0, Mt, Gt, gradient)


_AUXILIARY = (_lib.PROP_AUX_INDEPENDENT, _lib.PROP_AUX_GUIDED)  # the proposals built around u = x + sqrt(delta / 2) eps_aux


def key_noise(handle, key, Cn, T, N, d, dtype, wide=None):
    """The explicit noise arrays a THREEFRY sweep with `key` draws in-kernel (index map: csrc/csmc.hip::k_csmc_fwd): an
    EXPLICIT sweep on these arrays is bit-identical to the keyed one.  Debug / test utility.  wide (default: d > 4): the wide-state kernels
    (csrc/csmc_wide.hip) index their draws by the natural flat position in the explicit arrays."""
    if wide is None:
        wide = d > 4
    if wide:
        return dict(eps_aux=handle.rng_normal(key, 1, (Cn, T, d), dtype).to_host(), eps_prop=handle.rng_normal(key, 2, (Cn, T, N, d), dtype).to_host(),
                    u_res=handle.rng_uniform(key, 3, (Cn, max(T - 1, 0), N), dtype).to_host() if T > 1 else np.zeros((Cn, 0, N), dtype),
                    u_bwd=handle.rng_uniform(key, 4, (Cn, T), dtype).to_host())
    T2 = (T + 1) // 2
    ep = handle.rng_normal(key, 2, (Cn, T2, N, d, 2), dtype).to_host()
    ur = handle.rng_uniform(key, 3, (Cn, T2, N, 2), dtype).to_host()
    return dict(eps_aux=handle.rng_normal(key, 1, (Cn, T, d), dtype).to_host(),
                eps_prop=np.ascontiguousarray(np.moveaxis(ep, 4, 2).reshape(Cn, 2 * T2, N, d)[:, :T]),
                u_res=np.ascontiguousarray(np.moveaxis(ur, 3, 2).reshape(Cn, 2 * T2, N)[:, :max(T - 1, 0)]),
                u_bwd=handle.rng_uniform(key, 4, (Cn, T), dtype).to_host())


def _noise(handle, dtype, Cn, key, noise=None, shapes=None, jax_noise=None, need_all=False):
    """(CsmcNoise, the device buffers it points to) of one sweep.  noise: dict of explicit arrays, uploaded in the shapes of `shapes` (need_all: every name of
    `shapes` must be there; otherwise an absent one stays NULL); None -> Threefry(key), or under random.set_compat("jax") the reference's own draws from this
    key as explicit arrays, jax_noise(key) per chain (several chains: one key per chain, `key` (C, 2) or split(key, C))."""
    nz, keep = _lib.CsmcNoise(), []
    if noise is None and _random.compat() == "jax":
        kk = np.asarray(key, np.uint32)
        keys = kk if kk.ndim == 2 else (_random.as_key(key)[None] if Cn == 1 else _random.jax_split(_random.as_key(key), Cn))
        if keys.shape[0] != Cn:
            raise ValueError(f"{keys.shape[0]} keys for {Cn} chains")
        per = [jax_noise(k_) for k_ in keys]
        noise = {name: np.stack([p_[name] for p_ in per]) for name in per[0]}
    if noise is None:
        k = _random.as_key(key)
        nz.mode, nz.key0, nz.key1 = _lib.NOISE_THREEFRY, int(k[0]), int(k[1])
        return nz, keep
    nz.mode = _lib.NOISE_EXPLICIT
    for name, shp in shapes.items():
        a = noise[name] if need_all else noise.get(name)
        if a is None:
            continue
        buf = handle.to_device(np.asarray(a, dtype).reshape(shp))
        keep.append(buf)
        setattr(nz, name, buf.ptr.value)
    return nz, keep


def _no_jax_resident():
    if _random.compat() == "jax":
        raise NotImplementedError('random.set_compat("jax") runs the particle kernels on explicit arrays of the reference\'s draws (T x N x d per chain): pass host '
                                  "states (csmc/_device.py::sweep); resident chains draw inside the kernels from this package's own streams")


class CsmcChains:
    """C chains' reference trajectories resident in HBM, (C, T, d), with the sweep's other per-chain buffers: a run of sweeps on them
    (kernel(key, state, delta) with state.x a CsmcChains) never returns to the host.  delta: per-time-step step sizes (T,) kept on the
    device beside sqrt(delta / 2), the array the sweep reads (csmc/generic.py:61-63)."""

    def __init__(self, handle, x, delta=None, dtype=None):
        x = np.asarray(x)
        if x.ndim == 2:
            x = x[None]
        self.handle = handle
        self.C, self.T, self.dx = x.shape
        self.dtype = np.dtype(dtype or (np.float32 if x.dtype == np.float32 else np.float64))
        self.x = handle.to_device(x, self.dtype)
        self.ancestors = handle.zeros((self.C, self.T), np.int32)
        self.delta = self.sqrt_half_delta = None
        self.dynamics = None  # ChainDynamics: per-chain (F, b, Q, chol_Q), attached by loop.DynamicsThetaStep -- the sweeps then read chain c's own transition
        if delta is not None:
            self.set_delta(delta)

    def set_delta(self, delta):
        d = np.asarray(delta, np.float64) * np.ones(self.T)
        self.delta = self.handle.to_device(d, self.dtype)
        self.sqrt_half_delta = self.handle.to_device(np.sqrt(0.5 * d), self.dtype)

    def to_host(self):
        return self.x.to_host()

    def stats_to_host(self, a):
        return a.to_host()


class ChainDynamics:
    """Per-chain linear-Gaussian transitions of resident cSMC chains (auxssm_csmc_sweep_chain_dynamics): the LIVE quadruple F (C, d, d), b (C, d), Q (C, d, d),
    chol_Q (C, d, d) the sweep reads, the STAGING buffers F_new, b_new, Q_new a conjugate draw is written into, the draw's step_flags and the commit's flags
    (auxssm_csmc_dynamics_commit moves a chain's staging values into the live ones, or leaves them and says why).  All start as C copies of (F, b, Q)."""

    def __init__(self, handle, dtype, C, F, b, Q):
        F, Q = (np.atleast_2d(np.asarray(a, np.float64)) for a in (F, Q))
        d = F.shape[0]
        b = np.asarray(b, np.float64).reshape(d)
        Qr = Q.astype(dtype).astype(np.float64)  # the factor of Q as the live buffer holds it, as the commit forms it
        host = dict(F=F, b=b, Q=Q, chol_Q=np.linalg.cholesky(Qr), F_new=F, b_new=b, Q_new=Q)
        for name, a in host.items():
            setattr(self, name, handle.to_device(np.repeat(a[None], C, axis=0), dtype))
        self.step_flags, self.flags = handle.zeros((C,), np.int32), handle.zeros((C,), np.int32)
        self.handle, self.dtype, self.C, self.dx = handle, np.dtype(dtype), int(C), d

    def struct(self):
        return _lib.FkChainDynamics(self.F.ptr.value, self.b.ptr.value, self.chol_Q.ptr.value)

    def commit(self):
        self.handle.csmc_dynamics_commit(self.F_new, self.b_new, self.Q_new, self.step_flags, self.F, self.b, self.Q, self.chol_Q, self.flags)


def _check_chain_dynamics(fk, chains):
    """why a description cannot run on the per-chain transitions of chains.dynamics (ValueError), or nothing"""
    dyn = chains.dynamics
    why = None
    if fk.user is not None:
        why = "user-defined models (DevicePotential / DeviceGaussianDynamics) are compiled for chain-shared transitions"
    elif fk.proposal == _lib.PROP_AUX_GUIDED:
        why = "guided proposals run chain-shared transitions (their K_t / chol Lambda_t tables would be per chain and step)"
    elif fk.dx > 4:
        why = f"dx={fk.dx}: the wide-state kernels (dx > 4) read one chain-shared transition"
    elif fk.transition != _lib.TRANS_LINEAR:
        why = "Lorenz63Dynamics has no (F, b, Q) to replace"
    elif fk.tv is not None:
        why = "the description's transitions vary in time; per-chain dynamics are time-invariant"
    elif (dyn.C, dyn.dx) != (chains.C, chains.dx) or dyn.handle is not chains.handle or dyn.dtype != chains.dtype:
        why = f"they were attached for {dyn.C} chains of dx={dyn.dx} ({dyn.dtype}), the chains are {chains.C} of dx={chains.dx} ({chains.dtype})"
    if why is not None:
        raise ValueError(f"these chains carry per-chain dynamics (CsmcChains.dynamics, attached by a DynamicsThetaStep), which this kernel cannot read: {why}")


def sweep_resident(fk, chains, N, backward, key):
    """One Threefry-keyed auxssm_csmc_sweep on resident chains -- auxssm_csmc_sweep_chain_dynamics when the chains carry per-chain dynamics.  Asynchronous."""
    _no_jax_resident()
    handle, d = chains.handle, chains.dx
    if d != fk.dx:
        raise ValueError(f"state dimension {d} != model dimension {fk.dx}")
    m = fk.struct(handle, chains.dtype, chains.T)
    shd = None
    if fk.proposal in _AUXILIARY:
        if chains.sqrt_half_delta is None:
            raise ValueError("delta is required")
        shd = chains.sqrt_half_delta
    nz, _ = _noise(handle, chains.dtype, chains.C, key)
    dyn = None
    if chains.dynamics is not None:
        _check_chain_dynamics(fk, chains)
        dyn = chains.dynamics.struct()
    _csmc_call(handle, fk, chains.dtype, m, chains.C, chains.T, N, backward, shd, chains.x, nz, chains.ancestors, None, None, None, dyn)


def _csmc_call(handle, fk, dtype, m, Cn, T, N, backward, shd, xd, nz, anc, xs, lws, As, dyn=None):
    """auxssm_csmc_sweep, auxssm_csmc_sweep_chain_dynamics with per-chain transitions (dyn: an FkChainDynamics), or auxssm_csmc_sweep_program for a model with
    device-code parts"""
    args = (Cn, T, N, int(bool(backward)), shd.ptr if shd is not None else None, xd.ptr, C.byref(nz), anc.ptr,
            xs.ptr if xs else None, lws.ptr if lws else None, As.ptr if As else None)
    if dyn is not None:
        if fk.user is not None:
            raise ValueError("per-chain dynamics: user-defined models are compiled for chain-shared transitions")
        _lib.check(handle.lib.auxssm_csmc_sweep_chain_dynamics(handle.h, _lib.dtype_code(dtype), C.byref(m), C.byref(dyn), *args))
    elif fk.user is None:
        _lib.check(handle.lib.auxssm_csmc_sweep(handle.h, _lib.dtype_code(dtype), C.byref(m), *args))
    else:
        u = fk.user.struct(handle, dtype, T)
        _lib.check(handle.lib.auxssm_csmc_sweep_program(handle.h, fk.user.program(dtype), _lib.dtype_code(dtype), C.byref(m), C.byref(u), *args))


def pit_sweep_resident(fk, chains, N, key):
    """One Threefry-keyed auxssm_csmc_pit_sweep (parallel-in-time cSMC) on resident chains.  Asynchronous."""
    _no_jax_resident()
    handle = chains.handle
    _no_user_pit(fk)
    if chains.dynamics is not None:
        raise ValueError("these chains carry per-chain dynamics (CsmcChains.dynamics, attached by a DynamicsThetaStep): the parallel-in-time kernels read one "
                         "chain-shared transition and would ignore them; run the sequential sweep (parallel=False)")
    if chains.dx != fk.dx:
        raise ValueError(f"state dimension {chains.dx} != model dimension {fk.dx}")
    if chains.sqrt_half_delta is None:
        raise ValueError("delta is required")
    m = fk.struct(handle, chains.dtype, chains.T)
    nz, _ = _noise(handle, chains.dtype, chains.C, key)
    _lib.check(handle.lib.auxssm_csmc_pit_sweep(handle.h, _lib.dtype_code(chains.dtype), C.byref(m), chains.C, chains.T, N,
                                                chains.sqrt_half_delta.ptr, chains.x.ptr, C.byref(nz), chains.ancestors.ptr))


def _no_user_pit(fk):
    if fk.user is not None:
        raise NotImplementedError("user-defined models (DevicePotential / DeviceGaussianDynamics) run the sequential cSMC sweep only: the "
                                  "parallel-in-time kernels are not compiled for them")


def pit_sweep(fk, x, N, *, key=None, noise=None, delta=None, handle=None):
    """Parallel-in-time cSMC sweep.  x: (T, d) one chain or (C, T, d).  noise: dict(eps_aux (C,T,d), eps_prop (C,T,N,d), u_res (C,T,N)) of
    explicit arrays or None -> Threefry(key).  Returns (x_new, ancestors)."""
    _no_user_pit(fk)
    handle = handle or _lib.default_handle()
    x = np.asarray(x)
    single = x.ndim == 2
    xc = x[None] if single else x
    Cn, T, d = xc.shape
    if d != fk.dx:
        raise ValueError(f"state dimension {d} != model dimension {fk.dx}")
    if delta is None:
        raise ValueError("delta is required")
    dtype = np.dtype(np.float32) if xc.dtype == np.float32 else np.dtype(np.float64)
    xd = handle.to_device(xc, dtype)
    anc = handle.zeros((Cn, T), np.int32)
    m = fk.struct(handle, dtype, T)
    shd = handle.to_device(np.sqrt(0.5 * np.asarray(delta, np.float64)) * np.ones(T), dtype)
    nz, keep = _noise(handle, dtype, Cn, key, noise, dict(eps_prop=(Cn, T, N, d), u_res=(Cn, T, N), eps_aux=(Cn, T, d)),
                      lambda k_: _random.jax_pit_noise(k_, T, N, d, dtype, handle), need_all=True)
    _lib.check(handle.lib.auxssm_csmc_pit_sweep(handle.h, _lib.dtype_code(dtype), C.byref(m), Cn, T, N, shd.ptr, xd.ptr, C.byref(nz), anc.ptr))
    xo, ao = xd.to_host(), anc.to_host()
    return (xo[0], ao[0]) if single else (xo, ao)


def sweep(fk, x, N, backward, *, key=None, noise=None, delta=None, handle=None, want_history=False, chain_dynamics=None):
    """x: (T, d) one chain or (C, T, d).  noise: dict of explicit arrays (eps_prop, u_res, u_bwd[, eps_aux]) or None -> Threefry(key).
    chain_dynamics: (F (C, d, d), b (C, d), chol_Q (C, d, d)) host arrays -> auxssm_csmc_sweep_chain_dynamics, chain c on its own transition.
    Returns (x_new, ancestors, history dict or None)."""
    handle = handle or _lib.default_handle()
    x = np.asarray(x)
    single = x.ndim == 2
    xc = x[None] if single else x
    Cn, T, d = xc.shape
    if d != fk.dx:
        raise ValueError(f"state dimension {d} != model dimension {fk.dx}")
    dtype = np.dtype(np.float32) if xc.dtype == np.float32 else np.dtype(np.float64)
    xd = handle.to_device(xc, dtype)
    anc = handle.zeros((Cn, T), np.int32)
    m = fk.struct(handle, dtype, T)
    shd = None
    if fk.proposal in _AUXILIARY:
        if delta is None:
            raise ValueError("delta is required")
        shd_h = np.sqrt(0.5 * np.asarray(delta, np.float64)) * np.ones(T)  # csmc/generic.py:61-63
        shd = handle.to_device(shd_h, dtype)
    # jax compat, the plain cSMC kernel: its draws are made by the model's own M0.sample / Mt.sample in the reference -- one normal(key, (N, d)) per call in every
    # model the reference defines, which is what the device proposal kernels apply their Cholesky factors to (random.jax_csmc_noise; the reference draws the same
    # shapes for the independent and the guided kernel)
    nz, keep = _noise(handle, dtype, Cn, key, noise, dict(eps_prop=(Cn, T, N, d), u_res=(Cn, max(T - 1, 0), N), u_bwd=(Cn, T), eps_aux=(Cn, T, d)),
                      lambda k_: _random.jax_csmc_noise(k_, T, N, d, dtype, bool(backward), handle, auxiliary=fk.proposal in _AUXILIARY))
    hist = None
    xs = lws = As = None
    if want_history:
        xs = handle.empty((Cn, T, N, d), dtype)
        lws = handle.empty((Cn, T, N), dtype)
        As = handle.zeros((Cn, max(T - 1, 1), N), np.int32)
    dyn = None
    if chain_dynamics is not None:
        dbuf = [handle.to_device(np.asarray(a, np.float64).reshape(shp), dtype) for a, shp in zip(chain_dynamics, ((Cn, d, d), (Cn, d), (Cn, d, d)))]
        dyn = _lib.FkChainDynamics(*(a.ptr.value for a in dbuf))
    _csmc_call(handle, fk, dtype, m, Cn, T, N, backward, shd, xd, nz, anc, xs, lws, As, dyn)
    xo, ao = xd.to_host(), anc.to_host()
    if want_history:
        hist = dict(xs=xs.to_host(), log_ws=lws.to_host(), As=As.to_host()[:, :T - 1])
        if single:
            hist = {k_: v[0] for k_, v in hist.items()}
    return (xo[0], ao[0], hist) if single else (xo, ao, hist)
