"""CPU: per-chain dynamics in the cSMC sweep (particle Gibbs over (x, F, b, Q)) as far as a host without a GPU can see it.
  1. auxssm_csmc_sweep_chain_dynamics and auxssm_csmc_dynamics_commit are declared in include/auxssm.h, exported by the library and bound with the declared
     number of arguments; the ctypes struct FkChainDynamics has the header's fields in the header's order.
  2. the commit's per-chain body (csrc/chain_dynamics.h, compiled by g++: tests/hostsim_chain_dynamics) against the NumPy restatement below -- the same IEEE
     operations in the same order, so every output is compared with assert_array_equal: committed chains, a chain the update flagged, a Q that is positive
     definite in double and not once rounded to float32 (flag 5, the live quadruple untouched), non-finite staging entries.
  3. what DynamicsThetaStep refuses in its constructor, and which chains each kind of step asks for."""
import ctypes as C
import os
import re

import numpy as np
import numpy.testing as npt
import pytest

from tests import dynamics_theta_np as NP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("auxssm_csmc_sweep_chain_dynamics", "auxssm_csmc_dynamics_commit")


def _header():
    return open(os.path.join(ROOT, "include", "auxssm.h")).read()


def _declaration(name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", _header())
    assert m, f"{name} is not declared in include/auxssm.h"
    return [a.strip() for a in m.group(1).split(",")]


# ---- 1. the C ABI ----------------------------------------------------------------------------------------------------------------------------------------
def test_the_two_symbols_are_declared_exported_and_bound():
    from aux_ssm_samplers_amd import _lib
    lib = _lib.load()
    for name in SYMBOLS:
        args = _declaration(name)
        assert hasattr(lib, name), f"{name} declared in include/auxssm.h but not exported"
        assert name in _lib.exported_symbols()
        assert len(getattr(lib, name).argtypes) == len(args), (name, args)
    sweep, shared = _declaration("auxssm_csmc_sweep_chain_dynamics"), _declaration("auxssm_csmc_sweep")
    norm = lambda a: re.sub(r"\s+", " ", a)  # noqa: E731
    # (h, dtype, model, dyn, then exactly auxssm_csmc_sweep's arguments from C on)
    assert [norm(a) for a in sweep[:3]] == [norm(a) for a in shared[:3]]
    assert norm(sweep[3]) == "const auxssm_fk_chain_dynamics* dyn"
    assert [norm(a) for a in sweep[4:]] == [norm(a) for a in shared[3:]]
    assert [norm(a).split()[-1].lstrip("*") for a in _declaration("auxssm_csmc_dynamics_commit")] == \
        ["h", "dtype", "C", "dx", "F_new", "b_new", "Q_new", "step_flags", "F", "b", "Q", "chol_Q", "flags"]
    assert lib.auxssm_version() == 108


def test_the_ctypes_struct_is_the_header_struct():
    from aux_ssm_samplers_amd import _lib
    m = re.search(r"typedef struct \{([^}]*)\} auxssm_fk_chain_dynamics;", _header())
    assert m, "auxssm_fk_chain_dynamics is not defined in include/auxssm.h"
    fields = re.findall(r"const void\*\s*(\w+)\s*;", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert fields == ["F", "b", "chol_Q"]
    assert [f[0] for f in _lib.FkChainDynamics._fields_] == fields
    vp = C.sizeof(C.c_void_p)
    assert C.sizeof(_lib.FkChainDynamics) == 3 * vp
    assert [getattr(_lib.FkChainDynamics, f).offset for f in fields] == [0, vp, 2 * vp]
    # the model struct did not grow: the new arrays have a struct of their own
    assert C.sizeof(_lib.FkModelObs) == 136 and _lib.FkModelObs.obs_const.offset == 128


def test_the_entry_points_refuse_bad_arguments_without_a_device():
    """the refusals that come before the handle is used for anything: a NULL handle, and (past it) nothing else can be checked without a GPU"""
    from aux_ssm_samplers_amd import _lib
    lib = _lib.load()
    rc = lib.auxssm_csmc_dynamics_commit(None, _lib.F64, 1, 1, None, None, None, None, None, None, None, None, None)
    assert rc == _lib.ERR_ARG
    m, nz, dyn = _lib.FkModelObs(), _lib.CsmcNoise(), _lib.FkChainDynamics()
    assert lib.auxssm_csmc_sweep_chain_dynamics(None, _lib.F64, C.byref(m), C.byref(dyn), 1, 2, 2, 1, None, None, C.byref(nz), None, None, None, None) == _lib.ERR_ARG
    assert lib.auxssm_csmc_sweep_chain_dynamics(None, _lib.F64, C.byref(m), None, 1, 2, 2, 1, None, None, C.byref(nz), None, None, None, None) == _lib.ERR_ARG
    assert "dyn is NULL" in lib.auxssm_last_error().decode()


# ---- 2. the commit body ----------------------------------------------------------------------------------------------------------------------------------
def _chol_np(a):
    """csrc/dynamics_theta.h::dt_chol operation by operation on Python floats (IEEE doubles, one rounding per operation): the factor, or None"""
    n = a.shape[0]
    l = [[0.0] * n for _ in range(n)]
    for j in range(n):
        d = float(a[j, j])
        for k in range(j):
            d -= l[j][k] * l[j][k]
        if not (d > NP.PIVOT_TOL * float(a[j, j])) or not np.isfinite(d):
            return None
        dj = float(np.sqrt(np.float64(d)))
        l[j][j] = dj
        for i in range(j + 1, n):
            s = float(a[i, j])
            for k in range(j):
                s -= l[i][k] * l[j][k]
            l[i][j] = s / dj
    return np.array(l, np.float64)


def commit_np(F_new, b_new, Q_new, step_flags, F, b, Q, chol_Q):
    """the restatement of csrc/chain_dynamics.h::cd_commit, chain by chain, in the arrays' own dtype"""
    dtype = F.dtype
    F, b, Q, LQ = (np.array(a, dtype) for a in (F, b, Q, chol_Q))
    flags = np.zeros(len(b), np.int32)
    for c in range(len(b)):
        if step_flags[c] != 0:
            flags[c] = step_flags[c]
            continue
        fin = np.all(np.isfinite(Q_new[c])) and np.all(np.isfinite(F_new[c])) and np.all(np.isfinite(b_new[c]))
        l = _chol_np(Q_new[c].astype(np.float64)) if fin else None
        if l is None:
            flags[c] = 5
            continue
        with np.errstate(over="ignore", under="ignore"):
            lr = l.astype(dtype)
        if not np.all(np.isfinite(lr)) or not np.all(np.diag(lr) > 0):
            flags[c] = 5
            continue
        F[c], b[c], Q[c], LQ[c] = F_new[c], b_new[c], Q_new[c], lr
    return F, b, Q, LQ, flags


def _staging(d, Cn, dtype, seed):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((Cn, d, d))
    Qn = (A @ np.swapaxes(A, 1, 2) + 0.1 * np.eye(d)).astype(dtype)
    Qn = np.maximum(Qn, np.swapaxes(Qn, 1, 2))       # symmetric in dtype, as the update writes it
    live = (np.full((Cn, d, d), 0.5, dtype), np.full((Cn, d), -1.0, dtype), np.tile(np.eye(d, dtype=dtype), (Cn, 1, 1)), np.tile(2 * np.eye(d, dtype=dtype), (Cn, 1, 1)))
    return rng.standard_normal((Cn, d, d)).astype(dtype), rng.standard_normal((Cn, d)).astype(dtype), Qn, live


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_commit_body_equals_the_restatement(d, dtype):
    from tests import hostsim_chain_dynamics as HS
    Cn = 9
    Fn, bn, Qn, live = _staging(d, Cn, dtype, 50 + d)
    sf = np.zeros(Cn, np.int32)
    sf[2], sf[5] = 2, 4                              # two chains the update flagged: their staging values are stale and must not be read
    Qn[2] = np.nan
    Fn[6, 0, 0] = np.inf                             # non-finite staging entries of unflagged chains
    bn[7, d - 1] = np.nan
    Qn[8] = -Qn[8]                                   # not positive definite at all
    got = HS.commit(Fn, bn, Qn, sf, *live)
    want = commit_np(Fn, bn, Qn, sf, *live)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype
        npt.assert_array_equal(g, w)
    F, b, Q, LQ, flags = got
    npt.assert_array_equal(flags, [0, 0, 2, 0, 0, 4, 5, 5, 5])
    for c in (2, 5, 6, 7, 8):                        # refused chains: the whole live quadruple as it was
        for g, l in zip((F, b, Q, LQ), live):
            npt.assert_array_equal(g[c], l[c])
    for c in (0, 1, 3, 4):                           # committed chains: the staging values, and a factor of the live Q to rounding
        npt.assert_array_equal(F[c], Fn[c])
        npt.assert_array_equal(b[c], bn[c])
        npt.assert_array_equal(Q[c], Qn[c])
        assert np.all(np.triu(LQ[c], 1) == 0)
        L = LQ[c].astype(np.float64)
        # L = chol(Q) in double (backward error d eps64 |L| |L|^T) rounded to dtype (relative 2^-24 / 2^-53 per entry: 2 eps |L| |L|^T in the product)
        eps = float(np.finfo(dtype).eps)
        npt.assert_array_less(np.abs(L @ L.T - Q[c].astype(np.float64)), (2 * eps + 8 * 2.0 ** -52) * (np.abs(L) @ np.abs(L).T) + 1e-300)
    assert np.all(np.isfinite(LQ)) and np.all(np.isfinite(F)) and np.all(np.isfinite(Q))


def test_a_q_that_loses_definiteness_in_float32_is_flag_5():
    """[[1, 1 - 1e-9], [1 - 1e-9, 1]] is positive definite in double (second pivot 2e-9, far above 2^-46) and the all-ones matrix in float32 (pivot 0): the double
    commit takes it, the float32 commit refuses it with 5 and leaves the live quadruple untouched; the chain next to it commits"""
    from tests import hostsim_chain_dynamics as HS
    d, Cn = 2, 2
    near = np.array([[1.0, 1.0 - 1e-9], [1.0 - 1e-9, 1.0]])
    assert NP.chol_checked(near) is not None and NP.chol_checked(near.astype(np.float32).astype(np.float64)) is None
    for dtype, want in ((np.float64, 0), (np.float32, 5)):
        Fn, bn, Qn, live = _staging(d, Cn, dtype, 7)
        Qn[0] = near.astype(dtype)
        F, b, Q, LQ, flags = HS.commit(Fn, bn, Qn, np.zeros(Cn, np.int32), *live)
        npt.assert_array_equal(flags, [want, 0])
        for g, w in zip((F, b, Q, LQ, flags), commit_np(Fn, bn, Qn, np.zeros(Cn, np.int32), *live)):
            npt.assert_array_equal(g, w)
        if want:
            for g, l in zip((F, b, Q, LQ), live):
                npt.assert_array_equal(g[0], l[0])
        else:
            npt.assert_array_equal(Q[0], Qn[0])
        npt.assert_array_equal(Q[1], Qn[1])


def test_a_factor_that_underflows_in_float32_is_flag_5():
    """Q = 1e-80 is a positive float64 whose factor 1e-40 is a float32 subnormal ... and Q itself is 0 in float32: refused there; in float64 it commits"""
    from tests import hostsim_chain_dynamics as HS
    for dtype, want in ((np.float64, 0), (np.float32, 5)):
        Fn, bn, Qn, live = _staging(1, 1, dtype, 3)
        with np.errstate(under="ignore"):
            Qn[0, 0, 0] = dtype(1e-80)
        *_, flags = HS.commit(Fn, bn, Qn, np.zeros(1, np.int32), *live)
        assert flags[0] == want == commit_np(Fn, bn, Qn, np.zeros(1, np.int32), *live)[4][0]


# ---- 3. the Python layer ---------------------------------------------------------------------------------------------------------------------------------
def _prior(d):
    from aux_ssm_samplers_amd.loop import MNIWPrior
    return MNIWPrior(np.zeros((d, d + 1)), np.eye(d + 1), d + 2.0, np.eye(d))


def test_constructor_refusals_name_the_reason():
    from aux_ssm_samplers_amd.csmc import LinearGaussianDynamics, Lorenz63Dynamics
    from aux_ssm_samplers_amd.csmc.models import DeviceGaussianDynamics
    from aux_ssm_samplers_amd.loop import DynamicsThetaStep
    with pytest.raises(ValueError, match=r"Lorenz63Dynamics is parameterised by its drift"):
        DynamicsThetaStep(Lorenz63Dynamics(theta=[10.0, 28.0, 8.0 / 3.0], sigma_x=1.0, dt=0.01), _prior(3))
    with pytest.raises(ValueError, match=r"DeviceGaussianDynamics has a user-defined transition mean"):
        DynamicsThetaStep(DeviceGaussianDynamics(source="", Q=np.eye(2)), _prior(2))
    T = 5
    tv = LinearGaussianDynamics(F=np.tile(0.5 * np.eye(2), (T - 1, 1, 1)), b=np.zeros((T - 1, 2)), Q=np.tile(np.eye(2), (T - 1, 1, 1)))
    with pytest.raises(ValueError, match=r"varies in time"):
        DynamicsThetaStep(tv, _prior(2))
    with pytest.raises(ValueError, match=r"dx <= 4 \(the model has dx = 5\)"):
        DynamicsThetaStep(LinearGaussianDynamics(F=0.5 * np.eye(5), b=np.zeros(5), Q=np.eye(5)), _prior(4))
    with pytest.raises(ValueError, match=r"the prior is for d = 3, the model has dx = 2"):
        DynamicsThetaStep(LinearGaussianDynamics(F=0.5 * np.eye(2), b=np.zeros(2), Q=np.eye(2)), _prior(3))
    with pytest.raises(ValueError, match=r"prior must be an MNIWPrior"):
        DynamicsThetaStep(LinearGaussianDynamics(F=[[0.5]], b=[0.0], Q=[[1.0]]), None)
    step = DynamicsThetaStep(LinearGaussianDynamics(F=[[0.9]], b=[0.0], Q=[[2.0]]), _prior(1))   # (scalars as nested lists, the SV example's form)
    assert step.dx == 1


def test_each_kind_of_step_says_which_chains_it_needs():
    """a step built on a Kalman-sampler model given cSMC chains, and the reverse: ValueError naming the chains the step needs (no device: the chains are bare
    instances, the check comes before anything touches them)"""
    from aux_ssm_samplers_amd.csmc import LinearGaussianDynamics
    from aux_ssm_samplers_amd.csmc._device import CsmcChains
    from aux_ssm_samplers_amd.kalman import LGConcatModel
    from aux_ssm_samplers_amd.kalman.generic import DeviceChains
    from aux_ssm_samplers_amd.loop import DynamicsThetaStep, LorenzThetaStep
    from aux_ssm_samplers_amd.workloads import lg_model
    T, d = 6, 2
    m = lg_model(T, d)
    bt = np.broadcast_to
    model = LGConcatModel(m["m0"], m["P0"], bt(m["F"], (T - 1, d, d)), bt(m["Q"], (T - 1, d, d)), bt(m["b"], (T - 1, d)), bt(m["Hobs"], (T, d, d)),
                          bt(m["Robs"], (T, d, d)), bt(m["cobs"], (T, d)), m["y"])
    key = np.array([1, 2], np.uint32)
    csmc_chains, kalman_chains = object.__new__(CsmcChains), object.__new__(DeviceChains)
    kalman_step = DynamicsThetaStep(model, _prior(d))
    for call in (lambda: kalman_step(key, csmc_chains), lambda: kalman_step.params(csmc_chains)):
        with pytest.raises(ValueError, match=r"needs kalman\.DeviceChains"):
            call()
    csmc_step = DynamicsThetaStep(LinearGaussianDynamics(F=m["F"], b=m["b"], Q=m["Q"]), _prior(d))
    for call in (lambda: csmc_step(key, kalman_chains), lambda: csmc_step.params(kalman_chains)):
        with pytest.raises(ValueError, match=r"needs csmc\.CsmcChains"):
            call()
    with pytest.raises(ValueError, match=r"LorenzThetaStep.*needs kalman\.DeviceChains"):
        LorenzThetaStep(None, 1.0)(key, csmc_chains)
