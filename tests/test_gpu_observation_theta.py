"""GPU: the conjugate step on the observation model (H, c, R) of an LGConcatModel (csrc/observation_theta.hip, loop.ObservationThetaStep) against the literal
restatement tests/observation_theta_np.py.  Cells: (dx, dy) in {1, 4} x {1, 4} plus (2, 3) and (3, 2); T = 2, 3, a segment less one, a segment, a segment plus
one, three segments and a ragged tail; C = 1, 3, 33, 70; each layout forced through DeviceChains(chain_minor=...); float64 and float32 states; rows of y missing
at the first step, at the last step and in a run across the 512-step edge.
  1. auxssm_observation_stats, post_out and the explicit-noise draws (H, c, R)   fp64 at 1e-9 relative (to the largest entry of each matrix); fp32 states against
     the restatement on the same float32-rounded inputs at FP32_*_BAR (measured: see there)
  2. a chain alone = the chain in its batch, bit for bit
  3. R alone: H, c keep their bits, R against the restatement
  4. contained failure: flags 1 - 4, the chain's three arrays keep their bits, the other chains of the call update
  5. the sweep behind the step: the C-chain sweep on per-chain observation models = one-chain sweeps of fresh models built from them; with a DynamicsThetaStep
     on the same model in either order of first use; chain-minor chains and another chain count are refused before any launch
  6. (tests/test_observation_theta_host.py: the new kernels use no scratch, by the compiler's remarks)
  7. moments of the step: 4096 chains on one trajectory, one keyed call
  8. joint ground truth: loop() over (x, H, c, R) against quadrature (tests/golden/observation_theta_quadrature.json)"""
import ctypes as C
import functools
import json
import os

import numpy as np
import numpy.testing as npt
import pytest

from tests import observation_theta_cases as OC, observation_theta_np as NP

pytestmark = pytest.mark.gpu

L = NP.SEGMENT_LEN
DIMS = [(1, 1), (1, 4), (4, 1), (4, 4), (2, 3), (3, 2)]
T_CASES = [2, 3, L - 1, L, L + 1, 3 * L + 38]
C_CASES = [1, 3, 33, 70]
C_MAX = 70
FP64_BAR = 1e-9
# float32 states against the restatement on the same float32-rounded inputs; each bar is twice the worst error measured over every cell, rounded up.  The sums are
# formed in double from the float32 values, so the statistics and the posterior are as accurate as for float64 states: measured worst 3.85e-15 (statistics) and
# 1.36e-13 (posterior; float64 states: 3.59e-15 and 1.30e-13).  The draws are rounded to float32 on the way out: measured 0 -- every entry equal to the restatement's
# rounded to float32 -- so that bar is rounded up to 2^-24 of the largest entry, one float32 rounding step, the smallest error above 0 the comparison can show.
FP32_STATS_BAR = 8e-15
FP32_POST_BAR = 3e-13
FP32_DRAW_BAR = 2.0 ** -24


@pytest.fixture(scope="module")
def handle():
    from aux_ssm_samplers_amd import _lib
    return _lib.default_handle()


def missing_rows(T):
    """the first step (T >= 3), the last step (T == 2 or T >= 511) and a run across the 512-step edge"""
    if T == 2:
        return (1,)
    if T == 3:
        return (0,)
    return tuple(sorted({0, T - 1} | {t for t in range(L - 4, L + 4) if t < T - 1}))


def _round(a, f32):
    return np.asarray(a, np.float32).astype(np.float64) if f32 else np.asarray(a, np.float64)


@functools.lru_cache(maxsize=None)
def cell(dx, dy, T, f32):
    """the problem of one (dx, dy, T) for C_MAX chains, its explicit noise, and the restatement's statistics, posterior and draws -- on the float32-rounded
    inputs when f32.  Computed once and shared; nothing in it is changed by a test"""
    p = OC.problem(dx, dy, T, 1000 * dx + 100 * dy + T, missing=missing_rows(T), C=C_MAX)
    x, y = _round(p["x"], f32), _round(p["y"], f32)
    nobs = int(NP.observed(y).sum())
    chi, ew, ea = (_round(a, f32) for a in OC.noise(dx, dy, 7 * dx + dy + T, p["nu0"] + nobs, (C_MAX,)))
    H0, c0, R0 = _round(p["H"], f32), _round(p["c"], f32), _round(p["R"], f32)
    syy, _ = NP.data_terms(y)
    S = NP.stats(x, y)
    post = NP.posterior_joint(S, syy, nobs, p["M0"], p["K0"], p["nu0"], p["Psi0"])
    R, A = NP.draw(post, chi, ew, ea)
    A0 = np.concatenate([H0, c0[:, None]], axis=1)
    post_r = NP.posterior_r(S, syy, nobs, p["nu0"], p["Psi0"], np.broadcast_to(A0, (C_MAX,) + A0.shape))
    R_alone = NP.draw_r(post_r[3], chi, ew)
    for a in (x, y, chi, ew, ea, R, A, R_alone):
        a.setflags(write=False)
    return dict(p=p, x=x, y=y, nobs=nobs, chi=chi, ew=ew, ea=ea, H0=H0, c0=c0, R0=R0, syy_nobs=NP.syy_nobs(y), stats=NP.stats_flat(x, y), post=NP.post_flat(post),
                R=R, A=A, post_r=NP.post_flat(post_r), R_alone=R_alone)


def _prior(p, chi_scale=1.0, **over):
    from aux_ssm_samplers_amd.loop import ObsMNIWPrior
    q = dict(p, **over)
    return ObsMNIWPrior(q["M0"], q["K0"], q["nu0"], q["Psi0"]).struct(chi_scale)


def _device_update(handle, cl, x, dtype, chain_minor, mask=1, prior=None, chi=None, y=None, first=0):
    """-> (stats, post, flags, H, c, R) as host arrays for the chains x (C, T, dx) with the cell's explicit noise (rows first .. first + C of it)"""
    from aux_ssm_samplers_amd.kalman.generic import DeviceChains
    Cn, T, dx = x.shape
    y = cl["y"] if y is None else y
    dy, n = y.shape[1], dx + 1
    chains = DeviceChains(handle, x, dtype, chain_minor=chain_minor)
    assert chains.chain_minor == chain_minor
    ybuf = handle.to_device(y, dtype)
    yarr = ybuf.arr(0, dy, 0)
    stats = handle.observation_stats(chains.x, yarr, dy, chains.layout).to_host()
    rep = lambda a: handle.to_device(np.repeat(np.asarray(a)[None], Cn, axis=0), dtype)
    H, c, R = rep(cl["H0"]), rep(cl["c0"]), rep(cl["R0"])
    post = handle.zeros((Cn, dy * n + n * n + 1 + dy * dy), np.float64)
    flags = handle.to_device(np.full(Cn, -1, np.int32))
    sl = slice(first, first + Cn)
    chi = cl["chi"] if chi is None else chi
    syy_nobs = cl["syy_nobs"] if y is cl["y"] else NP.syy_nobs(_round(y, np.dtype(dtype) == np.float32))
    handle.observation_theta_update(chains.x, yarr, dy, syy_nobs, prior or _prior(cl["p"]), mask, handle.to_device(chi[sl], dtype),
                                    handle.to_device(cl["ew"][sl], dtype), handle.to_device(cl["ea"][sl], dtype), H.arr(dy * dx, 0, 0), c.arr(dy, 0, 0),
                                    R.arr(dy * dy, 0, 0), flags, post_out=post, layout=chains.layout)
    return stats, post.to_host(), flags.to_host(), H.to_host(), c.to_host(), R.to_host()


def _blocks(dx, dy):
    """column slices of the statistics' and the posterior's matrices"""
    n = dx + 1
    sb = [slice(0, n * n), slice(n * n, n * n + dy * n)]
    o = [0, dy * n, dy * n + n * n, dy * n + n * n + 1, dy * n + n * n + 1 + dy * dy]
    return sb, [slice(o[i], o[i + 1]) for i in range(4)]


def _rel_rows(got, want):
    """worst over the chains of (largest difference / the reference's largest entry) of one matrix per row"""
    got, want = np.asarray(got, np.float64).reshape(len(got), -1), np.asarray(want, np.float64).reshape(len(want), -1)
    return float(np.max(np.max(np.abs(got - want), axis=1) / np.max(np.abs(want), axis=1)))


# ---- 1. statistics, posterior and draws ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain_minor", [False, True], ids=["dense", "chain_minor"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("dx,dy", DIMS)
def test_statistics_posterior_and_draws(handle, dx, dy, dtype, chain_minor):
    f32 = dtype == np.float32
    sb, pb = _blocks(dx, dy)
    worst = dict(stats=0.0, post=0.0, draw=0.0)
    for T in T_CASES:
        cl = cell(dx, dy, T, f32)
        for Cn in C_CASES:
            stats, post, flags, H, c, R = _device_update(handle, cl, cl["x"][:Cn], dtype, chain_minor)
            assert not flags.any(), (T, Cn, flags)
            for s in sb:
                worst["stats"] = max(worst["stats"], _rel_rows(stats[:, s], cl["stats"][:Cn, s]))
            for s in pb:
                worst["post"] = max(worst["post"], _rel_rows(post[:, s], cl["post"][:Cn, s]))
            A = np.concatenate([H, c[:, :, None]], axis=2)
            wR, wA = (cl["R"][:Cn].astype(dtype), cl["A"][:Cn].astype(dtype)) if f32 else (cl["R"][:Cn], cl["A"][:Cn])
            worst["draw"] = max(worst["draw"], _rel_rows(R, wR), _rel_rows(A, wA))
            npt.assert_array_equal(R, np.swapaxes(R, 1, 2))
            assert R.dtype == dtype and np.all(np.isfinite(R)) and np.all(np.isfinite(A))
            assert np.all(stats[:, dx * (dx + 1) + dx] == cl["nobs"])       # So_zz[dx, dx] is the number of observed rows, exactly
    print(f"observation_theta dx={dx} dy={dy} {np.dtype(dtype).name} {'chain-minor' if chain_minor else 'dense'}: worst relative error stats {worst['stats']:.2e} "
          f"post {worst['post']:.2e} draw {worst['draw']:.2e}")
    assert worst["stats"] <= (FP32_STATS_BAR if f32 else FP64_BAR)
    assert worst["post"] <= (FP32_POST_BAR if f32 else FP64_BAR)
    assert worst["draw"] <= (FP32_DRAW_BAR if f32 else FP64_BAR)


# ---- 2. batch independence ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain_minor", [False, True], ids=["dense", "chain_minor"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_a_chain_alone_is_the_chain_in_its_batch(handle, dtype, chain_minor):
    """a chain alone, as member 2 of 3 and as member 40 of 70: the same bits in stats_out, post_out and the written H, c, R"""
    dx, dy, T = 4, 4, 3 * L + 38
    cl = cell(dx, dy, T, dtype == np.float32)
    for first, count, member in ((0, 70, 39), (38, 3, 1)):   # (chain 39 of the cell is member 40 of all 70 and member 2 of chains 38 .. 40)
        batch = _device_update(handle, cl, cl["x"][first:first + count], dtype, chain_minor, first=first)
        alone = _device_update(handle, cl, cl["x"][39:40], dtype, chain_minor, first=39)
        assert first + member == 39
        for got, want in zip(alone, batch):
            npt.assert_array_equal(got[0], want[member])


# ---- 3. R alone ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain_minor", [False, True], ids=["dense", "chain_minor"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("dx,dy", DIMS)
def test_r_alone_leaves_h_and_c(handle, dx, dy, dtype, chain_minor):
    f32 = dtype == np.float32
    _, pb = _blocks(dx, dy)
    for T, Cn in ((3, 3), (L + 1, 33)):
        cl = cell(dx, dy, T, f32)
        nan_prior = _prior(cl["p"])
        for k in range(20):
            nan_prior.M0[k] = float("nan")      # M0 and K0 are not read
        for k in range(25):
            nan_prior.K0[k] = float("nan")
        stats, post, flags, H, c, R = _device_update(handle, cl, cl["x"][:Cn], dtype, chain_minor, mask=2, prior=nan_prior)
        assert not flags.any()
        npt.assert_array_equal(H, np.repeat(cl["H0"][None], Cn, axis=0).astype(dtype))
        npt.assert_array_equal(c, np.repeat(cl["c0"][None], Cn, axis=0).astype(dtype))
        for s in pb:
            assert _rel_rows(post[:, s], cl["post_r"][:Cn, s]) <= (FP32_POST_BAR if f32 else FP64_BAR)
        want = cl["R_alone"][:Cn].astype(dtype) if f32 else cl["R_alone"][:Cn]
        assert _rel_rows(R, want) <= (FP32_DRAW_BAR if f32 else FP64_BAR)
        npt.assert_array_equal(R, np.swapaxes(R, 1, 2))


# ---- 4. contained failure ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain_minor", [False, True], ids=["dense", "chain_minor"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("dx,dy", [(1, 1), (4, 4), (3, 2)])
def test_a_failed_chain_keeps_its_parameters(handle, dx, dy, dtype, chain_minor):
    """chain 1 of 3 fails with each flag in turn; its H, c, R keep their bits, nothing non-finite is written, and chains 0 and 2 are drawn as usual.  With every
    row of y missing all three chains raise flag 1."""
    f32 = dtype == np.float32
    T, n = 40, dx + 1
    cl = cell(dx, dy, T, f32)
    p = cl["p"]
    keep = [np.repeat(np.asarray(a)[None], 3, axis=0).astype(dtype) for a in (cl["H0"], cl["c0"], cl["R0"])]

    def check(out, want, modes_updated=True):
        stats, post, flags, H, c, R = out
        assert flags[1] == want, (flags, want)
        for got, k in zip((H, c, R), keep):
            npt.assert_array_equal(got[1], k[1])
            assert np.all(np.isfinite(got))
        assert np.all(np.isfinite(post))
        if modes_updated:
            assert flags[0] == 0 and flags[2] == 0
            assert not np.array_equal(R[0], keep[2][0]) and not np.array_equal(R[2], keep[2][2])

    for mask in (1, 2):
        # flag 1: every row missing -- the data is shared, so every chain
        y = np.full((T, dy), np.nan)
        out = _device_update(handle, cl, cl["x"][:3], dtype, chain_minor, mask=mask, y=y)
        assert list(out[2]) == [1, 1, 1]
        check(out, 1, modes_updated=False)
        # flag 2: chain 1 and the data are an exact affine fit, the prior mean is that map, Psi0 vanishes
        xe, ye, Ae, Psi0 = OC.exact_fit(dx, dy, T)
        x = cl["x"][:3].copy()
        x[1] = xe
        fit = dict(cl, H0=Ae[:, :dx], c0=Ae[:, dx])
        keep_fit = [np.repeat(np.asarray(a)[None], 3, axis=0).astype(dtype) for a in (fit["H0"], fit["c0"], fit["R0"])]
        assert NP.step(xe, ye, Ae, np.eye(n), p["nu0"], Psi0, cl["chi"][1], cl["ew"][1], cl["ea"][1], mode=mask, A0=Ae)[0] == 2
        stats, post, flags, H, c, R = _device_update(handle, fit, x, dtype, chain_minor, mask=mask, y=ye, prior=_prior(p, M0=Ae, K0=np.eye(n), Psi0=Psi0))
        assert flags[1] == 2 and flags[0] == 0 and flags[2] == 0, flags
        for got, k in zip((H, c, R), keep_fit):
            npt.assert_array_equal(got[1], k[1])
            assert np.all(np.isfinite(got))
        assert not np.array_equal(R[0], keep_fit[2][0])
        # flag 3: a chi that is not positive
        chi = cl["chi"].copy()
        chi[1, dy - 1] = 0.0
        check(_device_update(handle, cl, cl["x"][:3], dtype, chain_minor, mask=mask, chi=chi), 3)
        # flag 4: a chi so small that R is not finite in the model's dtype
        chi = cl["chi"].copy()
        chi[1, 0] = 1e-44 if f32 else 1e-320
        check(_device_update(handle, cl, cl["x"][:3], dtype, chain_minor, mask=mask, chi=chi), 4)
    # flag 1 of ONE chain (joint mode): chain 1 never moves and K0 vanishes -- K_n = So_zz has rank one
    if dx >= 1:
        x = cl["x"][:3].copy()
        x[1] = 1.75 + np.arange(dx)
        K0 = 1e-200 * np.eye(n)
        assert NP.step(x[1], cl["y"], p["M0"], K0, p["nu0"], p["Psi0"], cl["chi"][1], cl["ew"][1], cl["ea"][1])[0] == 1
        check(_device_update(handle, cl, x, dtype, chain_minor, prior=_prior(p, K0=K0)), 1)


def test_the_entry_points_refuse_before_anything_is_enqueued(handle):
    """the C ABI itself (handle.lib): every refusal include/auxssm.h lists, each with its reason, the outputs untouched"""
    from aux_ssm_samplers_amd import _lib
    dx, dy, T, Cn = 2, 3, 9, 3
    n = dx + 1
    cl = cell(dx, dy, L - 1, False)
    lib, h = handle.lib, handle.h
    x = handle.to_device(cl["x"][:Cn, :T])
    ybuf = handle.to_device(cl["y"][:T])
    ya = ybuf.arr(0, dy, 0)
    stats = handle.to_device(np.full((Cn, n * n + dy * n), 7.0))
    chi, ew, ea = handle.to_device(cl["chi"][:Cn]), handle.to_device(cl["ew"][:Cn]), handle.to_device(cl["ea"][:Cn])
    rep = lambda a: handle.to_device(np.repeat(a[None], Cn, axis=0))
    H, c, R = rep(cl["H0"]), rep(cl["c0"]), rep(cl["R0"])
    flags = handle.to_device(np.full(Cn, -1, np.int32))
    Ha, ca, Ra = H.arr(dy * dx, 0, 0), c.arr(dy, 0, 0), R.arr(dy * dy, 0, 0)
    sn = NP.syy_nobs(cl["y"][:T])

    def refused(rc, why, code=_lib.ERR_ARG):
        assert rc == code, rc
        assert why in lib.auxssm_last_error().decode(), lib.auxssm_last_error().decode()

    def stats_call(Cn_=Cn, T_=T, dx_=dx, dy_=dy, layout=0, x_=x, y_=ya, out=stats):
        return lib.auxssm_observation_stats(h, _lib.F64, Cn_, T_, dx_, dy_, layout, x_.ptr if x_ is not None else None, C.byref(y_) if y_ is not None else None,
                                            out.ptr if out is not None else None)

    refused(stats_call(x_=None), "must be non-NULL")
    refused(stats_call(y_=None), "must be non-NULL")
    refused(stats_call(out=None), "stats_out must be non-NULL")
    refused(stats_call(layout=7), "layout must be")
    refused(stats_call(T_=1), "T >= 2")
    refused(stats_call(dx_=5), "1 <= dx <= 4 and 1 <= dy <= 4", _lib.ERR_UNSUPPORTED)
    refused(stats_call(dy_=5), "1 <= dx <= 4 and 1 <= dy <= 4", _lib.ERR_UNSUPPORTED)
    refused(stats_call(y_=ybuf.arr(T * dy, dy, 0)), "its chain stride must be 0")
    refused(stats_call(Cn_=65535 * 64 + 1, T_=2, dx_=1, layout=_lib.LAYOUT_CHAIN_MINOR), "C <= 4194240")
    refused(stats_call(Cn_=2 ** 30, T_=2 * L), "exceeds one launch")

    def update(prior=None, mask=1, chi_=chi, ea_=ea, H_=Ha, c_=ca, R_=Ra, flags_=flags, null_prior=False, sn_=sn, **kw):
        pr = prior or _prior(cl["p"])
        s = np.ascontiguousarray(sn_, np.float64) if sn_ is not None else None
        return lib.auxssm_observation_theta_update(h, _lib.F64, Cn, T, dx, dy, 0, x.ptr, C.byref(ya), s.ctypes.data_as(C.POINTER(C.c_double)) if s is not None else None,
                                                   None if null_prior else C.byref(pr), mask, chi_.ptr if chi_ is not None else None, ew.ptr,
                                                   ea_.ptr if ea_ is not None else None, C.byref(H_) if H_ is not None else None, C.byref(c_), C.byref(R_), None,
                                                   flags_.ptr if flags_ is not None else None)

    refused(update(null_prior=True), "must be non-NULL")
    refused(update(sn_=None), "must be non-NULL")
    refused(update(chi_=None), "must be non-NULL")
    refused(update(ea_=None), "must be non-NULL")
    refused(update(H_=None), "must be non-NULL")
    refused(update(flags_=None), "must be non-NULL")
    refused(update(mask=3), "update_mask must be 1")
    refused(update(mask=0), "update_mask must be 1")
    refused(update(H_=H.arr(dy * dx, 1, 0)), "time strides of H, c and R must be 0")
    refused(update(R_=R.arr(dy * dy, 2, 0)), "time strides of H, c and R must be 0")
    refused(update(H_=H.arr(0, 0, 0)), "every chain needs its own H, c, R")
    refused(update(c_=c.arr(dy - 1, 0, 0)), "every chain needs its own H, c, R")
    low = _prior(cl["p"])
    low.nu0 = dy - 1.0
    refused(update(prior=low), "nu0 > dy - 1")
    nan = _prior(cl["p"])
    nan.Psi0[0] = float("nan")
    refused(update(prior=nan), "non-finite")
    nan = _prior(cl["p"])
    nan.M0[0] = float("nan")
    refused(update(prior=nan), "non-finite")
    skew = _prior(cl["p"])
    skew.K0[1] += 0.25                       # K0[0, 1] != K0[1, 0]
    refused(update(prior=skew), "must be symmetric")
    indef = _prior(cl["p"])
    indef.Psi0[0], indef.Psi0[1], indef.Psi0[3], indef.Psi0[4] = 1.0, 2.0, 2.0, 1.0
    refused(update(prior=indef), "must be positive definite")
    indef = _prior(cl["p"], K0=np.eye(n))
    indef.K0[0] = -1.0
    refused(update(prior=indef), "must be positive definite")
    scale = _prior(cl["p"])
    scale.chi_scale = 0.0
    refused(update(prior=scale), "chi_scale must be positive")
    bad_sn = sn.copy()
    bad_sn[-1] = -1.0
    refused(update(sn_=bad_sn), "n_obs >= 0")
    handle.sync()
    npt.assert_array_equal(stats.to_host(), 7.0)
    npt.assert_array_equal(flags.to_host(), -1)
    npt.assert_array_equal(H.to_host(), np.repeat(cl["H0"][None], Cn, axis=0))
    npt.assert_array_equal(R.to_host(), np.repeat(cl["R0"][None], Cn, axis=0))
    assert update() == 0 and not flags.to_host().any()     # (and the same call with nothing wrong goes through)
    assert update(mask=2, ea_=None, prior=skew) == 0 and not flags.to_host().any()   # (R alone reads neither eps_a nor K0)


# ---- 5. the sweep behind the step ---------------------------------------------------------------------------------------------------------
def _lg(T, dx, dy, seed=4, H=None, c=None, R=None, F=None, b=None, Q=None, base=None):
    """an LGConcatModel with time-invariant parameters as broadcast views; base: another one whose data, initial state and unnamed parameters are kept"""
    from aux_ssm_samplers_amd.kalman import LGConcatModel
    bt = np.broadcast_to
    if base is None:
        p = OC.problem(dx, dy, T, seed, missing=(3,))
        F0 = 0.7 * np.eye(dx) + 0.05
        vals = dict(m0=np.zeros(dx), P0=np.eye(dx), F=F0, Q=0.3 * np.eye(dx) + 0.02, b=0.1 * np.ones(dx), H=p["H"], R=p["R"], c=p["c"], y=p["y"], x=p["x"])
    else:
        vals = dict(base.vals)
    for k, v in dict(H=H, c=c, R=R, F=F, b=b, Q=Q).items():
        if v is not None:
            vals[k] = np.asarray(v, np.float64)
    model = LGConcatModel(vals["m0"], vals["P0"], bt(vals["F"], (T - 1, dx, dx)), bt(vals["Q"], (T - 1, dx, dx)), bt(vals["b"], (T - 1, dx)),
                          bt(vals["H"], (T, dy, dx)), bt(vals["R"], (T, dy, dy)), bt(vals["c"], (T, dy)), vals["y"])
    model.vals = vals
    return model


def _obs_prior(model, dx, dy):
    """keeps the draws near the model's observation parameters"""
    from aux_ssm_samplers_amd.loop import ObsMNIWPrior
    v = model.vals
    return ObsMNIWPrior(np.concatenate([v["H"], v["c"][:, None]], axis=1), 50.0 * np.eye(dx + 1), dy + 60.0, 60.0 * v["R"])


@pytest.mark.parametrize("with_dynamics", [None, "dynamics_first", "observation_first"])
@pytest.mark.parametrize("dx,dy", [(2, 3), (4, 4), (1, 1)])
def test_the_sweep_reads_per_chain_observation_models(handle, dx, dy, with_dynamics):
    """after one step, an explicit-noise sweep of 3 dense chains = a one-chain sweep of a fresh model built from step.params(chains)[c], chain by chain: state and
    log alpha.  Also with a DynamicsThetaStep on the same model, in both orders of first use."""
    from aux_ssm_samplers_amd.kalman import get_kernel
    from aux_ssm_samplers_amd.kalman.generic import DeviceChains
    from aux_ssm_samplers_amd.loop import DynamicsThetaStep, MNIWPrior, ObservationThetaStep, ThetaSteps
    T, Cn, delta = 40, 3, 0.5
    model = _lg(T, dx, dy)
    v = model.vals
    rng = np.random.default_rng(17)
    x = v["x"][None] + 0.05 * rng.standard_normal((Cn, T, dx))
    noise = dict(eps_aux=rng.standard_normal((Cn, T, dx)), eps_samp=rng.standard_normal((Cn, T, dx)), u_accept=np.full(Cn, 0.5))
    init, kernel = get_kernel(model.dynamics_factory, model.observations_factory, model.log_likelihood_fn, True)
    chains = DeviceChains(handle, x, np.float64, chain_minor=False)
    obs = ObservationThetaStep(model, _obs_prior(model, dx, dy))
    dyn = DynamicsThetaStep(model, MNIWPrior(np.concatenate([v["F"], v["b"][:, None]], axis=1), 50.0 * np.eye(dx + 1), dx + 60.0, 60.0 * v["Q"]))
    key = np.array([3, 4], np.uint32)
    if with_dynamics is None:
        obs(key, chains)
    elif with_dynamics == "dynamics_first":
        ThetaSteps(dyn, obs)(key, chains)
    else:
        ThetaSteps(obs, dyn)(key, chains)
    assert not obs.flags(chains).any()
    Hc, cc, Rc = obs.params(chains)
    assert np.ptp(Hc, axis=0).max() > 0 and np.ptp(Rc, axis=0).max() > 0       # (the chains really hold different parameters)
    if with_dynamics is not None:
        assert not dyn.flags(chains).any()
        Fc, bc, Qc = dyn.params(chains)
        assert np.ptp(Fc, axis=0).max() > 0
    kernel(None, init(chains), delta, noise=noise)
    got_x, got_la = chains.to_host(), chains.logs.to_host()[:, 0]
    assert np.all(np.isfinite(got_x)) and np.all(np.isfinite(got_la))
    worst, bits = 0.0, True
    for k in range(Cn):
        over = dict(H=Hc[k], c=cc[k], R=Rc[k])
        if with_dynamics is not None:
            over.update(F=Fc[k], b=bc[k], Q=Qc[k])
        fresh = _lg(T, dx, dy, base=model, **over)
        i1, k1 = get_kernel(fresh.dynamics_factory, fresh.observations_factory, fresh.log_likelihood_fn, True)
        one = DeviceChains(handle, x[k:k + 1], np.float64, chain_minor=False)
        k1(None, i1(one), delta, noise={n_: a[k:k + 1] for n_, a in noise.items()})
        want_x, want_la = one.to_host()[0], one.logs.to_host()[0, 0]
        worst = max(worst, float(np.max(np.abs(got_x[k] - want_x)) / np.max(np.abs(want_x))), abs(got_la[k] - want_la) / max(1.0, abs(want_la)))
        bits = bits and np.array_equal(got_x[k], want_x) and got_la[k] == want_la
    print(f"sweep behind the observation step dx={dx} dy={dy} {with_dynamics}: worst error {worst:.2e}, equal to the bit: {bits}")
    assert worst <= FP64_BAR


def test_chain_minor_chains_and_another_chain_count_are_refused(handle):
    """the per-chain sweep serves the dense layout: the step refuses chain-minor chains with the reason, and so does the sweep entry itself; after the step made
    the model per-chain for 3 chains a sweep with 5 (resident or a host state) or 1 is refused before any launch, 3 still sweep"""
    from aux_ssm_samplers_amd import _lib
    from aux_ssm_samplers_amd.kalman import get_kernel
    from aux_ssm_samplers_amd.kalman.generic import DeviceChains
    from aux_ssm_samplers_amd.loop import ObservationThetaStep
    T, dx, dy = 30, 2, 2
    model = _lg(T, dx, dy)
    rng = np.random.default_rng(2)
    x = model.vals["x"][None] + 0.05 * rng.standard_normal((34, T, dx))
    init, kernel = get_kernel(model.dynamics_factory, model.observations_factory, model.log_likelihood_fn, True)
    step = ObservationThetaStep(model, _obs_prior(model, dx, dy))
    key = np.array([5, 6], np.uint32)
    cm = DeviceChains(handle, x, np.float64, chain_minor=True)
    with pytest.raises(ValueError, match="dense layout only .* chain_minor=False"):
        step(key, cm)
    kernel(key, init(cm), 0.5)     # (nothing was re-pointed: the chain-shared model still sweeps chain-minor chains)
    three = DeviceChains(handle, x[:3], np.float64, chain_minor=False)
    step(key, three)
    five = DeviceChains(handle, x[:5], np.float64, chain_minor=False)
    before = five.to_host()
    for state, count in ((five, 5), (x[:5], 5), (x[0], 1)):
        with pytest.raises(ValueError, match=f"per-chain observation model .* of 3 chains .* the chains are {count}"):
            kernel(key, init(state), 0.5)
    npt.assert_array_equal(five.to_host(), before)
    kernel(key, init(three), 0.5)
    assert np.all(np.isfinite(three.to_host()))
    # the sweep entry itself: chain strides on Hs / Rs / cs in the chain-minor layout, on a time-varying model, with per-chain data
    dl, ybuf, yarr = model.device(handle, np.float64)
    cm3 = DeviceChains(handle, x[:3], np.float64, chain_minor=True)
    dims = _lib.Dims(3, T, 1, dx, dy)

    def sweep(lg, ya, layout, ch):
        return handle.lib.auxssm_kalman_sweep(handle.h, _lib.F64, _lib.KMODEL_LG_CONCAT, C.byref(dims), C.byref(lg), C.byref(ya), 0.5, 1, 0, layout, ch._x.ptr,
                                              ch.eps_aux.ptr, ch.eps_samp.ptr, ch.u_acc.ptr, ch.accepted.ptr, ch.logs.ptr)

    def refused(rc, why):
        assert rc == _lib.ERR_ARG, rc
        assert why in handle.lib.auxssm_last_error().decode(), handle.lib.auxssm_last_error().decode()

    refused(sweep(dl.c, yarr, _lib.LAYOUT_CHAIN_MINOR, cm3), "in the dense layout")
    tv = _lib.Lgssm.from_buffer_copy(dl.c)
    tv.Hs = _lib.Arr(dl.c.Hs.ptr, dl.c.Hs.sc, dy * dx, 0)
    refused(sweep(tv, yarr, _lib.LAYOUT_DENSE, three), "must be time-invariant")
    refused(sweep(dl.c, _lib.Arr(yarr.ptr, 1, yarr.st, 0), _lib.LAYOUT_DENSE, three), "per-chain data is not supported")


# ---- 7. moments of the step -------------------------------------------------------------------------------------------------------------
def test_one_keyed_call_has_the_posterior_means(handle):
    from aux_ssm_samplers_amd.kalman.generic import DeviceChains
    from aux_ssm_samplers_amd.loop import ObservationThetaStep, ObsMNIWPrior
    N, T, dx, dy = 4096, 64, 2, 2
    model = _lg(T, dx, dy, seed=9)
    p = OC.problem(dx, dy, T, 9, missing=(3,))
    x, y = model.vals["x"], model.vals["y"]
    chains = DeviceChains(handle, np.broadcast_to(x, (N, T, dx)), np.float64, chain_minor=False)
    step = ObservationThetaStep(model, ObsMNIWPrior(p["M0"], p["K0"], p["nu0"], p["Psi0"]))
    step(np.array([11, 12], np.uint32), chains)
    assert not step.flags(chains).any()
    H, c, R = step.params(chains)
    syy, nobs = NP.data_terms(y)
    Mn, Kn, nun, Psi = NP.posterior_joint(NP.stats(x, y), syy, nobs, p["M0"], p["K0"], p["nu0"], p["Psi0"])
    A = np.concatenate([H, c[:, :, None]], axis=2)
    for got, want in ((A, Mn), (R, Psi / (nun - dy - 1))):
        se = got.std(axis=0, ddof=1) / np.sqrt(N)
        z = np.abs(got.mean(axis=0) - want) / se
        assert np.all(z <= 5), z.max()
    npt.assert_array_equal(R, np.swapaxes(R, 1, 2))
    with pytest.raises(ValueError, match="per-chain parameters of 4096 chains"):
        step(np.array([1, 2], np.uint32), DeviceChains(handle, np.broadcast_to(x, (3, T, dx)), np.float64, chain_minor=False))


# ---- 8. joint ground truth ---------------------------------------------------------------------------------------------------------------
def test_gibbs_over_state_and_observation_model_matches_quadrature(handle):
    """LGConcatModel, dx = dy = 1, T = 6, 2048 independent dense chains, 150 + 250 loop() sweeps with the ObservationThetaStep alone (F, b, Q fixed): the posterior
    means of H, c, log R, x_0 and x_5 against the quadrature of tests/golden/make_observation_theta_quadrature.py (which checks, on the CPU, that its mass at
    H < 0 is below 1e-6 and that halving its grid moves the means by less than 1e-8).  Standard errors from the spread of the per-chain averages; 4 of them."""
    from aux_ssm_samplers_amd.kalman import LGConcatModel, get_kernel
    from aux_ssm_samplers_amd.kalman.generic import DeviceChains
    from aux_ssm_samplers_amd.loop import ObservationThetaStep, ObsMNIWPrior, loop
    from tests.golden.make_observation_theta_quadrature import joint_model
    golden = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "observation_theta_quadrature.json")))
    assert golden["mass_H_negative"] < 1e-6 and golden["grid_halving_moves"] < 1e-8
    truth = np.array(golden["means"])
    j = joint_model()
    T, Cn, burn, keep = j["T"], 2048, 150, 250
    bt = np.broadcast_to
    one = lambda v, shape: bt(np.array(v, np.float64).reshape(shape[1:]), shape)
    model = LGConcatModel(np.array([j["m0"]]), np.array([[j["P0"]]]), one(j["F"], (T - 1, 1, 1)), one(j["Q"], (T - 1, 1, 1)), one(j["b"], (T - 1, 1)),
                          one(1.0, (T, 1, 1)), one(0.3, (T, 1, 1)), one(0.0, (T, 1)), j["y"][:, None])
    init, kernel = get_kernel(model.dynamics_factory, model.observations_factory, model.log_likelihood_fn, True)
    rng = np.random.default_rng(8)
    chains = DeviceChains(handle, 1.0 + 0.3 * rng.standard_normal((Cn, T, 1)), np.float64, chain_minor=False)
    step = ObservationThetaStep(model, ObsMNIWPrior(j["M0"], j["K0"], j["nu0"], j["Psi0"]))
    acc = np.zeros((Cn, 5))
    flagged = [0]

    def collect(i, state):
        if i < burn:
            return
        H, c, R = step.params(chains)
        x = chains.to_host()
        acc[:, 0] += H[:, 0, 0]
        acc[:, 1] += c[:, 0]
        acc[:, 2] += np.log(R[:, 0, 0])
        acc[:, 3] += x[:, 0, 0]
        acc[:, 4] += x[:, T - 1, 0]
        flagged[0] += int(step.flags(chains).any())

    loop(np.array([21, 22], np.uint32), 1.5, init(chains), kernel, None, burn + keep, theta_step=step, callback=collect)
    assert flagged[0] == 0
    per_chain = acc / keep
    mean, se = per_chain.mean(axis=0), per_chain.std(axis=0, ddof=1) / np.sqrt(Cn)
    z = np.abs(mean - truth) / se
    print("joint ground truth (H, c, log R, x_0, x_5): chains", mean, "quadrature", truth, "se", se, "z", z)
    assert np.all(z <= 4), z
