"""EM for linear-Gaussian state-space models on the device, against the literal NumPy restatement tests/lgssm_em_np.py:
  1. auxssm_kalman_smooth_stats behind the device filter and smoother: every block of stats_out and `cross`, fp64 at 1e-9 of the block's largest entry, for
     dx = 1..4, dy in {1, 3, 8}, T on either side of the 512-transition segment edge, 1 and 3 sequences, both scan modes, missing first / last rows and a run of
     missing rows across the segment edge; fp32 moments at FP32_BAR (measured: see there); a sequence alone = the sequence in its batch, bit for bit
  2. fit_em: the restatement's iterates and log-likelihoods at 1e-8, a log-likelihood that does not decrease, subsets of the blocks, the MAP fit, a block that
     cannot be solved keeps its bits and raises its flag while the others update
  3. smoothing_lag_one = filter_smoothing bit for bit, plus `cross`
  4. what the C entry points refuse."""
import ctypes as C

import numpy as np
import pytest

from tests import lgssm_em_np as E

pytestmark = pytest.mark.gpu

T_CASES = (2, 3, 511, 513, 514, 1574)   # 1, 2, 510 transitions: one segment; 512: exactly one; 513: a second segment of one transition; 1573: four segments
DIMS = [(dx, dy) for dx in (1, 2, 3, 4) for dy in (1, 3, 8)]
FP64_BAR = 1e-9
# fp32 moments (filter, smoother and `cross` in float32; products and sums in double) against the fp64 restatement on the same float32-rounded data and
# parameters, relative to each block's largest entry: twice the worst error measured over every cell of test_statistics_fp32 (1.20e-06, `cross` at dx = 1,
# dy = 8; the sums themselves: 1.01e-06), rounded up
FP32_BAR = 2.5e-6


@pytest.fixture(scope="module")
def handle():
    from aux_ssm_samplers_amd import _lib
    return _lib.default_handle()


def _missing(T, s):
    edge = [t for t in range(510, 516) if t < T]
    return sorted(set(([0] + edge, [T - 1], [0, T - 1] + edge)[s]))


def _cell(dx, dy, T, f32=False):
    """three sequences of one random model -> (parameters, ys (3, T, dy), restatement [(statistics, ell, moments)] per sequence)"""
    rng = np.random.default_rng(1000 * dx + 10 * dy + T)
    p = E.random_model(rng, dx, dy)
    ys = np.stack([E.simulate(rng, p, T, _missing(T, s))[1] for s in range(3)])
    if f32:
        p = {k: v.astype(np.float32).astype(np.float64) for k, v in p.items()}
        p["Q"], p["R"], p["P0"] = E.sym(p["Q"]), E.sym(p["R"]), E.sym(p["P0"])
        ys = ys.astype(np.float32).astype(np.float64)
    return p, ys, [E.e_step(ys[s], p) for s in range(3)]


def _device_e_step(handle, p, ys, dtype, parallel, moments=None):
    """filter, smoother and statistics pass for the sequences ys (S, T, dy) -> (stats (S, NS), cross (S, T - 1, dx, dx)); moments: host (ms, Ps, sms, sPs)
    lists to put in place of the device's own"""
    from aux_ssm_samplers_amd._primitives.kalman.em import _Fit
    fit = _Fit(handle, ys, p, dtype, parallel, 0)
    if moments is None:
        fit.filter(0)
        fit.smooth()
    else:
        for buf, a in zip((fit.ms, fit.Ps, fit.sms, fit.sPs), moments):
            buf.copy_from_host(np.asarray(a).reshape(buf.shape))
    cross = handle.empty((fit.S, fit.T - 1, 1, fit.dx, fit.dx), dtype)
    fit.statistics(cross)
    return fit.stats.to_host(), cross.to_host()[:, :, 0]


def _worst(stats, cross, ref, dx, dy):
    """largest error of a sequence's blocks, each relative to the block's largest entry in the restatement"""
    st, _, (ms, Ps, sms, sPs, X) = ref
    got = E.split(stats, dx, dy)
    errs = {k: float(np.max(np.abs(got[k] - st[k]))) / max(float(np.max(np.abs(st[k]))), 1e-300) for k in E.STAT_BLOCKS if np.max(np.abs(st[k])) > 0}
    for k in E.STAT_BLOCKS:
        if not np.max(np.abs(st[k])) > 0:
            assert not np.any(got[k]), k   # (no observed step: the block is exactly zero)
    errs["cross"] = float(np.max(np.abs(cross - X))) / float(np.max(np.abs(X)))
    assert np.array_equal(got["S_zz"], got["S_zz"].T) and np.array_equal(got["S_xx"], got["S_xx"].T) and np.array_equal(got["So_zz"], got["So_zz"].T)
    return errs


@pytest.mark.parametrize("dx,dy", DIMS)
def test_statistics_fp64(handle, dx, dy):
    worst = {}
    for T in T_CASES:
        p, ys, refs = _cell(dx, dy, T)
        for parallel in (True, False):
            for seqs in ((1,), (0, 1, 2)):
                stats, cross = _device_e_step(handle, p, ys[list(seqs)], np.float64, parallel)
                assert np.all(np.isfinite(stats)) and np.all(np.isfinite(cross))
                for row, s in enumerate(seqs):
                    assert stats[row, (dx + 1) ** 2 - 1] == T - 1   # the transition count, exactly
                    for k, e in _worst(stats[row], cross[row], refs[s], dx, dy).items():
                        worst[k] = max(worst.get(k, 0.0), e)
    print(f"lgssm_em statistics fp64 dx={dx} dy={dy}: worst relative error per block " + " ".join(f"{k} {e:.2e}" for k, e in worst.items()))
    assert max(worst.values()) <= FP64_BAR, worst


@pytest.mark.parametrize("dx,dy", DIMS)
def test_statistics_fp32(handle, dx, dy):
    worst = {}
    for T in (3, 513, 1574):
        p, ys, refs = _cell(dx, dy, T, f32=True)
        stats, cross = _device_e_step(handle, p, ys, np.float32, True)
        assert cross.dtype == np.float32 and np.all(np.isfinite(stats)) and np.all(np.isfinite(cross))
        for s in range(3):
            for k, e in _worst(stats[s], cross[s].astype(np.float64), refs[s], dx, dy).items():
                worst[k] = max(worst.get(k, 0.0), e)
    print(f"lgssm_em statistics fp32 dx={dx} dy={dy}: worst relative error per block " + " ".join(f"{k} {e:.2e}" for k, e in worst.items()))
    assert max(worst.values()) <= FP32_BAR, worst


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_batch_invariance(handle, dtype):
    """the same moments alone and as member 2 of 3: stats_out and cross bit for bit (the sums' order depends on T alone)"""
    dx, dy, T = 4, 8, 1574
    p, ys, refs = _cell(dx, dy, T)
    mom = [[refs[s][2][k] for s in range(3)] for k in range(4)]   # ms, Ps, sms, sPs of the three sequences
    stats3, cross3 = _device_e_step(handle, p, ys, dtype, True, moments=mom)
    stats1, cross1 = _device_e_step(handle, p, ys[1:2], dtype, True, moments=[m[1:2] for m in mom])
    assert np.array_equal(stats3[1], stats1[0]) and np.array_equal(cross3[1], cross1[0])
    assert not np.array_equal(stats3[0], stats3[1])


def _lgssm(p, T):
    from aux_ssm_samplers_amd._primitives.kalman import LGSSM
    dx, dy = p["m0"].shape[0], p["c"].shape[0]
    bt = np.broadcast_to
    return LGSSM(p["m0"], p["P0"], bt(p["F"], (T - 1, dx, dx)), bt(p["Q"], (T - 1, dx, dx)), bt(p["b"], (T - 1, dx)), bt(p["H"], (T, dy, dx)),
                 bt(p["R"], (T, dy, dy)), bt(p["c"], (T, dy)))


def _params(fitted):
    m0, P0, Fs, Qs, bs, Hs, Rs, cs = fitted
    return dict(m0=m0, P0=P0, F=Fs[0], Q=Qs[0], b=bs[0], H=Hs[0], R=Rs[0], c=cs[0])


def _compare_iterates(handle, ys_list, start, n_iter, tol, **kw):
    """fit_em stopped after k = 1 .. n_iter iterations against the restatement's k-th iterate; every ell of the longest fit"""
    from aux_ssm_samplers_amd._primitives.kalman import fit_em
    prior = kw.get("prior")
    its, ells_ref, flags_ref = E.em(ys_list, start, n_iter, update=kw.get("update", E.NAMES),
                                    prior=(prior.M0, prior.K0, prior.nu0, prior.Psi0) if prior is not None else None)
    assert not flags_ref.any()
    T = ys_list[0].shape[0]
    ys = ys_list[0] if len(ys_list) == 1 else np.stack(ys_list)
    worst = 0.0
    for k in range(1, n_iter + 1):
        fitted, ells, flags = fit_em(ys, _lgssm(start, T), k, handle=handle, **kw)
        assert not flags.any() and flags.shape == (k, 4) and ells.shape == (k + 1,)
        got = _params(fitted)
        for name in E.NAMES:
            worst = max(worst, float(np.max(np.abs(got[name] - its[k][name]))))
        for name in ("Q", "R", "P0"):
            if name in kw.get("update", E.NAMES):
                assert np.array_equal(got[name], got[name].T), name
    err_ell = float(np.max(np.abs(ells - ells_ref)))
    print(f"fit_em against the restatement, {n_iter} iterations: worst |parameter difference| {worst:.2e}, worst |ell difference| {err_ell:.2e} at |ell| "
          f"{np.max(np.abs(ells_ref)):.1f}")
    assert worst <= tol and err_ell <= tol, (worst, err_ell)
    assert np.all(np.diff(ells) >= -1e-9 * np.abs(ells[:-1])), np.diff(ells)
    return ells


@pytest.mark.parametrize("parallel", [True, False], ids=["parallel", "sequential"])
def test_fit_em_iterates(handle, parallel):
    ys, start, _ = E.em_problem()
    ells = _compare_iterates(handle, [ys], start, 10, 1e-8, parallel=parallel)
    assert ells[-1] > ells[0] + 1.0


def test_fit_em_three_sequences(handle):
    """the statistics of several sequences are pooled (restatement: a list of sequences)"""
    rng = np.random.default_rng(21)
    truth = E.random_model(rng, 3, 2)
    ys_list = [E.simulate(rng, truth, 120, missing=(5 * s,))[1] for s in range(3)]
    _compare_iterates(handle, ys_list, E.perturbed(rng, truth), 4, 1e-8)


def test_fit_em_from_the_truth(handle):
    from aux_ssm_samplers_amd._primitives.kalman import fit_em
    rng = np.random.default_rng(3)
    truth = E.random_model(rng, 1, 1)
    _, ys = E.simulate(rng, truth, 2000)
    _, ells, flags = fit_em(ys, _lgssm(truth, 2000), 10, handle=handle)
    assert not flags.any()
    assert ells[-1] >= ells[0]
    assert np.all(np.diff(ells) >= -1e-9 * np.abs(ells[:-1])), np.diff(ells)


def test_fit_em_subsets_and_map(handle):
    from aux_ssm_samplers_amd._primitives.kalman import fit_em
    from aux_ssm_samplers_amd.loop import MNIWPrior
    ys, start, _ = E.em_problem()
    T, dx = ys.shape[0], start["m0"].shape[0]
    fitted, ells, flags = fit_em(ys, _lgssm(start, T), 5, update=("H", "c", "R"), handle=handle)
    got = _params(fitted)
    for name in ("F", "b", "Q", "m0", "P0"):
        assert np.array_equal(got[name], start[name]), name
    for name in ("H", "c", "R"):
        assert not np.array_equal(got[name], start[name]), name
    assert not flags.any() and ells[-1] > ells[0]
    _compare_iterates(handle, [ys], start, 5, 1e-8, update=("H", "c", "R"))
    rng = np.random.default_rng(9)
    prior = MNIWPrior(np.hstack([0.5 * np.eye(dx), np.zeros((dx, 1))]) + 0.1 * rng.standard_normal((dx, dx + 1)), 3.0 * np.eye(dx + 1), dx + 4.0, 0.5 * np.eye(dx))
    _compare_iterates(handle, [ys], start, 5, 1e-8, update=("F", "b", "Q"), prior=prior)
    # a partly observed row is accepted by the dynamics-only fit (as by `filtering`)
    part = ys.copy()
    part[7, 1] = np.nan
    fitted, ells, flags = fit_em(part, _lgssm(start, T), 3, update=("F", "b", "Q"), handle=handle)
    assert not flags.any() and np.all(np.isfinite(ells)) and all(np.all(np.isfinite(a)) for a in fitted)
    assert np.all(np.diff(ells) >= -1e-9 * np.abs(ells[:-1]))


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_failure_containment(handle, dtype):
    """T = 2 at dx = 4 with x_0 pinned by its prior (P0 = 1e-20 I): S_zz = sum of E[z_0 z_0^T] has rank 1 to working precision (tests/test_lgssm_em_host.py says
    why a diffuse x_0 would not do), the dynamics block is flagged 1 and keeps its bits, the observation and initial-state blocks update"""
    from aux_ssm_samplers_amd._primitives.kalman import fit_em
    dx, dy, S = 4, 2, 8
    rng = np.random.default_rng(17)
    p = E.random_model(rng, dx, dy)
    p["P0"] = 1e-20 * np.eye(dx)
    ys = np.stack([E.simulate(rng, p, 2)[1] for _ in range(S)])
    p = {k: v.astype(dtype) for k, v in p.items()}
    fitted, ells, flags = fit_em(ys.astype(dtype), _lgssm(p, 2), 1, handle=handle)
    got = _params(fitted)
    assert flags.tolist() == [[1, 0, 0, 0]]
    for name in ("F", "b", "Q"):
        assert got[name].dtype == dtype and np.array_equal(got[name], p[name]), name
    for name in ("H", "c", "R"):   # (m0 and P0 are re-estimated too, to the values they had: x_0 is pinned)
        assert not np.array_equal(got[name], p[name]), name
    assert all(np.all(np.isfinite(got[name])) for name in E.NAMES) and np.all(np.isfinite(ells))
    if dtype == np.float64:
        its, _, rflags = E.em(list(ys), {k: v.astype(np.float64) for k, v in p.items()}, 1)
        assert rflags.tolist() == [[1, 0, 0, 0]]
        for name in ("H", "c", "R", "m0"):
            assert np.max(np.abs(got[name] - its[1][name])) <= 1e-8, name


@pytest.mark.parametrize("parallel", [True, False], ids=["parallel", "sequential"])
def test_smoothing_lag_one(handle, parallel):
    from aux_ssm_samplers_amd._primitives.kalman import filter_smoothing, smoothing_lag_one
    dx, dy, T = 3, 3, 514
    p, ys, refs = _cell(dx, dy, T)
    lg = _lgssm(p, T)
    sms, sPs, cross, ell = smoothing_lag_one(ys[0], lg, parallel, handle=handle)
    sms0, sPs0, ell0 = filter_smoothing(ys[0], lg, parallel, handle=handle)
    assert np.array_equal(sms, sms0) and np.array_equal(sPs, sPs0) and np.array_equal(ell, ell0)
    X = refs[0][2][4]
    assert cross.shape == (T - 1, dx, dx)
    assert np.max(np.abs(cross - X)) <= FP64_BAR * np.max(np.abs(X))
    # equal rows instead of a broadcast view: still time-invariant
    lg2 = lg._replace(Fs=np.array(lg.Fs), Qs=np.array(lg.Qs), bs=np.array(lg.bs))
    assert np.array_equal(smoothing_lag_one(ys[0], lg2, parallel, handle=handle)[2], cross)


def test_c_entry_refusals(handle):
    from aux_ssm_samplers_amd import _lib
    from aux_ssm_samplers_amd._primitives.kalman.em import _Fit, NAMES
    dx, dy, T = 2, 3, 6
    p, ys, _ = _cell(dx, dy, T)
    fit = _Fit(handle, ys, p, np.float64, True, 1)
    fit.filter(0)
    fit.smooth()
    fit.statistics()
    lib, h = handle.lib, handle.h

    def refused(rc, text, status=_lib.ERR_ARG):
        assert rc == status, rc
        assert text in lib.auxssm_last_error().decode(), lib.auxssm_last_error().decode()

    def stats(dims=None, lg=None, ms=fit.ms.ptr, Ps=fit.Ps.ptr, sms=fit.sms.ptr, sPs=fit.sPs.ptr, cross=None, out=fit.stats.ptr, y=fit.yarr):
        return lib.auxssm_kalman_smooth_stats(h, _lib.F64, C.byref(dims or fit.dims), C.byref(lg or fit.lg), C.byref(y) if y is not None else None, ms, Ps, sms,
                                              sPs, cross, out)

    for kw in (dict(ms=None), dict(Ps=None), dict(sms=None), dict(sPs=None), dict(out=None), dict(y=None)):
        refused(stats(**kw), "must be non-NULL")
    refused(stats(dims=_lib.Dims(3, T, 1, 5, dy)), "dx <= 4", _lib.ERR_UNSUPPORTED)
    refused(stats(dims=_lib.Dims(3, T, 1, dx, 9)), "dy <= 8", _lib.ERR_UNSUPPORTED)
    refused(stats(dims=_lib.Dims(3, 1, 1, dx, dy)), "T >= 2")
    lg = _lib.Lgssm()
    C.memmove(C.byref(lg), C.byref(fit.lg), C.sizeof(lg))
    lg.Fs = fit.par["F"].arr(0, dx * dx, 0)
    refused(stats(lg=lg), "time strides of Fs, Qs and bs must be 0")
    refused(stats(out=fit.sPs.ptr), "may not alias")
    refused(stats(cross=fit.Ps.ptr), "may not alias")
    refused(stats(cross=fit.stats.ptr), "may not alias")
    refused(stats(dims=_lib.Dims(1 << 30, 1 << 20, 1, dx, dy)), "exceeds one launch")

    syy = (C.c_double * (dy * dy + 1))(*([0.0] * (dy * dy) + [1.0]))
    refs = [C.byref(fit.arr[name]) for name in NAMES]

    def mstep(dx_=dx, dy_=dy, nseq=3, stats_=fit.stats.ptr, syy_=syy, mask=7, refs_=refs, flags=fit.flags.ptr):
        return lib.auxssm_lgssm_em_mstep(h, _lib.F64, dx_, dy_, nseq, stats_, syy_, None, mask, *refs_, flags)

    refused(mstep(stats_=None), "must be non-NULL")
    refused(mstep(syy_=None), "must be non-NULL")
    refused(mstep(flags=None), "must be non-NULL")
    refused(mstep(dx_=5), "dx <= 4", _lib.ERR_UNSUPPORTED)
    refused(mstep(dy_=9), "dy <= 8", _lib.ERR_UNSUPPORTED)
    refused(mstep(nseq=0), "nseq >= 1")
    refused(mstep(mask=8), "update_mask")
    refused(mstep(refs_=[None] + refs[1:]), "must be non-NULL")
    bad = fit.par["H"].arr(0, dy * dx, 0)
    refused(mstep(refs_=refs[:3] + [C.byref(bad)] + refs[4:]), "time strides")
    assert mstep(mask=2, refs_=[None] * 3 + refs[3:6] + [None] * 2) == 0   # arrays of blocks outside the mask may be NULL
    handle.sync()
