"""All 64 narrow Kalman filter entries (dx 1..4 x dy 1..8, fp32 and fp64) on every launch form of `auxssm_kalman_filter` (csrc/kernels.hip.h::run_filter), on the
cases of tests/kalman_grid_cases.py: contracting time-varying models with placed missing rows (wholly missing, component 0, component dy-1, one component present)
at the last step and on both sides of the first chunk / tile edge.

  seq     T = 70, one sequence, parallel=False   k_filter_t0, k_filter_init<R,D,P>, one-chunk scan; fp32 ell by k_ell_pass<R,D,P>
  chunk   T = 70, one sequence, parallel=True    chunks of 4 elements; fp64 also against seq at rtol 1e-9 / atol 1e-10
  tile    T = 600, one sequence, parallel=True   FilterOpBuild<R,D,P,0> inside k_ks_tile: three tiles, the last one partial
  lanes   T = 33, B = 64, C = 4, both orders     FilterOpBuildCm<R,D,P,0> / FilterOpSeqWalk<R,D,P> through the C ABI, ell by per-chunk sums
plus the joint log-density (run_logpdf<R,D,P>) and the sampler (dx 1..4, T = 70 and 600).

Bars: fp64 TOL64 = rtol 1e-7, atol 1e-9 against the fp64 sequential oracle.  fp32: per case max|device - fp64| / max|fp64| at most 4 times the fp32 NumPy oracle's
own error on the same group of cases (kalman_grid_cases.fp32_reference_error), separately for means, covariances and ell; the log-densities and the sampler
likewise against the oracle's functions run in fp32.

fp32 oracle errors, worst of the 32 pairs and both orders (printed by the tests, -s):
  one sequence T = 70 (seq, chunk)   means 1.23e-06  covariances 1.04e-06  ell 3.05e-07
  one sequence T = 600 (tile)        means 2.11e-06  covariances 1.58e-06  ell 9.03e-07
  lanes T = 33                       means 3.26e-06  covariances 6.87e-07  ell 1.37e-07
  log-densities at T = 70            posterior 4.48e-05  prior 1.53e-07  log-likelihood 1.53e-07
  sampler, worst of dx 1..4          T = 70  1.66e-07    T = 600  1.47e-07
Measured on an MI355X, fp32 error / the oracle's, worst over the pairs (bar: 4):
  seq     means 0.87  covariances 0.56  ell 0.19
  chunk   means 0.87  covariances 0.56  ell 0.19
  tile    means 0.81  covariances 0.47  ell 0.08
  lanes   means 0.57  covariances 0.68  ell 0.59 (parallel=False)  0.46 (parallel=True)
  log-densities   posterior 1.06  prior 0.87  log-likelihood 1.48
  sampler         T = 70  1.84    T = 600  1.50   (both orders alike)
fp64, worst max|device - oracle| / max|oracle| over all forms: means 5.7e-15, covariances 3.2e-15, ell 1.3e-15.  No bar was exceeded.
"""
import ctypes as C

import numpy as np
import numpy.testing as npt
import pytest

from tests import kalman_grid_cases as G

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
GRID = pytest.mark.parametrize("dx,dy", G.PAIRS)


@pytest.fixture(scope="module")
def P():
    import aux_ssm_samplers_amd._primitives.kalman as prim
    return prim


def test_grid_is_complete():
    assert len(G.PAIRS) == 32 and len(set(G.PAIRS)) == 32


def _check(got, want, dtype, T, form, what):
    assert got[0].dtype == dtype and got[1].dtype == dtype
    if dtype == np.float64:
        errs = G.filter_errors(got, want)
        print(f"{form} {what}: fp64 errors  means {errs[0]:.1e}  covariances {errs[1]:.1e}  ell {errs[2]:.1e}")
        for g, w in zip(got, want):
            npt.assert_allclose(g, w, **G.TOL64)
    else:
        G.check_fp32(got, want, T, form, what)


def _run(P, dx, dy, T, dtype, parallel):
    cs = G.case(dx, dy, T)
    ys, lg = cs.as_dtype(dtype)
    return cs, P.filtering(ys, P.LGSSM(*lg), parallel)


def _lanes_filter(cs, dx, dy, dtype, parallel):
    """auxssm_kalman_filter on a lanes case: one model per b shared by the chains (chain stride 0), ys (C, T, B, dy)"""
    from aux_ssm_samplers_amd import _lib
    from aux_ssm_samplers_amd._primitives.kalman.base import DeviceLGSSM
    Cn, T, B, _ = cs.ys.shape
    h = _lib.default_handle()
    dl = DeviceLGSSM(h, cs.lg, 1, T, B, dx, dy, True, dtype)
    yd = h.to_device(cs.ys.astype(dtype))
    msd, Psd, elld = h.empty((Cn, T, B, dx), dtype), h.empty((Cn, T, B, dx, dx), dtype), h.empty((Cn,), dtype)
    dims = _lib.Dims(Cn, T, B, dx, dy)
    yarr = yd.arr(T * B * dy, B * dy, dy)
    _lib.check(h.lib.auxssm_kalman_filter(h.h, _lib.dtype_code(dtype), C.byref(dims), C.byref(dl.c), C.byref(yarr), int(parallel), msd.ptr, Psd.ptr, elld.ptr))
    return msd.to_host(), Psd.to_host(), elld.to_host()


@pytest.mark.parametrize("dx,dy", [(1, 1), (4, 8)])
@DTYPES
def test_forms_take_their_launch_paths(P, dx, dy, dtype):
    """The shapes above reach the forms they are named after (the thresholds live in run_filter / use_ks / auxssm_kalman_filter): seq and chunk build an element
    buffer (one k_filter_init stage), tile and lanes build their elements inside the scan (none).  (4, 8) in fp64 is the heaviest operator of the tile threshold."""
    from aux_ssm_samplers_amd import _lib
    h = _lib.default_handle()

    def groups(run):
        h.prof_enable(_lib.K_ALL, 64)
        try:
            run()
            return {k: n for k, (n, _) in h.prof_read_groups().items()}
        finally:
            h.prof_disable()

    for T, parallel, init in ((70, False, 1), (70, True, 1), (600, True, 0)):
        g = groups(lambda: _run(P, dx, dy, T, dtype, parallel))
        assert g.get("filter_init", 0) == init and g.get("filter_scan", 0) == 1, (T, parallel, g)
    for parallel in (False, True):
        g = groups(lambda: _lanes_filter(G.lanes_case(dx, dy), dx, dy, dtype, parallel))
        assert g.get("filter_init", 0) == 0 and g.get("filter_scan", 0) == 1, (parallel, g)


@GRID
@DTYPES
def test_seq(P, dx, dy, dtype):
    cs, got = _run(P, dx, dy, 70, dtype, False)
    _check(got, G.reference(cs), dtype, 70, "seq", f"dx={dx} dy={dy}")


@GRID
@DTYPES
def test_chunk(P, dx, dy, dtype):
    cs, got = _run(P, dx, dy, 70, dtype, True)
    _check(got, G.reference(cs), dtype, 70, "chunk", f"dx={dx} dy={dy}")
    if dtype == np.float64:
        _, seq = _run(P, dx, dy, 70, dtype, False)
        for g, s in zip(got, seq):
            npt.assert_allclose(g, s, rtol=1e-9, atol=1e-10)


@GRID
@DTYPES
def test_tile(P, dx, dy, dtype):
    cs, got = _run(P, dx, dy, 600, dtype, True)
    _check(got, G.reference(cs), dtype, 600, "tile", f"dx={dx} dy={dy}")


@pytest.mark.parametrize("parallel", [False, True], ids=["walk", "scan"])
@GRID
@DTYPES
def test_lanes(dx, dy, dtype, parallel):
    """One model per b, shared by the chains (chain stride 0); each (c, b) sequence its own observations and missing rows; against the oracle's batched filter per
    chain (fp32 yardstick: that filter in fp32)."""
    cs = G.lanes_case(dx, dy)
    ms, Ps, ell = _lanes_filter(cs, dx, dy, dtype, parallel)
    want = G.lanes_reference(cs)
    for c in range(cs.ys.shape[0]):
        _check((ms[c], Ps[c], ell[c]), want[c], dtype, cs.T, "lanes", f"dx={dx} dy={dy} parallel={int(parallel)} c={c}")


@GRID
@DTYPES
def test_joint_logpdf(P, dx, dy, dtype):
    """posterior_logpdf, prior_logpdf, log_likelihood at states near the filtered means"""
    cs = G.case(dx, dy, 70)
    xs, want = G.logpdf_case(dx, dy)
    ys, lg = cs.as_dtype(dtype)
    lg, xs, ell = P.LGSSM(*lg), xs.astype(dtype), dtype(G.reference(cs)[2])
    got = (P.posterior_logpdf(ys, xs, ell, lg), P.prior_logpdf(xs, lg), P.log_likelihood(ys, xs, lg))
    if dtype == np.float64:
        for g, w in zip(got, want):
            npt.assert_allclose(g, w, **G.TOL64)
        return
    bar = G.fp32_logpdf_error()
    errs = [G.rel_err(g, w) for g, w in zip(got, want)]
    print(f"logpdf dx={dx} dy={dy}: fp32 error / oracle's  posterior {errs[0] / bar[0]:.2f}  prior {errs[1] / bar[1]:.2f}  log-likelihood {errs[2] / bar[2]:.2f}")
    for name, e, b in zip(("posterior_logpdf", "prior_logpdf", "log_likelihood"), errs, bar):
        assert e <= G.FP32_FACTOR * b, f"{name}: error {e:.3e} is {e / b:.1f} times the fp32 oracle's {b:.3e}"


@pytest.mark.parametrize("parallel", [False, True])
@pytest.mark.parametrize("T", [70, 600])
@pytest.mark.parametrize("dx", [1, 2, 3, 4])
@DTYPES
def test_sampler(P, dx, T, parallel, dtype):
    """The pathwise sampler on the oracle's filtered moments (T = 600 in parallel: the tile scan)"""
    cs, ms, Ps, eps, want = G.sampler_case(dx, T)
    _, lg = cs.as_dtype(dtype)
    xs = P.sampling(None, ms.astype(dtype), Ps.astype(dtype), P.LGSSM(*lg), parallel, eps=eps.astype(dtype))
    assert xs.dtype == dtype
    if dtype == np.float64:
        npt.assert_allclose(xs, want[parallel], **G.TOL64)
        return
    err, bar = G.rel_err(xs, want[False]), G.fp32_sampler_error(T)
    print(f"sampler dx={dx} T={T} parallel={int(parallel)}: fp32 error / oracle's {err / bar:.2f}")
    assert err <= G.FP32_FACTOR * bar, f"error {err:.3e} is {err / bar:.1f} times the fp32 oracle's {bar:.3e}"
