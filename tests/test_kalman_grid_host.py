"""The narrow Kalman filter's full (dx, dy) grid on the CPU: the product's per-lane bodies (csrc/kalman_math.h, csrc/kalman_bodies.h) compiled for the host
(tests/hostsim) against the NumPy oracle on the cases of tests/kalman_grid_cases.py -- every (R, D, P) the device library instantiates, E = 0 (sequential form),
E = 4 (chunked form) and E = -4 (chain-minor buffers), with the placed missing rows on both sides of the first chunk edge.  Also where the conditions on the cases
themselves are asserted.  fp64 at TOL64 (rtol 1e-7, atol 1e-9); fp32 at most 4 times the fp32 oracle's own error (kalman_grid_cases.fp32_reference_error).

Measured (the tests print every figure, -s):
  fp32 oracle error, worst of the 32 pairs and both orders
      T = 70    means 1.23e-06  covariances 1.04e-06  ell 3.05e-07
      T = 600   means 2.11e-06  covariances 1.58e-06  ell 9.03e-07
      joint log-density at T = 70   1.43e-07
  host build (g++ -O1 -ffp-contract=off) fp32 error / the oracle's, worst over the pairs (bar: 4)
      T = 70    E = 0    means 1.13  covariances 1.15  ell 2.17        E = 4 and -4   means 1.13  covariances 1.15  ell 1.00
      T = 600   E = 0    means 0.54  covariances 0.88  ell 1.94        E = 4 and -4   means 0.54  covariances 0.88  ell 0.80
      joint log-density  2.41
  host build fp64: worst max|host - oracle| / max|oracle| 6.5e-15
"""
import numpy as np
import numpy.testing as npt
import pytest

from oracle import kalman_np as K
from tests import hostsim as HS
from tests import kalman_grid_cases as G

CASES = [(dx, dy, 70) for dx, dy in G.PAIRS] + [(dx, dy, 600) for dx, dy in G.PAIRS if dy in (1, 8)]


def test_grid_is_complete():
    assert len(G.PAIRS) == 32 and len(set(G.PAIRS)) == 32
    assert len(CASES) == 40


@pytest.mark.parametrize("T", [70, 600])
@pytest.mark.parametrize("dx,dy", G.PAIRS)
def test_case_conditions(dx, dy, T):
    cs = G.case(dx, dy, T)
    assert cs.observed_fraction() >= 0.8
    ms, Ps, ell = G.reference(cs)
    assert np.all(np.isfinite(ms)) and np.all(np.isfinite(Ps)) and np.isfinite(ell)
    assert abs(ell) >= 10
    _check_placement(cs.ys, cs.where, T, dy)


def _check_placement(ys, where, T, dy):
    nan = ~np.isfinite(ys)
    left, right = G.edge_steps(T)
    for t in (left, right, T - 1):
        assert nan[t].any(), t
    kinds = set(where.values())
    assert "A" in kinds and nan.all(axis=1).any()
    if dy > 1:
        assert any(nan[t, 0] and nan[t].sum() == 1 for t in where)                 # only component 0 missing
        assert any(nan[t, dy - 1] and nan[t].sum() == 1 for t in where)            # only component dy - 1 missing
    if dy >= 3:
        assert any(nan[t].sum() == dy - 1 for t in where)                          # exactly one component present
    assert nan[0].any() == bool(dy % 2)
    assert not nan[[t for t in range(T) if t not in where]].any()


@pytest.mark.parametrize("dx,dy", G.PAIRS)
def test_lanes_case_conditions(dx, dy):
    cs = G.lanes_case(dx, dy)
    T, B, Cn = G.LANES["T"], G.LANES["B"], G.LANES["C"]
    assert cs.ys.shape == (Cn, T, B, dy)
    assert cs.observed_fraction() >= 0.8
    for c in (0, Cn - 1):
        for b in (0, 31, B - 1):
            assert np.mean(np.all(np.isfinite(cs.ys[c, :, b]), axis=-1)) >= 0.8
            _check_placement(cs.ys[c, :, b], cs.where[c, b], T, dy)
    assert len({tuple(sorted(w.items())) for w in cs.where.values()}) > 1 or dy == 1     # the chains and lanes do not share one pattern
    for ms, Ps, ell in G.lanes_reference(cs):
        assert np.all(np.isfinite(ms)) and np.all(np.isfinite(Ps)) and np.isfinite(ell) and abs(ell) >= 10


@pytest.mark.parametrize("E", [0, 4, -4])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("dx,dy,T", CASES)
def test_filter_grid(dx, dy, T, dtype, E):
    cs = G.case(dx, dy, T)
    ys, lg = cs.as_dtype(dtype)
    got = HS.filtering(ys, lg, E, dtype=dtype)
    want = G.reference(cs)
    assert got[0].dtype == dtype
    if dtype == np.float64:
        for g, w in zip(got, want):
            npt.assert_allclose(g, w, **G.TOL64)
    else:
        G.check_fp32(got, want, T, "host", f"dx={dx} dy={dy} T={T} E={E}")


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("dx,dy", G.PAIRS)
def test_joint_logpdf_grid(dx, dy, dtype):
    """log_likelihood + prior_logpdf in one pass (kalman_bodies.h::body_logpdf) at states near the filtered means; a row with a missing component drops its whole
    observation term (the reference's nansum)"""
    cs = G.case(dx, dy, 70)
    xs, (_, prior, ll) = G.logpdf_case(dx, dy)
    ys, lg = cs.as_dtype(dtype)
    got = HS.joint_logpdf(ys, xs.astype(dtype), lg, dtype=dtype)
    if dtype == np.float64:
        npt.assert_allclose(got, prior + ll, **G.TOL64)
    else:
        err, bar = G.rel_err(got, prior + ll), G.fp32_logpdf_error()[3]
        print(f"host joint logpdf dx={dx} dy={dy}: fp32 error / oracle's {err / bar:.2f}")
        assert err <= G.FP32_FACTOR * bar, (err, bar)
