"""The cases of tests/fused_cases.py on the CPU: the conditions the oracle alone must meet before tests/test_gpu_fused_models.py holds the fused sweep
(csrc/fused_shared.h) to it.  On the host restatement of the device's draws (`device_noise`), over the three consecutive oracle sweeps of every checked chain:
the reference policy accepts and rejects (so the ping-pong selector of the second sweep is mixed), no accept flag hinges on rounding, the masked oracle gives
log alpha = 0 (the model is exact: the independent check of `masked_log_likelihood`), and without missing data it is the reference oracle."""
import numpy as np
import numpy.testing as npt
import pytest

from tests import fused_cases as FC

ids = [c.id for c in FC.CASES]


def test_the_cases_are_the_shapes_that_reach_every_launch_form():
    assert [(c.d, c.po) for c in FC.GROUP_A] == FC.PAIRS and all((c.T, c.C, c.E) == (70, 6, 16) for c in FC.GROUP_A)
    assert [(c.d, c.po, c.T, c.C, c.E) for c in FC.GROUP_B] == [(3, 2, 64, 4, 16), (4, 1, 97, 30, 16), (2, 4, 130, 64, 16), (3, 3, 97, 128, 32), (3, 2, 70, 130, 32),
                                                                (1, 3, 70, 258, 32), (4, 4, 130, 1024, 64)]
    assert [(c.d, c.po, c.T, c.C, c.tinv) for c in FC.GROUP_C] == [(2, 3, 70, 6, True), (4, 4, 70, 130, True)]
    assert [c.C for c in FC.NAN_CASES] == [30, 130, 258]
    # 16 pairs x 2 dtypes + 7 x 3 + 2 x 2 oracle comparisons; every pair in both dtypes
    assert len(FC.RUNS) == 57
    for dt in ("float64", "float32"):
        assert {(c.d, c.po) for c, d_, _ in FC.RUNS if d_ == dt} >= set(FC.PAIRS)
    for c in FC.CASES:
        ch = c.checked
        assert ch == sorted(set(ch)) and (ch == list(range(c.C)) if c.C <= 30 else 12 <= len(ch) <= 16 and {0, c.C - 1} <= set(ch))
        assert all(b - 1 in ch and b in ch for b in (64, 192, 256) if b < c.C)
        if c.nan_chain is not None:
            assert c.nan_chain in c.nan_wave and (c.C <= 30 or ({c.nan_chain - 1, c.nan_chain + 1} <= set(ch) and c.nan_chain not in ch))
            E = c.E
            assert c.nan_row("mid") % E == E // 2 and c.nan_row("first") % E == 0 and 0 < c.nan_row("mid") < c.T and 0 < c.nan_row("first") < c.T


@pytest.mark.parametrize("case", FC.CASES, ids=ids)
def test_every_forced_edge_row_is_missing_and_the_rest_is_a_mix(case):
    y, full = case.y, case.m["y"]
    nan = np.isnan(y)
    assert set(case.forced_rows) == {0, case.E - 1, case.E, case.T - 1} and len(case.forced_rows) == 4
    for t, kind in case.forced_rows.items():
        assert nan[t].all() if kind == "whole" else (nan[t].sum() == 1 and case.po > 1), (t, kind)
    kinds = [case.forced_rows[0], case.forced_rows[case.T - 1]]
    assert case.po == 1 or sorted(kinds) == ["partial", "whole"]
    npt.assert_array_equal(y[~nan], full[~nan])
    assert (~nan).all(axis=1).sum() >= case.T // 2      # most rows are observed
    assert case.tinv == (case.m["Hs"].strides[0] == 0 and case.m["Fs"].strides[0] == 0)


def test_t0_alternates_between_a_whole_and_a_partial_row():
    multi = [c.forced_rows[0] for c in FC.CASES if c.po > 1]
    assert multi.count("whole") >= 4 and multi.count("partial") >= 4


@pytest.mark.parametrize("case", FC.CASES, ids=ids)
def test_reference_policy_accepts_and_rejects_with_margins(case):
    ch = case.checked
    runs = [FC.oracle_chain(case, "reference", c) for c in ch]
    acc = np.array([[r["accepted"] for r in rr] for rr in runs])
    la = np.array([[r["log_alpha"] for r in rr] for rr in runs])
    mg = np.array([[r["margin"] for r in rr] for rr in runs])
    print(f"{case.id}: accepted {acc.sum(0)} of {len(ch)}, log alpha in [{la.min():.2f}, {la.max():.2f}], smallest margin {mg.min():.3g}, "
          f"margins above {FC.FP32_MARGIN}: {(mg > FC.FP32_MARGIN).sum(0)}")
    assert np.isfinite(la).all()
    assert acc[:, 0].sum() >= 2 and (~acc[:, 0]).sum() >= 2       # the selector is mixed going into the second sweep
    assert mg.min() >= FC.MIN_MARGIN
    assert ((mg > FC.FP32_MARGIN).sum(0) * 8 >= 7 * len(ch)).all()  # fp32 flags: at least 7 of 8 checked chains stay in the comparison


@pytest.mark.parametrize("case", FC.CASES, ids=ids)
def test_masked_oracle_has_log_alpha_zero_and_equals_the_reference_oracle_without_missing_data(case):
    ea, es, ua = FC.device_noise(case, 0)
    for c in case.checked:
        r = FC.oracle_chain(case, "masked", c, 1)[0]
        assert abs(r["log_alpha"]) < 1e-9 and r["accepted"], (c, r["log_alpha"])
    c = case.checked[-1]
    full = case.m["y"]
    a = case.oracle_sweep("masked", case.x0[c], FC.DELTAS[0], ea[c], es[c], ua[c], y=full)
    b = case.oracle_sweep("reference", case.x0[c], FC.DELTAS[0], ea[c], es[c], ua[c], y=full)
    npt.assert_allclose(a["x_prop"], b["x_prop"], rtol=0, atol=0)
    for k in ("lp_prop", "lp_rev", "lt_prop", "lt_rev"):
        npt.assert_allclose(a[k], b[k], rtol=1e-12, atol=0)
    assert abs(a["log_alpha"] - b["log_alpha"]) < 1e-12 * max(abs(b["lt_prop"]), abs(b["lp_prop"])) and abs(b["log_alpha"]) < 1e-9


def test_device_noise_is_the_flat_index_of_the_chain_minor_layout():
    """the restatement draws n = T d C values per key and reads them as (T, d, C): chain c, step t, component k is flat index (t d + k) C + c"""
    from oracle import rng_np as RN
    from aux_ssm_samplers_amd import random as R
    case = FC.GROUP_A[6]
    ea, es, ua = FC.device_noise(case, 1)
    k_aux, k_samp, k_acc = R.split(case.key(1), 3)
    flat = RN.normal(k_samp, 0, case.T * case.d * case.C, np.float64)
    t, k, c = 11, case.d - 1, 4
    assert es[c, t, k] == flat[(t * case.d + k) * case.C + c] and ea.shape == es.shape == (case.C, case.T, case.d)
    npt.assert_array_equal(ua, RN.uniform(k_acc, 0, case.C, np.float64))
