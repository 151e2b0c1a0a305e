"""The fused chain-shared sweep after u left memory (csrc/fused_shared.h): pass AC keeps u in registers and forms no MH terms; pass E reads x through the
selector, rebuilds u_{t+1} from the keyed draw (normals_cm inside pass E: the lane-pair exchange for d >= 2, the odd-D tail for d = 1, 3) and forms the terms
of both states, the pair (t + 1, t) summed into the chunk of t.

Shapes: d = po in {1, 2, 3, 4}; C in {2, 6, 66} (packed form; 66 chains = more than one wave of chains) and 130 (plain form, partly filled last tile);
T in {64, 70, 3 E + 5} with E the driver's chunk length (16 below 96 chains, 32 from there): chunks that fit exactly, a ragged last chunk, several chunks with a
ragged last one -- the x load at a chunk's top, the pair across every chunk boundary and the last chunk (no pair above T - 1) are all walked.  3 E + 5 is run
where the library takes it: at E = 16 it is 53, below the fused sweep's floor of T >= 64 (csrc/api.hip::fused_refusal), and T = 70 = 4 E + 6 is the packed form's
several chunks with a ragged last one; at E = 32 it is 101.  Every case is a
time-varying model with missing rows and components (tests/fused_cases.py).  po != d, the NaN in the state and both NaN policies: B-d3p2-T70-C130 of
fused_cases.

Harness and bars are those of tests/test_gpu_fused_models.py: three consecutive keyed sweeps on a lazy state that is never resolved (from the second sweep on
pass E reads x from both buffers); against the oracle and against the keyed sweep (fused=False): states 1e-9 / 1e-10, the four totals 1e-12 of their scale,
log alpha 1e-7, fp64 flags identical, a rejected chain's state bit for bit; fp32: states 2e-3, log alpha within fused_cases.FP32_MARGIN.

Seeds: per case the smallest for which, on the CPU oracle, the checked chains of the first sweep hold an acceptance and a rejection and every checked margin
|log alpha - log u| of the three sweeps is at least fused_cases.MIN_MARGIN (test_seeds_give_both_flags_on_the_oracle, no GPU)."""
import numpy as np
import pytest

from tests import fused_cases as FC
from tests import test_gpu_fused_models as M

gpu = pytest.mark.gpu

#         index  d  po   T    C  seed
_SPEC = [(100, 1, 1, 64, 2, 0), (101, 2, 2, 70, 2, 2), (102, 3, 3, 70, 6, 0), (103, 4, 4, 64, 6, 0),
         (104, 1, 1, 70, 66, 0), (105, 2, 2, 64, 66, 0), (106, 3, 3, 70, 66, 0),
         (107, 4, 4, 101, 130, 0), (108, 3, 3, 64, 130, 0), (109, 2, 2, 70, 130, 0)]
CASES = [FC.Case(i, "F", d, po, T, C, seed) for i, d, po, T, C, seed in _SPEC]
IDS = [c.id for c in CASES]
MIXED = FC.GROUP_B[4]    # B-d3p2-T70-C130: po != d, NaN chain 100


def test_the_shapes_are_the_ones_meant():
    assert MIXED.id == "B-d3p2-T70-C130" and MIXED.nan_chain == 100
    assert {c.d for c in CASES} == {1, 2, 3, 4} and {c.C for c in CASES} == {2, 6, 66, 130}
    for c in CASES:
        assert c.T in (64, 70, 3 * c.E + 5) and c.E == (32 if c.C == 130 else 16)
    assert {c.T for c in CASES if c.C == 130} == {64, 70, 101}
    for C in (2, 6, 66):
        assert {c.T for c in CASES if c.C == C} == {64, 70}


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_seeds_give_both_flags_on_the_oracle(case):
    runs = [FC.oracle_chain(case, "reference", c) for c in case.checked]
    acc = [r[0]["accepted"] for r in runs]
    assert 0 < sum(acc) < len(acc)
    assert min(q["margin"] for r in runs for q in r) >= FC.MIN_MARGIN


@gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_two_states_in_pass_e_equal_the_oracle_and_the_keyed_sweep(case):
    res = M.fused_run(case, "float64", "reference")
    M._check_bookkeeping(case, res)
    M._check_against_oracle(case, "float64", "reference", res, case.checked)
    M._check_against_unfused(case, "float64", "reference", res, np.arange(case.C), case.checked)
    first = res[0]["accepted"][case.checked]
    assert 0 < first.sum() < len(first)                           # both flags, as the oracle said
    assert set(np.unique(res[1]["sel_old"])) == {0, 1}             # the second sweep's pass E reads x from both buffers
    for rec in res:
        assert np.abs(rec["logs"][:, 0] - rec["unf_logs"][:, 0]).max() < 1e-7


@gpu
@pytest.mark.parametrize("policy", ["reference", "masked"])
def test_po_other_than_d_with_missing_rows_under_both_policies(policy):
    res = M.fused_run(MIXED, "float64", policy)
    M._check_bookkeeping(MIXED, res)
    M._check_against_oracle(MIXED, "float64", policy, res, MIXED.checked)
    M._check_against_unfused(MIXED, "float64", policy, res, np.arange(MIXED.C), MIXED.checked)
    if policy == "masked":
        for rec in res:
            assert np.abs(rec["logs"][:, 0]).max() < 1e-7 and rec["accepted"].all()
    else:
        assert set(np.unique(res[1]["sel_old"])) == {0, 1}


@gpu
@pytest.mark.parametrize("policy", ["reference", "masked"])
def test_a_nan_in_the_state_takes_the_slow_path_for_both_states(policy):
    """the NaN chain's wave redoes x's and x''s terms under the per-term policy in pass E, and pass AC masks the chain's u for the fold as before: every other chain
    of the wave keeps the bars, the NaN chain is rejected with its state untouched"""
    case, nc = MIXED, MIXED.nan_chain
    res = M.fused_run(case, "float64", policy, "mid")
    others = [c for c in case.nan_wave if c != nc]
    M._check_bookkeeping(case, res)
    M._check_against_oracle(case, "float64", policy, res, others)
    M._check_against_unfused(case, "float64", policy, res, [c for c in range(case.C) if c != nc], others)
    for i, rec in enumerate(res):
        assert np.isnan(rec["logs"][nc, 0]) and rec["accepted"][nc] == 0 and rec["sel_new"][nc] == 0, i
        assert M._same_bits(rec["new"][nc], res[0]["prev"][nc]) and np.isnan(rec["new"][nc]).sum() == 1, i
        fa, un = rec["logs"][nc], rec["unf_logs"][nc]
        scale = np.abs(rec["unf_logs"][others][:, 1:]).max()
        np.testing.assert_allclose([fa[3], fa[4], fa[2] - fa[1]], [un[3], un[4], un[2] - un[1]], rtol=0, atol=1e-12 * scale, equal_nan=True)
        assert np.isfinite(fa[3:]).all()


@gpu
def test_fp32_takes_the_table_free_draws_and_its_own_lds_sizes():
    case = CASES[7]   # d = 4, T = 3 E + 5, 130 chains
    res = M.fused_run(case, "float32", "reference")
    M._check_bookkeeping(case, res)
    M._check_against_oracle(case, "float32", "reference", res, case.checked)
    M._check_against_unfused(case, "float32", "reference", res, np.arange(case.C), case.checked)
