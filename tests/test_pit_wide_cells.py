"""The wide-state cells of the parallel-in-time cSMC sweep (tests/pit_wide_cases.py: 4 < d <= 32, N <= 64) on the CPU: the inputs that
tests/test_gpu_pit_wide.py holds the HIP kernels of csrc/pit_wide.hip to.  For every cell, on the literal tree alone (oracle/pit_np.py), the smallest draw
margin is >= 2 N^2 eps (tests/test_oracle_pit_literal.py, "Ties"), so an index mismatch is a defect and never a tie; then the contract oracle
(oracle/csmc_ref.c::csmc_ref_pit_sweep, generic in d up to 32) in fp64 equals the literal: origins identical, trajectory within 1e-12.  A cell with N >= 25 that
left every time step on the reference trajectory would compare nothing but the leaves: each moves at least one."""
import numpy as np
import numpy.testing as npt
import pytest

from tests import pit_cases as PC
from tests import pit_wide_cases as W


def test_cells_cover_the_sizes_and_every_potential_with_gradient_and_time_varying_off_and_on():
    cells = W.WIDE_CELLS
    assert all(4 < c[0] <= 32 and 2 <= c[1] <= 64 and c[2] >= 2 for c in cells)
    assert {5, 8, 17, 30, 32} <= {c[0] for c in cells}
    assert {2, 25, 32, 33, 64} <= {c[1] for c in cells}
    assert {2, 3, 5, 9, 33} <= {c[2] for c in cells}
    for pot in (W.FLAT, W.GAUSS, W.SV, W.MASKED):
        assert {c[4] for c in cells if c[3] == pot} == {0, 1}, pot
        assert {c[5] for c in cells if c[3] == pot} == {0, 1}, pot
    for named in ((5, 25, 9, W.SV, 0, 0, 0), (8, 33, 5, W.MASKED, 1, 0, 0), (30, 25, 33, W.SV, 0, 0, 0), (32, 64, 8, W.GAUSS, 1, 1, 0),
                  (30, 25, 9, W.SV, 1, 0, 0), (16, 2, 37, W.FLAT, 0, 1, 0)):
        assert named in cells


@pytest.mark.parametrize("cell", W.WIDE_CELLS, ids=PC.cell_id)
def test_contract_oracle_fp64_equals_the_literal_tree_on_a_wide_cell(cell):
    c = PC.case(cell)
    xl, origins, hist = PC.literal(cell)
    threshold = PC.margin_threshold(c.N)
    print(f"{PC.cell_id(cell)}: smallest draw margin {hist['min_margin']:.2e} (threshold {threshold:.2e}), {int((origins != 0).sum())} of {c.T} steps updated")
    assert hist["min_margin"] >= threshold
    ref = c.oracle_sweep(np.float64)
    npt.assert_array_equal(ref["ancestors"], origins)
    npt.assert_allclose(ref["x"], xl, rtol=1e-12, atol=1e-12)
    if c.N >= 25:
        assert (origins != 0).any()


@pytest.mark.parametrize("cell", W.COUPLED_CELLS, ids=W.coupled_cell_id)
def test_coupled_cells_meet_the_margin_condition_and_move(cell):
    c = W.coupled_case(cell)
    _, origins, hist = W.coupled_literal(cell)
    assert hist["min_margin"] >= PC.margin_threshold(c.N)
    assert (origins != 0).any()
    assert np.isnan(c.m.y[c.flat_rows]).all() and np.isfinite(np.delete(c.m.y, c.flat_rows, axis=0)).all()
