"""The one kernel between the two streaming passes of the fused sweep (csrc/fused_shared.h: k_fs_mid, with the range-product tables of k_fs_gtab) at chunk
counts that take every branch of its two scans, through the public path DeviceChains(..., fused=...), against the keyed sweep with the bars of
tests/test_gpu_fused.py::test_fused_equals_keyed_sweep (x' 1e-9 / 1e-10, the four totals 1e-12 of their scale, log alpha 1e-7, flags equal; fp32 2e-3, 2e-6, 5e-2).

Chunk counts (a workgroup of 256 lanes scans a chain's nchunk aggregates, E2 = ceil(nchunk / 256) per lane; below 96 chains a chunk is 16 steps):
  T = 4080, 4096, 4100 -> nchunk 255, 256, 257: the last lane empty | every lane one chunk | E2 = 2 and the trailing lanes empty;   T = 8200 -> 513: E2 = 3, a ragged
  last lane;   T = 3001 at 96 and 130 chains (chunks of 32 steps, the unpacked passes) -> 94.
  T = 12, 32, 48 (nchunk 1, 2, 3) and the odd chain count 3 are in the list too, but the library refuses the fused sweep below T = 64 and for odd chain counts
  (csrc/api.hip::fused_refusal) before anything is enqueued: for these the test asserts the refusal (and a finite state after the keyed sweep that runs instead) --
  there is no fused sweep to hold to the bars.  The smallest chunk counts the kernel can be given are 4 and 5 (T = 64, 65: a last chunk of one step), which are here
  as well, and nchunk = 1, 2, 3 are covered by the host check (tests/test_fused_mid_host.py).
  (Two KEYED sweeps of T = 12, d = 1, 2 chains, fp64 with one key, the first of them the first sweep of the process, were seen to differ in the third digit in
  three of six runs, with the library of the commit before this kernel as well as with this one: a finding about the keyed sweep, not held against this kernel.)
The memoised tables: the model stage keeps its tables in a ring of three slabs, so a slab's tables are first REUSED by the fourth consecutive fused sweep; the memo
case runs five sweeps at one step size (the fourth and fifth reuse), then three at another (rebuilt: the step size is part of the memo's key), then one more (reused)."""
import numpy as np
import numpy.testing as npt
import pytest

from tests.test_gpu_fused import _setup

pytestmark = pytest.mark.gpu


def _fusable(T, Cn):
    return T >= 64 and Cn % 2 == 0


def _bars(dtype, a_x, b_x, la, lb, acc_a, acc_b, msg):
    tol = dict(rtol=1e-9, atol=1e-10) if dtype == np.float64 else dict(rtol=2e-3, atol=2e-3)
    npt.assert_array_equal(acc_a, acc_b, err_msg=msg)
    npt.assert_allclose(a_x, b_x, err_msg=msg, **tol)
    scale = np.abs(lb[:, 1:]).max()
    err_tot, err_la = np.abs(la[:, 1:] - lb[:, 1:]).max() / scale, np.abs(la[:, 0]).max()
    print(f"{msg}: totals {err_tot:.3g} of their scale, |log alpha| {err_la:.3g}, max |x' - keyed| {np.abs(a_x - b_x).max():.3g}")
    npt.assert_allclose(la[:, 1:], lb[:, 1:], rtol=0, atol=(1e-12 if dtype == np.float64 else 2e-6) * scale, err_msg=msg)
    assert err_la < (1e-7 if dtype == np.float64 else 5e-2), msg


_SHAPES = ([(T, d, Cn) for T in (12, 32, 48, 64, 65, 4080, 4096, 4100, 8200) for d in (1, 4) for Cn in (2, 3)]
           + [(4100, 4, 6), (3001, 4, 96), (3001, 4, 130)])


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("T,d,Cn", _SHAPES)
def test_fused_equals_keyed_sweep_at_every_branch_of_the_scans(dtype, T, d, Cn):
    from aux_ssm_samplers_amd import _lib, random as R
    from aux_ssm_samplers_amd.kalman.generic import DeviceChains, KalmanSampler
    h = _lib.default_handle()
    m, model, kernel, x0 = _setup(T, d, dtype, Cn)
    a = DeviceChains(h, x0, chain_minor=True)               # fused where the library takes it
    b = DeviceChains(h, x0, chain_minor=True, fused=False)  # the keyed sweep
    for i, delta in enumerate([0.5, 0.5, 0.2]):
        key = R.PRNGKey(40 + i)
        kernel(key, KalmanSampler(x=a, updated=None), delta)
        assert a.fused is _fusable(T, Cn)
        if not a.fused:     # refused before anything was enqueued: the keyed sweep ran, there is no fused sweep to compare
            assert np.isfinite(a.to_host()).all()
            return
        kernel(key, KalmanSampler(x=b, updated=None), delta)
        assert b.fused is False
        _bars(dtype, a.to_host(), b.to_host(), a.logs.to_host(), b.logs.to_host(), a.accepted.to_host(), b.accepted.to_host(), f"T={T} d={d} C={Cn} sweep {i}")
    assert a.accepted.to_host().all()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_reused_and_rebuilt_tables_give_the_keyed_sweeps(dtype):
    from aux_ssm_samplers_amd import _lib, random as R
    from aux_ssm_samplers_amd.kalman.generic import DeviceChains, KalmanSampler
    h = _lib.default_handle()
    T, d, Cn = 4100, 4, 2                                   # nchunk 257: E2 = 2
    m, model, kernel, x0 = _setup(T, d, dtype, Cn)
    deltas = [0.5] * 5 + [0.2] * 4
    a = DeviceChains(h, x0, chain_minor=True)
    got = []
    for i, delta in enumerate(deltas):                      # consecutive fused sweeps: nothing else opens a model stage in between
        kernel(R.PRNGKey(70 + i), KalmanSampler(x=a, updated=None), delta)
        assert a.fused is True
        got.append((a.to_host(), a.logs.to_host(), a.accepted.to_host()))
    b = DeviceChains(h, x0, chain_minor=True, fused=False)
    for i, delta in enumerate(deltas):
        kernel(R.PRNGKey(70 + i), KalmanSampler(x=b, updated=None), delta)
        assert b.fused is False
        _bars(dtype, got[i][0], b.to_host(), got[i][1], b.logs.to_host(), got[i][2], b.accepted.to_host(), f"sweep {i} delta {delta}")
        assert got[i][2].all()


def test_time_varying_model_with_missing_rows_against_its_oracle():
    """tests/fused_cases.py, A-d4p4-T70-C6 (five chunks, rows missing at t = 0, across the first chunk boundary and at T - 1), reference policy: the shared
    fused run of tests/test_gpu_fused_models.py against the oracle and the keyed sweep"""
    from tests import fused_cases as FC
    from tests import test_gpu_fused_models as FM
    case = next(c for c in FC.GROUP_A if (c.d, c.po) == (4, 4))
    assert (case.T + case.E - 1) // case.E >= 3
    run = FM.fused_run(case, "float64", "reference")
    FM._check_bookkeeping(case, run)
    FM._check_against_oracle(case, "float64", "reference", run, case.checked)
    FM._check_against_unfused(case, "float64", "reference", run, np.arange(case.C), case.checked)
