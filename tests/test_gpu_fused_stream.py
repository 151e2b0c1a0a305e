"""Pass E of the fused chain-shared sweep (csrc/fused_shared.h, k_fs_e) at the shapes where the mapping of its work to lanes and its memory instructions can go
wrong: last chunks of 1 ... 5 steps for the chunk length the plan picks at that chain count, chain counts with partial waves and more than one chain group
(130, 258: the unpacked form, which walks the chunks from the last one down with non-temporal record loads and x' stores; 64, 66: the packed one), d in {1, 2, 4}, both dtypes; a lazy state whose selector
differs / agrees inside the pairs of adjacent chains; one chain of such a pair with a NaN in its state under both NaN policies; and the shapes the fused sweep
refuses (odd chain counts, T below one chunk, T = 2), which take the keyed sweep.

Bars: those of tests/test_gpu_fused.py and tests/test_gpu_fused_models.py, whose helpers do the comparing -- against the keyed sweep: x' 1e-9 relative / 1e-10
absolute, the four log totals 1e-12 of their scale, |log alpha| difference below 1e-7, flags equal (fp32: 2e-3, 2e-6, flags where the oracle margin allows);
against the oracle (tests/fused_cases.py): x' 1e-9 / 1e-10, log totals 1e-9 relative, log alpha 1e-7."""
import ctypes as C

import numpy as np
import numpy.testing as npt
import pytest

from tests import fused_cases as FC
from tests.helpers import lg_model
from tests.test_gpu_fused_models import F64, _check_against_oracle, _check_against_unfused, _check_bookkeeping, _same_bits, fused_run

pytestmark = pytest.mark.gpu


def _case(i, d, po, T, Cn, nan_chain=None):
    return FC.Case(100 + i, "S", d, po, T, Cn, 0, nan_chain=nan_chain)


# chunk length 32 at 130 and 258 chains, 16 at 64 and 66 (fused_cases.chunk_len): T = 64 + r leaves a last chunk of r steps in both
TAILS = [_case(r, 4, 2, 64 + r, 130) for r in (1, 2, 3, 4, 5)]
SHAPES = [_case(10, 1, 3, 66, 258), _case(11, 2, 2, 97, 258), _case(12, 4, 4, 65, 64), _case(13, 2, 1, 67, 66), _case(14, 4, 4, 64, 130), _case(15, 1, 1, 69, 130)]
STREAM_RUNS = [(c, "float64") for c in TAILS + SHAPES] + [(c, "float32") for c in (TAILS[0], TAILS[4]) + tuple(SHAPES)]
NAN_PAIR = _case(20, 4, 3, 69, 130, nan_chain=101)   # chains (100, 101) are one pair of adjacent chains: 101 carries the NaN, 100 stays finite


@pytest.mark.parametrize("run", STREAM_RUNS, ids=lambda r: f"{r[0].id}-{r[1]}")
def test_short_last_chunks_and_partial_waves(run):
    """three fused sweeps on a lazy state that stays mixed (missing data: a real accept / reject mix) against the oracle on the checked chains and against the keyed
    sweep on every chain"""
    case, dtname = run
    res = fused_run(case, dtname, "reference")
    _check_bookkeeping(case, res)
    _check_against_oracle(case, dtname, "reference", res, case.checked)
    _check_against_unfused(case, dtname, "reference", res, np.arange(case.C), case.checked)


@pytest.mark.parametrize("Cn,T", [(65, 70), (129, 70), (130, 2), (130, 20), (258, 63)])
def test_refused_shapes_take_the_keyed_sweep(Cn, T):
    """odd chain counts and T < 64 (shorter than the longest chunk) are refused before anything is enqueued: kernel() gives the keyed sweep's numbers bit for bit"""
    from aux_ssm_samplers_amd import _lib, random as R
    from aux_ssm_samplers_amd.kalman.generic import DeviceChains, KalmanSampler
    from aux_ssm_samplers_amd.kalman import LGConcatModel, get_kernel
    h = _lib.default_handle()
    d = 2
    m = lg_model(T, d, dtype=np.float64)
    bt = np.broadcast_to
    model = LGConcatModel(m["m0"], m["P0"], bt(m["F"], (T - 1, d, d)), bt(m["Q"], (T - 1, d, d)), bt(m["b"], (T - 1, d)),
                          bt(m["Hobs"], (T, d, d)), bt(m["Robs"], (T, d, d)), bt(m["cobs"], (T, d)), m["y"])
    init, kernel = get_kernel(model.dynamics_factory, model.observations_factory, model.log_likelihood_fn, True)
    x0 = m["x_true"][None] + 0.3 * np.random.default_rng(4).standard_normal((Cn, T, d))
    a = DeviceChains(h, x0, chain_minor=True)
    b = DeviceChains(h, x0, chain_minor=True, fused=False)
    kernel(R.PRNGKey(11), KalmanSampler(x=a, updated=None), 0.5)
    kernel(R.PRNGKey(11), KalmanSampler(x=b, updated=None), 0.5)
    assert a.fused is False
    npt.assert_array_equal(a.to_host(), b.to_host())
    npt.assert_array_equal(a.logs.to_host(), b.logs.to_host())
    npt.assert_array_equal(a.accepted.to_host(), b.accepted.to_host())


def _raw_sweep(h, model, chains, key, delta, sel, x, x_alt, dtype):
    from aux_ssm_samplers_amd import _lib, random as R
    dl, ybuf, yarr = model.device(h, dtype)
    dims = _lib.Dims(chains.C, chains.T, 1, chains.dx, model.p_obs)
    keys = R.split(key, 3)
    k6 = (C.c_uint32 * 6)(*[int(v) for k in keys for v in np.asarray(k, np.uint32).reshape(2)])
    rc = h.lib.auxssm_kalman_sweep_fused(h.h, _lib.dtype_code(dtype), model.kmodel, C.byref(dims), C.byref(dl.c), C.byref(yarr), float(delta), None, k6, 1,
                                         _lib.NAN_REFERENCE, chains.layout, x.ptr, x_alt.ptr, sel.ptr, chains.u_acc.ptr, chains.accepted.ptr, chains.logs.ptr)
    _lib.check(rc)


@pytest.mark.parametrize("pattern", ["differs", "agrees"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_selector_inside_pairs_of_adjacent_chains(dtype, pattern):
    """the state scattered over the ping-pong pair (the other buffer's slots hold garbage) by a selector that alternates 0 / 1 from chain to chain, or is the same
    for chains (2 k, 2 k + 1) and alternates from pair to pair: the sweep of the gathered state bit for bit, every proposal in the buffer its chain's selector names"""
    from aux_ssm_samplers_amd import _lib, random as R
    from aux_ssm_samplers_amd.kalman.generic import DeviceChains, KalmanSampler
    h = _lib.default_handle()
    case = TAILS[2]
    Cn = case.C
    model = case.model()
    from aux_ssm_samplers_amd.kalman.generic import _get_device_kernel
    kernel = _get_device_kernel(model, True, nan_policy="reference")[1]
    x0 = case.x0.astype(dtype)
    key = R.PRNGKey(321)
    ref = DeviceChains(h, x0, chain_minor=True)
    kernel(key, KalmanSampler(x=ref, updated=None), 0.4)
    assert ref.fused is True
    acc = ref.accepted.to_host()
    assert 0 < acc.sum() < Cn
    xr, lr = ref.to_host(), ref.logs.to_host()
    sel0 = (np.arange(Cn) % 2 if pattern == "differs" else (np.arange(Cn) // 2) % 2).astype(np.int32)
    cm = lambda a: np.ascontiguousarray(np.asarray(a, dtype).transpose(1, 2, 0))
    junk = np.random.default_rng(2).standard_normal(x0.shape).astype(dtype) * 100
    ch = DeviceChains(h, x0, chain_minor=True)
    ch.x.copy_from_host(cm(np.where(sel0[:, None, None] == 0, x0, junk)))
    ch.x_alt = h.to_device(cm(np.where(sel0[:, None, None] == 1, x0, junk)), dtype)
    ch.sel = h.to_device(sel0, np.int32)
    _raw_sweep(h, model, ch, key, 0.4, ch.sel, ch.x, ch.x_alt, dtype)
    ch._lazy_dirty = True
    npt.assert_array_equal(ch.accepted.to_host(), acc)
    npt.assert_array_equal(ch.sel.to_host(), sel0 ^ acc)
    npt.assert_array_equal(ch.logs.to_host(), lr)
    npt.assert_array_equal(ch.to_host(), xr)


@pytest.mark.parametrize("variant", ["mid", "first"])
@pytest.mark.parametrize("policy", ["reference", "masked"])
def test_nan_in_one_chain_of_a_pair(policy, variant):
    """chain 101 has a NaN in its state, its neighbour 100 is finite: 100 and the rest of the wave meet the oracle and the keyed sweep, 100's first sweep is its
    sweep in the run without the NaN to the same bars, and the NaN chain is rejected with its state bit for bit unchanged"""
    case, dtname = NAN_PAIR, "float64"
    nc, mate = case.nan_chain, case.nan_chain - 1
    res = fused_run(case, dtname, policy, variant)
    clean = fused_run(case, dtname, policy)
    others = [c for c in case.nan_wave if c != nc]
    _check_bookkeeping(case, res)
    _check_against_oracle(case, dtname, policy, res, others)
    _check_against_unfused(case, dtname, policy, res, [c for c in range(case.C) if c != nc], others)
    a, b = res[0], clean[0]   # the first sweep starts from the same state in both runs
    npt.assert_allclose(a["prop"][mate], b["prop"][mate], **F64)
    scale = np.abs(b["logs"][mate, 1:]).max()
    npt.assert_allclose(a["logs"][mate, 1:], b["logs"][mate, 1:], rtol=0, atol=1e-12 * scale)
    assert abs(a["logs"][mate, 0] - b["logs"][mate, 0]) < 1e-7 and a["accepted"][mate] == b["accepted"][mate]
    for i, rec in enumerate(res):
        assert np.isnan(rec["logs"][nc, 0]) and rec["accepted"][nc] == 0 and rec["sel_new"][nc] == 0, i
        assert _same_bits(rec["new"][nc], res[0]["prev"][nc]) and np.isnan(rec["new"][nc]).sum() == 1, i
