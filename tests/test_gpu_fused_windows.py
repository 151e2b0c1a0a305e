"""64-step chunks of the fused sweep (csrc/fused_shared.h) at the shapes where a chunk spans two 32-row windows, and the chunk rule's clause for 256 chains.

These cases were written for a pass AC that keeps 32 coefficient rows in LDS and restages at every 32nd step of a chunk between two barriers.  That form was
measured against whole-chunk staging and not kept ("64-step chunks from 256 chains"); the cases stay, because they are the smallest shapes
at which a 64-step chunk, its ragged neighbours and a ragged chain tile meet, and no other test runs them together.  Short T selects 64 steps from 1024 chains on:
    T = 64    one chunk of 64 steps                      T = 69    a second chunk of 5 steps
    T = 130   a third chunk of 2 steps                   T = 197   a ragged fourth chunk of 5 steps
    C = 1026  a fifth chain tile with two live lanes and three idle waves, and 62 idle lanes in its first wave
Method and tolerances of tests/test_gpu_fused.py::test_fused_equals_keyed_sweep: three consecutive sweeps (delta 0.5, 0.5, 0.2) from a lazy state, the fused sweep
against the keyed one (fused=False) after every sweep.  One time-varying (3, 2) model with missing rows (tests/fused_cases.py), rows forced at 31 | 32 (the
middle of chunk 0) and 63 | 64 (a chunk boundary), under both NaN policies.  One case at the smallest shape at which a 256-CU device takes 64-step chunks from
256 chains (T = 65536, d = 1): it asserts agreement with the keyed sweep, not the chunk length, so it also holds on a partition with fewer compute units."""
import numpy as np
import numpy.testing as npt
import pytest

from tests import fused_cases as FC
from tests.helpers import lg_model

pytestmark = pytest.mark.gpu

DELTAS = (0.5, 0.5, 0.2)


def _bt(a, n):
    return np.broadcast_to(a, (n,) + a.shape)


def _lg(T, d, dtype):
    from aux_ssm_samplers_amd.kalman import LGConcatModel
    m = lg_model(T, d, dtype=dtype)
    return m, LGConcatModel(m["m0"], m["P0"], _bt(m["F"], T - 1), _bt(m["Q"], T - 1), _bt(m["b"], T - 1), _bt(m["Hobs"], T), _bt(m["Robs"], T), _bt(m["cobs"], T), m["y"])


def _tv(T, d, po, y=None):
    from aux_ssm_samplers_amd.kalman import LGConcatModel
    m = FC.tv_model(T, d, po, 0)
    return m, LGConcatModel(m["m0"], m["P0"], m["Fs"], m["Qs"], m["bs"], m["Hs"], m["Rs"], m["cs"], m["y"] if y is None else y)


def _tol(dtype):
    return dict(rtol=1e-9, atol=1e-10) if dtype == np.float64 else dict(rtol=2e-3, atol=2e-3)


def _compare(a, b, dtype, exact_posterior):
    la, lb = a.logs.to_host(), b.logs.to_host()
    npt.assert_array_equal(a.accepted.to_host(), b.accepted.to_host())
    npt.assert_allclose(a.to_host(), b.to_host(), **_tol(dtype))
    scale = np.abs(lb[:, 1:]).max()
    npt.assert_allclose(la[:, 1:], lb[:, 1:], rtol=0, atol=(1e-12 if dtype == np.float64 else 2e-6) * scale)
    if exact_posterior:  # log alpha is the difference of the four totals: identically 0 when nothing is missing
        assert np.abs(la[:, 0]).max() < (1e-7 if dtype == np.float64 else 5e-2)
    else:
        npt.assert_allclose(la[:, 0], lb[:, 0], rtol=0, atol=1e-7)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("d,po", [(4, 4), (1, 1), (3, 2)])
@pytest.mark.parametrize("T,Cn", [(64, 1024), (69, 1024), (130, 1024), (197, 1024), (197, 1026)])
def test_64_step_chunks_equal_keyed_sweep(T, Cn, d, po, dtype):
    from aux_ssm_samplers_amd import _lib, random as R
    from aux_ssm_samplers_amd.kalman import get_kernel
    from aux_ssm_samplers_amd.kalman.generic import DeviceChains, KalmanSampler
    h = _lib.default_handle()
    m, model = _lg(T, d, dtype) if d == po else _tv(T, d, po)
    _, kernel = get_kernel(model.dynamics_factory, model.observations_factory, model.log_likelihood_fn, True)
    x0 = (m["x_true"][None] + 0.3 * np.random.default_rng(0).standard_normal((Cn, T, d))).astype(dtype)
    a = DeviceChains(h, x0, chain_minor=True)               # fused, lazy state
    b = DeviceChains(h, x0, chain_minor=True, fused=False)  # the keyed sweep
    for i, delta in enumerate(DELTAS):
        key = R.PRNGKey(40 + i)
        kernel(key, KalmanSampler(x=a, updated=None), delta)
        kernel(key, KalmanSampler(x=b, updated=None), delta)
        assert a.fused is True and b.fused is False
        _compare(a, b, dtype, True)
    assert a.accepted.to_host().all()


@pytest.mark.parametrize("policy", ["reference", "masked"])
def test_missing_rows_inside_and_on_the_boundary_of_a_64_step_chunk(policy):
    """rows 31 | 32 lie in the middle of chunk 0, rows 63 | 64 straddle the boundary of chunks 0 and 1 (whole | one component missing); fp64"""
    from aux_ssm_samplers_amd import _lib, random as R
    from aux_ssm_samplers_amd.kalman.generic import DeviceChains, KalmanSampler, _get_device_kernel
    h = _lib.default_handle()
    T, d, po, Cn = 197, 3, 2, 1026
    m, _ = _tv(T, d, po)
    y = FC.missing(m["y"], {0: "whole", 31: "whole", 32: "partial", 63: "whole", 64: "partial", T - 1: "partial"}, np.random.default_rng(11))
    assert np.isnan(y[31]).all() and np.isnan(y[32]).sum() == 1 and np.isnan(y[63]).all() and np.isnan(y[64]).sum() == 1
    _, model = _tv(T, d, po, y)
    kernel = _get_device_kernel(model, True, nan_policy=policy)[1]
    x0 = m["x_true"][None] + 0.3 * np.random.default_rng(1).standard_normal((Cn, T, d))
    a = DeviceChains(h, x0, chain_minor=True)
    b = DeviceChains(h, x0, chain_minor=True, fused=False)
    for i, delta in enumerate(DELTAS):
        key = R.PRNGKey(60 + i)
        kernel(key, KalmanSampler(x=a, updated=None), delta)
        kernel(key, KalmanSampler(x=b, updated=None), delta)
        assert a.fused is True and b.fused is False
        _compare(a, b, np.float64, policy == "masked")
    if policy == "masked":  # (the proposal is the exact posterior; the reference policy drops the steps with a missing component and rejects chains)
        assert a.accepted.to_host().all()


def test_chunk_rule_at_256_chains_long_series():
    """T = 65536, 256 chains, d = 1, fp64 (134 MB per state buffer): two sweeps, so the second starts from a flipped selector; one comparison at the end"""
    from aux_ssm_samplers_amd import _lib, random as R
    from aux_ssm_samplers_amd.kalman import get_kernel
    from aux_ssm_samplers_amd.kalman.generic import DeviceChains, KalmanSampler
    h = _lib.default_handle()
    T, d, Cn, dtype = 65536, 1, 256, np.float64
    m, model = _lg(T, d, dtype)
    _, kernel = get_kernel(model.dynamics_factory, model.observations_factory, model.log_likelihood_fn, True)
    x0 = m["x_true"][None] + 0.3 * np.random.default_rng(2).standard_normal((Cn, T, d))
    a = DeviceChains(h, x0, chain_minor=True)
    b = DeviceChains(h, x0, chain_minor=True, fused=False)
    for i, delta in enumerate((0.5, 0.2)):
        key = R.PRNGKey(80 + i)
        kernel(key, KalmanSampler(x=a, updated=None), delta)
        kernel(key, KalmanSampler(x=b, updated=None), delta)
    assert a.fused is True and b.fused is False
    _compare(a, b, dtype, True)
    assert a.accepted.to_host().all()
