"""GPU: the RTS smoother (auxssm_kalman_smooth, `smoothing`, `filter_smoothing`) against the reference's stored smoother answers and
the oracle's sequential smoother, at the sizes that reach every scan form.

T = 1, 2, 3, 5: one chunk.  T = 70: 18 chunks of 4, the last holding 2 elements.  T = 300: 75 chunks, two groups of 64 with the second
partial, still below the tile scan's threshold of 512.  T = 600 (one sequence): the tile scan, three tiles, the last with 88 live lanes.

fp64 bars: rtol 1e-7 / atol 1e-9 against the oracle and the stored answers (the pathwise sampler's bar in tests/test_gpu_kalman.py and
tests/test_golden.py); two device results that must agree "at 1e-9 relative" are compared entry by entry at rtol 1e-9 / atol 1e-10, as
the sampler's and the filter's parallel-against-sequential tests are.

fp32: FP32_BAR_MEAN / FP32_BAR_COV bound max |device - oracle| / max |oracle| per case, the oracle being the fp64 sequential smoother on
the same fp32-rounded inputs, over T in T_LIST, dx in {1, 4}, both `parallel` values.  Measured on one MI355X: worst mean 1.547e-06 and
worst covariance 1.288e-05 (both at dx = 4, T = 600, sequential; the tile scan gave 1.531e-06 / 1.287e-05; dx = 1 stays below 1.6e-07 and
every T <= 300 below 2.3e-06); the bars are twice the worst figure, rounded up to one significant digit.  The smallest eigenvalue of any
fp32 sPs[t] was 2.005e-01 (dx = 1, T = 600), equal to the oracle's to the four digits printed: it never went negative.
"""
import ctypes as C

import numpy as np
import numpy.testing as npt
import pytest

from oracle import kalman_np as K
from tests.helpers import ref_lgssm_inputs, ref_batched_inputs
from tests.test_kalman_smoother_host import G, SMOOTH_CASES, LG

pytestmark = pytest.mark.gpu
TOL = dict(rtol=1e-7, atol=1e-9)
T_LIST = [1, 2, 3, 5, 70, 300, 600]

FP32_BAR_MEAN = 4e-6   # 2 x 1.547e-06
FP32_BAR_COV = 3e-5    # 2 x 1.288e-05


@pytest.fixture(scope="module")
def P():
    import aux_ssm_samplers_amd._primitives.kalman as prim
    return prim


def _close_rel(a, b):
    npt.assert_allclose(a, b, rtol=1e-9, atol=1e-10)


_CACHE = {}


def _oracle(T, dx, dtype=np.float64):
    """model, filtered moments and the oracle's smoothed moments; dtype float32: every input rounded to fp32 first, the arithmetic stays fp64"""
    key = ("o", T, dx, np.dtype(dtype).name)
    if key not in _CACHE:
        ys, lg = ref_lgssm_inputs(42 + T, T, dx, 3)
        r = lambda a: np.asarray(a, dtype).astype(np.float64)
        lg = tuple(r(a) for a in lg)
        ms, Ps, _ = K.filtering(ys, lg, False)
        ms, Ps = r(ms), r(Ps)
        _CACHE[key] = (lg, ms, Ps) + K.explicit_smoother(ms, Ps, lg[2], lg[3], lg[4])
    return _CACHE[key]


def _device(P, T, dx, parallel, dtype=np.float64):
    key = ("d", T, dx, bool(parallel), np.dtype(dtype).name)
    if key not in _CACHE:
        lg, ms, Ps, _, _ = _oracle(T, dx, dtype)
        _CACHE[key] = P.smoothing(ms.astype(dtype), Ps.astype(dtype), P.LGSSM(*[a.astype(dtype) for a in lg]), parallel)
    return _CACHE[key]


@pytest.mark.parametrize("name", SMOOTH_CASES)
@pytest.mark.parametrize("parallel", [False, True])
def test_vs_reference_answers(P, name, parallel):
    assert len(SMOOTH_CASES) == 16
    lg = tuple(G[f"{name}/{k}"] for k in LG)
    sm, sP = P.smoothing(G[f"{name}/ms"], G[f"{name}/Ps"], P.LGSSM(*lg), parallel)
    npt.assert_allclose(sm, G[f"{name}/sm"], **TOL)
    npt.assert_allclose(sP, G[f"{name}/sP"], **TOL)


@pytest.mark.parametrize("T", T_LIST)
@pytest.mark.parametrize("dx", [1, 2, 3, 4])
@pytest.mark.parametrize("parallel", [False, True])
def test_vs_oracle(P, T, dx, parallel):
    _, ms, Ps, esm, esP = _oracle(T, dx)
    sm, sP = _device(P, T, dx, parallel)
    assert sm.shape == (T, dx) and sP.shape == (T, dx, dx) and sm.dtype == np.float64
    npt.assert_allclose(sm, esm, **TOL)
    npt.assert_allclose(sP, esP, **TOL)
    npt.assert_array_equal(sP, np.swapaxes(sP, -1, -2))
    npt.assert_array_equal(sm[-1], ms[-1])


@pytest.mark.parametrize("T", T_LIST)
@pytest.mark.parametrize("dx", [1, 2, 3, 4])
def test_parallel_equals_sequential(P, T, dx):
    (sm1, sP1), (sm0, sP0) = _device(P, T, dx, True), _device(P, T, dx, False)
    _close_rel(sm1, sm0)
    _close_rel(sP1, sP0)


@pytest.mark.parametrize("T,dx", [(70, 4), (600, 4), (70, 1), (600, 2)])
@pytest.mark.parametrize("parallel", [False, True])
def test_mean_equals_the_sampler_without_noise(P, T, dx, parallel):
    lg, ms, Ps, _, _ = _oracle(T, dx)
    xs = P.sampling(None, ms, Ps, P.LGSSM(*lg), parallel, eps=np.zeros((T, dx)))
    _close_rel(_device(P, T, dx, parallel)[0], xs)


@pytest.mark.parametrize("seed", [42, 666])
@pytest.mark.parametrize("parallel", [False, True])
def test_batched_equals_block_diag(P, seed, parallel):
    T, dx, dy, B = 5, 2, 3, 3
    (bys, blg), (ys, lg) = ref_batched_inputs(seed, T, dx, dy, B)
    bms, bPs, _ = K.filtering(bys, blg, False)
    ms, Ps, _ = K.filtering(ys, lg, False)
    esm, esP = K.explicit_smoother(ms, Ps, lg[2], lg[3], lg[4])
    sm, sP = P.smoothing(bms, bPs, P.LGSSM(*blg), parallel)
    assert sm.shape == (T, B, dx) and sP.shape == (T, B, dx, dx)
    npt.assert_allclose(sm.reshape(T, B * dx), esm, **TOL)
    for b in range(B):
        npt.assert_allclose(sP[:, b], esP[:, b * dx:(b + 1) * dx, b * dx:(b + 1) * dx], **TOL)


def _smooth_c(h, dl, dims, msd, Psd, parallel, dtype=np.float64):
    from aux_ssm_samplers_amd import _lib
    sms, sPs = h.empty(msd.shape, dtype), h.empty(Psd.shape, dtype)
    _lib.check(h.lib.auxssm_kalman_smooth(h.h, _lib.dtype_code(dtype), C.byref(dims), C.byref(dl.c), msd.ptr, Psd.ptr, int(parallel), sms.ptr, sPs.ptr))
    return sms.to_host(), sPs.to_host()


@pytest.mark.parametrize("T", [70, 600])
@pytest.mark.parametrize("per_chain_model", [False, True])
@pytest.mark.parametrize("parallel", [False, True])
def test_chains_through_the_c_abi(T, per_chain_model, parallel):
    """C = 3 chains in one call -- a chain-shared model (chain stride 0) with per-chain moments, and a model per chain -- against each chain's own
    single-chain call, bit for bit: the plan is the same with one and with three sequences (T = 70: 18 chunks of 4; T = 600: the tile scan, three tiles
    per sequence, so a workgroup's (sequence, tile) decode is exercised with more than one sequence)."""
    from aux_ssm_samplers_amd import _lib
    from aux_ssm_samplers_amd._primitives.kalman.base import DeviceLGSSM
    Cn, dx = 3, 3
    h = _lib.default_handle()
    lgs, mss, Pss = [], [], []
    for c in range(Cn):
        ys, lg = ref_lgssm_inputs(7 + (c if per_chain_model else 0), T, dx, 3)
        ys = ys + c
        m, Pc, _ = K.filtering(ys, lg, False)
        lgs.append(lg), mss.append(m), Pss.append(Pc)
    five = lambda lg: list(lg[:5]) + [None, None, None]
    if per_chain_model:
        dl = DeviceLGSSM(h, five([np.stack([lg[k] for lg in lgs]) for k in range(5)]), Cn, T, 1, dx, 1, False, np.float64, chain_axis=True)
        assert dl.c.Fs.sc == (T - 1) * dx * dx
    else:
        dl = DeviceLGSSM(h, five(lgs[0]), 1, T, 1, dx, 1, False, np.float64)
        assert dl.c.Fs.sc == 0
    msd = h.to_device(np.stack(mss).reshape(Cn, T, 1, dx))
    Psd = h.to_device(np.stack(Pss).reshape(Cn, T, 1, dx, dx))
    sm, sP = _smooth_c(h, dl, _lib.Dims(Cn, T, 1, dx, 1), msd, Psd, parallel)
    for c in range(Cn):
        d1 = DeviceLGSSM(h, five(lgs[c]), 1, T, 1, dx, 1, False, np.float64)
        sm1, sP1 = _smooth_c(h, d1, _lib.Dims(1, T, 1, dx, 1), h.to_device(mss[c].reshape(1, T, 1, dx)), h.to_device(Pss[c].reshape(1, T, 1, dx, dx)), parallel)
        npt.assert_array_equal(sm[c], sm1[0])
        npt.assert_array_equal(sP[c], sP1[0])
        esm, esP = K.explicit_smoother(mss[c], Pss[c], lgs[c][2], lgs[c][3], lgs[c][4])
        npt.assert_allclose(sm[c, :, 0], esm, **TOL)
        npt.assert_allclose(sP[c, :, 0], esP, **TOL)


@pytest.mark.parametrize("T,dx,dy", [(5, 2, 3), (7, 1, 1), (70, 4, 3)])
@pytest.mark.parametrize("parallel", [False, True])
def test_filter_smoothing_with_missing_observations(P, T, dx, dy, parallel):
    ys, lg = ref_lgssm_inputs(5, T, dx, dy, nan_index=True)
    ms, Ps, ell = K.filtering(ys, lg, False)
    esm, esP = K.explicit_smoother(ms, Ps, lg[2], lg[3], lg[4])
    sm, sP, ell_d = P.filter_smoothing(ys, P.LGSSM(*lg), parallel)
    npt.assert_allclose(sm, esm, **TOL)
    npt.assert_allclose(sP, esP, **TOL)
    npt.assert_allclose(ell_d, ell, **TOL)
    npt.assert_array_equal(ell_d, P.filtering(ys, P.LGSSM(*lg), parallel)[2])


def test_fp32_vs_fp64_oracle(P):
    worst_m = worst_P = 0.0
    min_eig = np.inf
    for dx in (1, 4):
        for T in T_LIST:
            _, _, _, esm, esP = _oracle(T, dx, np.float32)
            for parallel in (False, True):
                sm, sP = _device(P, T, dx, parallel, np.float32)
                assert sm.dtype == np.float32 and sP.dtype == np.float32
                em = np.max(np.abs(sm - esm)) / np.max(np.abs(esm))
                eP = np.max(np.abs(sP - esP)) / np.max(np.abs(esP))
                ev = np.linalg.eigvalsh(sP.astype(np.float64)).min()
                print(f"fp32 smoother dx={dx} T={T} parallel={int(parallel)}: rel err mean {em:.3e} cov {eP:.3e} min eig {ev:.3e} (oracle min eig {np.linalg.eigvalsh(esP).min():.3e})")
                worst_m, worst_P, min_eig = max(worst_m, em), max(worst_P, eP), min(min_eig, ev)
                npt.assert_array_equal(sP, np.swapaxes(sP, -1, -2))
    print(f"fp32 smoother worst: mean {worst_m:.3e} cov {worst_P:.3e} min eig {min_eig:.3e}")
    assert worst_m <= FP32_BAR_MEAN, worst_m
    assert worst_P <= FP32_BAR_COV, worst_P
    assert min_eig > 0, min_eig


def test_c_level_refusals():
    from aux_ssm_samplers_amd import _lib
    from aux_ssm_samplers_amd._primitives.kalman.base import DeviceLGSSM
    h = _lib.default_handle()
    lib = h.lib

    def call(T, dx, ms, Ps, sms, sPs):
        ys, lg = ref_lgssm_inputs(3, T, dx, 1)
        dl = DeviceLGSSM(h, list(lg[:5]) + [None, None, None], 1, T, 1, dx, 1, False, np.float64)
        dims = _lib.Dims(1, T, 1, dx, 1)
        return lib.auxssm_kalman_smooth(h.h, _lib.F64, C.byref(dims), C.byref(dl.c), ms, Ps, 1, sms, sPs)

    T = 4
    for dx in (5, 2):
        ms, Ps = h.zeros((1, T, 1, dx), np.float64), h.zeros((1, T, 1, dx, dx), np.float64)
        sms, sPs = h.to_device(np.ones((1, T, 1, dx))), h.to_device(np.ones((1, T, 1, dx, dx)))
        if dx == 5:
            assert call(T, dx, ms.ptr, Ps.ptr, sms.ptr, sPs.ptr) == -2   # AUXSSM_ERR_UNSUPPORTED
            msg = lib.auxssm_last_error().decode()
            assert "dx <= 4" in msg and "auxssm_kalman_sample" in msg
        else:
            assert call(T, dx, ms.ptr, Ps.ptr, None, sPs.ptr) == -1      # AUXSSM_ERR_ARG
            assert call(T, dx, ms.ptr, Ps.ptr, sms.ptr, None) == -1
            assert call(T, dx, ms.ptr, Ps.ptr, ms.ptr, sPs.ptr) == -1    # sms == ms
            assert "alias" in lib.auxssm_last_error().decode()
            assert call(T, dx, ms.ptr, Ps.ptr, sms.ptr, Ps.ptr) == -1
        h.sync()
        assert (sms.to_host() == 1).all() and (sPs.to_host() == 1).all()  # nothing was enqueued: the outputs are untouched
    assert call(T, 2, ms.ptr, Ps.ptr, sms.ptr, sPs.ptr) == 0
    h.sync()
    assert not sms.to_host().any() and not sPs.to_host().any()            # (zero moments smooth to zero)
