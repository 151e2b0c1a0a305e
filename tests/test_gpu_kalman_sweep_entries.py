"""The four entry points of the auxiliary Kalman sweep -- auxssm_kalman_sweep (host step size, explicit noise), auxssm_kalman_sweep_dd (the same step size
resident on the device), auxssm_kalman_sweep_keyed (the library draws the noise from the keys) and auxssm_kalman_sweep_fused -- funnel into one driver per
device model (csrc/api.hip: sweep_lg_concat, sweep_sv, sweep_lorenz, sweep_lg_concat_fused).  For every model kind, at the smallest sizes at which each
driver branch is live, the first three must agree bit for bit on x, accepted and logs, and what an entry point cannot run it must refuse before it enqueues
anything."""
import ctypes as C

import numpy as np
import numpy.testing as npt
import pytest

from aux_ssm_samplers_amd import _lib
from aux_ssm_samplers_amd.kalman import DeviceChains, LGConcatModel, SVModel
from tests.helpers import lorenz_kalman_setup, sv_setup

pytestmark = pytest.mark.gpu

T = 5
KEYS = (11, 22, 33, 44, 55, 66)  # {aux0, aux1, samp0, samp1, acc0, acc1}
DTYPES = [np.float64, np.float32]
LAYOUTS = [(3, False), (34, True)]  # (chains, chain-minor)


def _lg(dx, dy):
    """a time-varying linear-Gaussian model with dy observed combinations of a dx-dimensional state"""
    rng = np.random.default_rng(100 * dx + dy)
    rep = lambda a, n: np.ascontiguousarray(np.broadcast_to(a, (n,) + a.shape))
    A = rng.standard_normal((dy, dy))
    return LGConcatModel(0.1 * rng.standard_normal(dx), np.eye(dx), rep(0.9 * np.eye(dx) + 0.03 * rng.standard_normal((dx, dx)), T - 1),
                         rep(0.1 * np.eye(dx), T - 1), rep(0.01 * rng.standard_normal(dx), T - 1), rep(rng.standard_normal((dy, dx)), T),
                         rep(0.5 * np.eye(dy) + A @ A.T / dy, T), rep(0.1 * rng.standard_normal(dy), T), rng.standard_normal((T, dy)))


def _sv(order, d=2):
    y, _, (m0, P0, F, Q, b) = sv_setup(T, d)
    return SVModel(y, m0, P0, F, Q, b, order=order)


# name -> (model, step size, whether the path takes the chain-minor layout)
MODELS = {
    "lg_2x3": (lambda: _lg(2, 3), 0.4, True),       # the register kernels
    "lg_6x6": (lambda: _lg(6, 6), 0.4, False),      # the wide-state path: dense only
    "sv1": (lambda: _sv(1), 0.05, True),
    "sv2": (lambda: _sv(2), 0.05, True),
    "lorenz": (lambda: lorenz_kalman_setup(T, every=2, dt=1e-3)[0], 1e-3, True),
}


def _x0(model, Cn, dtype):
    return (0.3 * np.random.default_rng(7).standard_normal((Cn, T, model.dx))).astype(dtype)


def _sweep(h, model, ch, entry, delta, layout=None):
    """one sweep of the resident chains through `entry` ("host", "dd", "keyed"); returns the status, nothing is checked"""
    dl, _, yarr = model.device(h, ch.dtype)
    dims = _lib.Dims(ch.C, T, 1, ch.dx, model.p_obs)
    head = (h.h, _lib.dtype_code(ch.dtype), model.kmodel, C.byref(dims), C.byref(dl.c), C.byref(yarr))
    tail = (1, _lib.NAN_REFERENCE, ch.layout if layout is None else layout, ch.x.ptr, ch.eps_aux.ptr, ch.eps_samp.ptr, ch.u_acc.ptr, ch.accepted.ptr, ch.logs.ptr)
    if entry == "host":
        return h.lib.auxssm_kalman_sweep(*head, float(delta), *tail)
    if entry == "dd":
        ch.delta_dev = h.to_device(np.full(1, delta, ch.dtype))  # (kept alive with the chains: the sweep is asynchronous)
        return h.lib.auxssm_kalman_sweep_dd(*head, ch.delta_dev.ptr, *tail)
    return h.lib.auxssm_kalman_sweep_keyed(*head, float(delta), None, (C.c_uint32 * 6)(*KEYS), *tail)


def _results(ch):
    return ch.to_host(), ch.accepted.to_host(), ch.logs.to_host()


# (the wide-state path in the chain-minor layout is a refusal: test_wide_path_refuses_the_chain_minor_layout)
CASES = [(name, Cn, cm) for name in MODELS for Cn, cm in LAYOUTS if MODELS[name][2] or not cm]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,Cn,chain_minor", CASES)
def test_host_device_delta_and_keyed_entries_agree_bit_for_bit(name, Cn, chain_minor, dtype):
    make, delta, _ = MODELS[name]
    h = _lib.default_handle()
    model = make()
    x0 = _x0(model, Cn, dtype)
    keyed = DeviceChains(h, x0, chain_minor=chain_minor)
    _lib.check(_sweep(h, model, keyed, "keyed", delta))
    want = _results(keyed)
    for entry in ("host", "dd"):
        ch = DeviceChains(h, x0, chain_minor=chain_minor)
        h.kalman_draw(KEYS[0:2], KEYS[2:4], KEYS[4:6], ch.eps_aux, ch.eps_samp, ch.u_acc)  # the explicit arrays: what the same keys draw
        _lib.check(_sweep(h, model, ch, entry, delta))
        for got, ref, what in zip(_results(ch), want, ("x", "accepted", "logs")):
            npt.assert_array_equal(got, ref, err_msg=f"{name} {entry} {what}")
    assert np.all(np.isfinite(want[2])) and np.all(want[2][:, 1:] != 0)  # (a sweep happened: every chain's four log-densities were written)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["sv1", "sv2", "lorenz"])
def test_fused_entry_refuses_other_model_kinds_with_nothing_enqueued(name, dtype):
    h = _lib.default_handle()
    model = MODELS[name][0]()
    Cn = 34
    x0 = _x0(model, Cn, dtype)
    ch = DeviceChains(h, x0, chain_minor=True)
    x_alt, sel = h.zeros(ch.x.shape, ch.dtype), h.zeros((Cn,), np.int32)
    dl, _, yarr = model.device(h, ch.dtype)
    dims = _lib.Dims(Cn, T, 1, ch.dx, model.p_obs)
    rc = h.lib.auxssm_kalman_sweep_fused(h.h, _lib.dtype_code(ch.dtype), model.kmodel, C.byref(dims), C.byref(dl.c), C.byref(yarr), MODELS[name][1], None,
                                         (C.c_uint32 * 6)(*KEYS), 1, _lib.NAN_REFERENCE, ch.layout, ch.x.ptr, x_alt.ptr, sel.ptr, ch.u_acc.ptr, ch.accepted.ptr,
                                         ch.logs.ptr)
    assert rc == _lib.ERR_UNSUPPORTED
    assert h.lib.auxssm_last_error().decode() == (f"auxssm_kalman_sweep_fused runs AUXSSM_KMODEL_LG_CONCAT (model_kind {model.kmodel}: "
                                                  "use auxssm_kalman_sweep_keyed)")
    npt.assert_array_equal(ch.to_host(), x0)
    assert not x_alt.to_host().any() and not sel.to_host().any() and not ch.accepted.to_host().any() and not ch.logs.to_host().any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_wide_path_refuses_the_chain_minor_layout(dtype):
    h = _lib.default_handle()
    for model, delta, msg in ((_lg(6, 6), 0.4, "(dx=6, dy=12) runs the wide-state path, which takes the dense (C, T, dx) layout only"),
                              (_sv(1, d=6), 0.05, "dx=6 runs the wide-state path, which takes the dense (C, T, dx) layout only")):
        x0 = _x0(model, 34, dtype)
        ch = DeviceChains(h, x0, chain_minor=True)
        h.kalman_draw(KEYS[0:2], KEYS[2:4], KEYS[4:6], ch.eps_aux, ch.eps_samp, ch.u_acc)
        assert _sweep(h, model, ch, "host", delta) == _lib.ERR_UNSUPPORTED
        assert h.lib.auxssm_last_error().decode() == msg
        npt.assert_array_equal(ch.to_host(), x0)
        assert not ch.accepted.to_host().any()
