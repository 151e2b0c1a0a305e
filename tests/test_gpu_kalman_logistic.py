"""kalman.BinomialModel and kalman.NegBinomialModel on the device (AUXSSM_KMODEL_LOGISTIC_FIRST / _SECOND: the SV sweep's kernels instantiated for the logistic
potential, which reads a size array beside the data) against the oracle's sweep (oracle.kalman_np.kalman_sweep) driven by the models' own NumPy factories, on
identical explicit noise and in fp64 at 1e-9: x at rtol 1e-9 / atol 1e-10, the four log terms at rtol 1e-9, log alpha at atol 1e-9 times the size of the terms it
is the difference of.  The cells, their missing entries and the placed acceptance uniforms are tests/kalman_logistic_cases.py's: every chain the oracle ran has a
margin |log alpha - log u| >= 0.05, so an accept flag that differs is a defect.  Then: the layouts against each other, host states against resident chains,
loop() with the step size on the device, jax compatibility, the C entry points, fp32 against the fp64 oracle (bars from measured errors), and the sampler against
the exact posterior by quadrature and against sequential particle Gibbs on the same density stated as a user program."""
import ctypes as C
import functools

import numpy as np
import numpy.testing as npt
import pytest

from tests import kalman_logistic_cases as LC

pytestmark = pytest.mark.gpu


def fns(model):
    return model.dynamics_factory, model.observations_factory, model.log_likelihood_fn


def resident_sweep(cell, u, dtype=np.float64, chain_minor=False, delta=None):
    """one sweep of all the cell's chains on resident buffers -> (x (C, T, d), flags (C,) bool, logs (C, 5))"""
    from aux_ssm_samplers_amd import _lib
    from aux_ssm_samplers_amd.kalman import get_kernel
    from aux_ssm_samplers_amd.kalman.generic import DeviceChains, KalmanSampler
    init, kernel = get_kernel(*fns(cell["model"]), cell.get("parallel", True))
    chains = DeviceChains(_lib.default_handle(), cell["x"].astype(dtype), chain_minor=chain_minor)
    assert chains.chain_minor == chain_minor
    kernel(None, KalmanSampler(x=chains, updated=None), cell["delta"] if delta is None else delta,
           noise=dict(eps_aux=cell["eps_aux"], eps_samp=cell["eps_samp"], u_accept=u))
    return chains.to_host(), chains.accepted.to_host() != 0, chains.logs.to_host()


def la_atol(ref_logs):
    """log alpha is a difference of the four log terms: 1e-9 relative to the largest of them (a start state that reaches |x| = 30 puts them at 1e4)"""
    return 1e-9 * np.maximum(1.0, np.abs(ref_logs[:, 1:]).max(axis=1))


def check_against_oracle(ref, x, flags, logs, u_index=0):
    """the oracle's chains of one resident sweep"""
    cell, idx = ref["cell"], ref["chains"]
    npt.assert_allclose(logs[idx, 1:], ref["logs"][:, 1:], rtol=1e-9)
    assert np.all(np.abs(logs[idx, 0] - ref["logs"][:, 0]) <= la_atol(ref["logs"]) + 1e-9 * np.abs(ref["logs"][:, 0]))
    npt.assert_array_equal(flags[idx], ref["accepted"][u_index])
    want = np.where(ref["accepted"][u_index][:, None, None], ref["x_prop"], cell["x"][idx])
    npt.assert_allclose(x[idx], want, rtol=1e-9, atol=1e-10)


def with_share(share, f):
    from aux_ssm_samplers_amd import _lib
    h = _lib.default_handle()
    h.set_option(_lib.OPT_SHARE_MODEL, share)
    try:
        return f()
    finally:
        h.set_option(_lib.OPT_SHARE_MODEL, 1)


# ---- fp64 parity ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", LC.FAMILIES)
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("d,T", LC.DENSE_SHAPES)
@pytest.mark.parametrize("parallel", [True, False])
def test_dense_one_chain_vs_oracle(family, order, d, T, parallel):
    """One chain, dense layout, through get_kernel's host-state form: both scan forms, both orders, both families; (1, 2) and (4, 3) are the pathwise sampler's
    first and only interior step, (2, 257) crosses the 256-element tile, (6, 60) and (30, 24) take the wide path.  The chain starts from the saturated point
    (|x| near 30) where T > 3.  Two sweeps on the same noise, one uniform on each side of the oracle's log alpha."""
    from aux_ssm_samplers_amd.kalman import get_kernel
    ref = LC.reference(family, d, T, 1, order, parallel)
    cell = ref["cell"]
    y, m = cell["model"].yobs, cell["model"].size
    assert (y == 0).any() and np.nanmax(m) >= 1000 and (T <= 3 or (np.isnan(y).sum() == d + 2 and np.abs(cell["x"]).max() > 20))
    init, kernel = get_kernel(*fns(cell["model"]), parallel)
    for k, u in enumerate(ref["us"]):
        out = kernel(None, init(cell["x"][0]), cell["delta"], noise=dict(eps_aux=cell["eps_aux"][0], eps_samp=cell["eps_samp"][0], u_accept=float(u[0])))
        npt.assert_allclose(out.logs[0, 1:], ref["logs"][0, 1:], rtol=1e-9)
        assert abs(out.log_alpha - ref["logs"][0, 0]) <= la_atol(ref["logs"])[0] + 1e-9 * abs(ref["logs"][0, 0])
        assert out.updated == bool(ref["accepted"][k][0])
        npt.assert_allclose(out.x, ref["x_prop"][0] if out.updated else cell["x"][0], rtol=1e-9, atol=1e-10)


@pytest.mark.parametrize("family", LC.FAMILIES)
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("d,T,Cn", LC.CM_SHAPES)
@pytest.mark.parametrize("share", [1, 0])
def test_chain_minor_vs_dense_and_oracle(family, order, d, T, Cn, share):
    """>= 32 chains chain-minor: order 2, and order 1 with sharing off, run the array-free passes (FilterOpFlySV / k_sv_logpdf_cm instantiated for the logistic
    potential, the size read beside the data); order 1 with sharing on runs the chain-shared tables.  Chain-minor == dense on every chain, every seventh chain
    against its own oracle sweep (those chains carry the placed uniforms and hold both outcomes; the others are swept at u = 0.5 and their flags compared
    between the layouts away from the margin)."""
    ref = LC.reference(family, d, T, Cn, order, True, 7)
    cell, u = ref["cell"], ref["us"][0]
    assert ref["accepted"][0].any() and not ref["accepted"][0].all()
    cm = with_share(share, lambda: resident_sweep(cell, u, chain_minor=True))
    dense = with_share(share, lambda: resident_sweep(cell, u, chain_minor=False))
    npt.assert_allclose(cm[0], dense[0], rtol=1e-9, atol=1e-10)
    npt.assert_allclose(cm[2][:, 1:], dense[2][:, 1:], rtol=1e-9)
    assert np.all(np.abs(cm[2][:, 0] - dense[2][:, 0]) <= la_atol(dense[2]) + 1e-9 * np.abs(dense[2][:, 0]))
    clear = np.abs(np.minimum(dense[2][:, 0], 0.0) - np.log(u)) > 1e-3
    npt.assert_array_equal(cm[1][clear], dense[1][clear])
    check_against_oracle(ref, *cm)
    check_against_oracle(ref, *dense)


@pytest.mark.parametrize("family", LC.FAMILIES)
@pytest.mark.parametrize("d,T,Cn", LC.WIDE_SHAPES)
@pytest.mark.parametrize("share", [1, 0])
def test_wide_several_chains_vs_oracle(family, d, T, Cn, share):
    """dx > 4, first order, three chains: with sharing on the chain-shared wide filter is told the observation pattern by the carrier of zeros (the logistic
    first-order pseudo-observations are finite by construction too) and keeps one copy of the filtered covariances; with sharing off every chain runs the general
    wide path."""
    ref = LC.reference(family, d, T, Cn, 1, True)
    assert ref["accepted"][0].any() and not ref["accepted"][0].all()
    check_against_oracle(ref, *with_share(share, lambda: resident_sweep(ref["cell"], ref["us"][0])))


# ---- host states, loop(), jax compatibility ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", LC.FAMILIES)
@pytest.mark.parametrize("order", [1, 2])
def test_host_factory_path_equals_device_sweep(family, order):
    """Hiding the model behind lambdas forces the generic host-factory path (NumPy factories + GPU primitives)."""
    from aux_ssm_samplers_amd.kalman import get_kernel
    ref = LC.reference(family, 2, 257, 1, order, True)
    cell, model = ref["cell"], ref["cell"]["model"]
    init, kdev = get_kernel(*fns(model), True)
    init2, khost = get_kernel(lambda z: model.dynamics_factory(z), lambda z, u, dl: model.observations_factory(z, u, dl), lambda z: model.log_likelihood_fn(z), True)
    noise = dict(eps_aux=cell["eps_aux"][0], eps_samp=cell["eps_samp"][0], u_accept=float(ref["us"][0][0]))
    a = kdev(None, init(cell["x"][0]), cell["delta"], noise=noise)
    b = khost(None, init2(cell["x"][0]), cell["delta"], noise=noise)
    npt.assert_allclose(a.x, b.x, rtol=1e-9, atol=1e-10)
    assert abs(a.log_alpha - b.log_alpha) <= la_atol(ref["logs"])[0] + 1e-9 * abs(b.log_alpha)
    assert a.updated == b.updated


@pytest.mark.parametrize("family", LC.FAMILIES)
@pytest.mark.parametrize("order", [1, 2])
def test_host_states_equal_resident_chains_bit_for_bit(family, order):
    """a host state (T, dx) is one dense resident chain, a host state (C, T, dx) of 40 chains is 40 chain-minor resident chains: state, log terms and flags"""
    from aux_ssm_samplers_amd.kalman import get_kernel
    for d, T, Cn, every in ((4, 150, 1, 1), (1, 300, 40, 7)):
        ref = LC.reference(family, d, T, Cn, order, True, every)
        cell, u = ref["cell"], ref["us"][0]
        init, kernel = get_kernel(*fns(cell["model"]), True)
        x0 = cell["x"][0] if Cn == 1 else cell["x"]
        pick = (lambda a: a[0]) if Cn == 1 else (lambda a: a)
        out = kernel(None, init(x0), cell["delta"], noise=dict(eps_aux=pick(cell["eps_aux"]), eps_samp=pick(cell["eps_samp"]), u_accept=float(u[0]) if Cn == 1 else u))
        x, flags, logs = resident_sweep(cell, u, chain_minor=Cn > 1)
        npt.assert_array_equal(out.x, pick(x))
        npt.assert_array_equal(out.logs, logs)
        npt.assert_array_equal(np.atleast_1d(out.updated), flags)
        assert np.isfinite(logs).all() and np.abs(x - cell["x"]).max() > 1e-3


@pytest.mark.parametrize("family", LC.FAMILIES)
@pytest.mark.parametrize("order", [1, 2])
def test_loop_with_the_step_size_on_the_device(family, order):
    """loop() under common.delta_adaptation keeps the step size on the device (auxssm_kalman_sweep_dd through the keyed sweep).  With an adaptation rate of 0 the
    rule leaves it where it is, so three sweeps of loop() are three kernel calls on the same keys with the host step size -- bit for bit, state and log terms;
    with a rate of 0.5 it adapts: the step size that comes back has moved."""
    from aux_ssm_samplers_amd import _lib, random as R
    from aux_ssm_samplers_amd.common import delta_adaptation
    from aux_ssm_samplers_amd.kalman import get_kernel
    from aux_ssm_samplers_amd.kalman.generic import DeviceChains, KalmanSampler
    from aux_ssm_samplers_amd.loop import loop
    cell = LC.reference(family, 1, 300, 40, order, True, 7)["cell"]
    init, kernel = get_kernel(*fns(cell["model"]), True)
    h = _lib.default_handle()
    key, delta = R.PRNGKey(3 + order), 0.015625
    a = DeviceChains(h, cell["x"])
    assert a.chain_minor
    _, _, state, delta_out, _, _ = loop(key, delta, KalmanSampler(x=a, updated=True), kernel, delta_adaptation, 3, target_alpha=0.5, lr=0.0)
    assert delta_out == delta
    b = DeviceChains(h, cell["x"])
    sb = KalmanSampler(x=b, updated=None)
    n_acc = 0
    for k in R.split(key, 3):
        sb = kernel(k, sb, delta)
        n_acc += int(b.accepted.to_host().sum())
    assert 0 < n_acc
    npt.assert_array_equal(a.to_host(), b.to_host())
    npt.assert_array_equal(a.logs.to_host(), b.logs.to_host())
    npt.assert_array_equal(a.accepted.to_host(), b.accepted.to_host())
    assert np.isfinite(a.logs.to_host()).all() and np.abs(a.to_host() - cell["x"]).max() > 1e-3
    c = DeviceChains(h, cell["x"])
    _, _, _, delta_adapted, _, _ = loop(key, delta, KalmanSampler(x=c, updated=True), kernel, delta_adaptation, 6, target_alpha=0.5, lr=0.5)
    assert np.isfinite(delta_adapted) and delta_adapted > 0 and delta_adapted != delta
    assert np.isfinite(c.logs.to_host()).all() and np.isfinite(c.to_host()).all()


@pytest.mark.parametrize("family", LC.FAMILIES)
def test_jax_compat_sweep_is_the_explicit_sweep_on_the_references_draws(family):
    from aux_ssm_samplers_amd import random as R
    from aux_ssm_samplers_amd.kalman import get_kernel
    cell = LC.reference(family, 4, 150, 1, 2, True)["cell"]
    init, kernel = get_kernel(*fns(cell["model"]), True)
    x = cell["x"][0]
    key = np.array([2024, 11], np.uint32)
    prev = R.set_compat("jax")
    try:
        got = kernel(key, init(x), cell["delta"])
        nz = R.jax_kalman_noise(key[None], cell["T"], cell["d"], np.float64)
    finally:
        R.set_compat(prev)
    want = kernel(None, init(x), cell["delta"], noise=dict(eps_aux=nz["eps_aux"][0], eps_samp=nz["eps_samp"][0], u_accept=float(nz["u_accept"][0])))
    npt.assert_array_equal(got.x, want.x)
    npt.assert_array_equal(got.logs, want.logs)
    assert got.updated == want.updated and np.isfinite(got.logs).all()


# ---- the C entry points ---------------------------------------------------------------------------------------------------------------------------------------
def test_c_entry_points():
    """auxssm_kalman_sweep_keyed runs kinds 13 and 14; a null size slot (or one with another time stride than the data's) is AUXSSM_ERR_ARG with nothing enqueued; auxssm_kalman_sweep_fused goes on refusing
    everything but LG_CONCAT, with its message, and enqueues nothing; kind 9 is refused as unknown kinds are."""
    from aux_ssm_samplers_amd import _lib
    from aux_ssm_samplers_amd.kalman.generic import DeviceChains
    cell = LC.reference("binomial", 2, 129, 33, 1, True, 7)["cell"]
    model, x0 = cell["model"], cell["x"]
    assert model.kmodel == 13
    h = _lib.default_handle()
    dims = _lib.Dims(cell["C"], cell["T"], 1, cell["d"], cell["d"])
    keys = (C.c_uint32 * 6)(1, 2, 3, 4, 5, 6)

    def call(kind, fused, null_size=False):
        ch = DeviceChains(h, x0, chain_minor=True)
        dl, _, yarr = model.device(h, ch.dtype)
        mc = _lib.Lgssm.from_buffer_copy(dl.c)
        if null_size == "stride":
            mc.cs = _lib.Arr(mc.cs.ptr, 0, mc.cs.st + 1, 0)
        elif null_size:
            mc.cs = _lib.Arr(None, 0, 0, 0)
        head = (h.h, _lib.dtype_code(ch.dtype), kind, C.byref(dims), C.byref(mc), C.byref(yarr))
        if fused:
            ch.x_alt, ch.sel = h.zeros(ch.x.shape, ch.dtype), h.zeros((ch.C,), np.int32)
            rc = h.lib.auxssm_kalman_sweep_fused(*head, 0.01, None, keys, 1, _lib.NAN_REFERENCE, ch.layout, ch.x.ptr, ch.x_alt.ptr, ch.sel.ptr, ch.u_acc.ptr,
                                                 ch.accepted.ptr, ch.logs.ptr)
        else:
            rc = h.lib.auxssm_kalman_sweep_keyed(*head, 0.01, None, keys, 1, _lib.NAN_REFERENCE, ch.layout, ch.x.ptr, ch.eps_aux.ptr, ch.eps_samp.ptr, ch.u_acc.ptr,
                                                 ch.accepted.ptr, ch.logs.ptr)
        return rc, ch

    def untouched(ch):
        npt.assert_array_equal(ch.to_host(), x0)
        assert not ch.accepted.to_host().any() and not ch.logs.to_host().any()

    for kind in (_lib.KMODEL_LOGISTIC_FIRST, _lib.KMODEL_LOGISTIC_SECOND):
        rc, ch = call(kind, fused=True)
        assert rc == _lib.ERR_UNSUPPORTED
        assert h.lib.auxssm_last_error().decode() == f"auxssm_kalman_sweep_fused runs AUXSSM_KMODEL_LG_CONCAT (model_kind {kind}: use auxssm_kalman_sweep_keyed)"
        untouched(ch)
        assert not ch.x_alt.to_host().any() and not ch.sel.to_host().any()
        for bad in (True, "stride"):   # no size array; one that is not laid out as the data is
            rc, ch = call(kind, fused=False, null_size=bad)
            assert rc == _lib.ERR_ARG and "size array" in h.lib.auxssm_last_error().decode()
            untouched(ch)
    for fused in (False, True):
        rc, ch = call(9, fused)
        assert rc == (_lib.ERR_UNSUPPORTED if fused else _lib.ERR_ARG)
        assert "model_kind 9" in h.lib.auxssm_last_error().decode()
        untouched(ch)
    # the other pointwise kinds go on ignoring the slot: SV_FIRST on the same arrays runs with and without it
    for null_size in (False, True):
        rc, ch = call(_lib.KMODEL_SV_FIRST, fused=False, null_size=null_size)
        assert rc == 0, h.lib.auxssm_last_error().decode()
    for kind in (_lib.KMODEL_LOGISTIC_FIRST, _lib.KMODEL_LOGISTIC_SECOND):
        rc, ch = call(kind, fused=False)
        assert rc == 0, h.lib.auxssm_last_error().decode()
        logs = ch.logs.to_host()
        assert np.isfinite(logs).all() and logs.any() and np.abs(ch.to_host() - x0).max() > 1e-3


# ---- fp32 ----------------------------------------------------------------------------------------------------------------------------------------------
# The bars are twice the worst error observed on the MI355X over the cases below, rounded up (the smoother's rule): see the test's docstring.
F32_X_BAR = 2e-6     # observed 8.9e-7
F32_LA_BAR = 0.09    # observed 4.3e-2
F32_CELLS = [("dense", 1, 2, 1), ("dense", 4, 3, 1), ("dense", 1, 400, 1), ("dense", 4, 150, 1), ("dense", 30, 24, 1), ("cm", 1, 300, 40), ("cm", 4, 70, 64)]
F32_CASES = [(f,) + c + (order,) for f in LC.FAMILIES for c in F32_CELLS for order in (1, 2)] + [(f, "dense", 30, 24, 3, 1) for f in LC.FAMILIES]


def fp32_errors(family, layout, d, T, Cn, order):
    """-> (ref, max |error| / max |value| of x_prop, max absolute error of log alpha) of a float32 sweep against the float64 oracle on the float32-rounded inputs"""
    ref = LC.reference(family, d, T, Cn, order, True, 7 if layout == "cm" else 1, True)
    cell, idx = ref["cell"], ref["chains"]
    # every chain is made to accept, so that the state that comes back is x_prop
    x, _, logs = resident_sweep(cell, np.zeros(Cn), np.float32, chain_minor=layout == "cm")
    ex = np.abs(x[idx].astype(np.float64) - ref["x_prop"]).max() / np.abs(ref["x_prop"]).max()
    ela = np.abs(logs[idx, 0].astype(np.float64) - ref["logs"][:, 0]).max()
    return ref, float(ex), float(ela)


@pytest.mark.parametrize("family,layout,d,T,Cn,order", F32_CASES)
def test_fp32_against_the_fp64_oracle(family, layout, d, T, Cn, order):
    """The cells above at d in {1, 4, 30} in float32, against the float64 oracle on the float32-rounded inputs (model, sizes, state and noise).  Measured: max
    |error| / max |value| of x_prop and the absolute error of log alpha.  Accept flags are asserted only for chains whose margin exceeds the log alpha bar.
    Observed on the MI355X (worst over the 30 cases): x_prop 8.89e-7 (negative binomial, dense d = 4, T = 3, order 1; the others 2.1e-9 .. 4.3e-7), log alpha
    4.32e-2 (binomial, dense d = 30, T = 24, order 1; the other long cells 8.4e-4 .. 2.1e-2, the two- and three-step cells 2.1e-6 .. 4.9e-4).  The log alpha
    error follows the size of the terms log alpha is the difference of: a chain that starts from |x| = 30 has a prior term of 2e4 to 3e4, whose float32 rounding is
    2e-3 per term, and 4.3e-2 is 1.4e-6 of it; the cells without that start (T <= 3, terms below 300) stay below 5e-4, kalman.PoissonModel's figure.  Bars: twice
    the worst, rounded up -- 2e-6 and 0.09."""
    ref, ex, ela = fp32_errors(family, layout, d, T, Cn, order)
    cell, idx = ref["cell"], ref["chains"]
    print(f"fp32 {family} {layout} d={d} T={T} C={Cn} order={order}: x_prop rel err {ex:.3e}  log alpha abs err {ela:.3e}  (log alpha in [{ref['logs'][:, 0].min():.1f}, "
          f"{ref['logs'][:, 0].max():.1f}], terms up to {np.abs(ref['logs'][:, 1:]).max():.0f})")
    assert ex < F32_X_BAR and ela < F32_LA_BAR
    for k, u in enumerate(ref["us"]):
        _, flags, _ = resident_sweep(cell, u, np.float32, chain_minor=layout == "cm")
        sure = np.abs(np.minimum(ref["logs"][:, 0], 0.0) - np.log(u[idx])) > F32_LA_BAR
        npt.assert_array_equal(flags[idx][sure], ref["accepted"][k][sure])


# ---- ground truth without a restatement ------------------------------------------------------------------------------------------------------------------
def logistic_posterior_by_quadrature(y, m, m0, P0, F, Q, b, n=151, width=7.0):
    """posterior mean / variance / third central moment of each x_t of the scalar logistic model with T = len(y) in (2, 3) by a tensor-product grid centred on the
    prior's stationary path: pi(x) ~ N(x_0; m0, P0) prod_t N(x_t; F x_{t-1} + b, Q) prod_t exp(y_t x_t - m_t softplus(x_t)), a NaN y_t contributing nothing.
    Independent of every sampler and of the oracle; softplus is numpy's logaddexp."""
    T = len(y)
    mean, var = [m0], [P0]
    for _ in range(1, T):
        mean.append(F * mean[-1] + b)
        var.append(F * F * var[-1] + Q)
    grids = [mu + np.linspace(-width * np.sqrt(v), width * np.sqrt(v), n) for mu, v in zip(mean, var)]
    xs = np.meshgrid(*grids, indexing="ij", sparse=True)
    lp = -0.5 * (xs[0] - m0) ** 2 / P0
    for t in range(1, T):
        lp = lp - 0.5 * (xs[t] - F * xs[t - 1] - b) ** 2 / Q
    for xt, yt, mt in zip(xs, y, m):
        if np.isfinite(yt):
            lp = lp + yt * xt - mt * np.logaddexp(0.0, xt)
    w = np.exp(lp - lp.max())
    w /= w.sum()
    out = []
    for ax in range(T):
        mg = w.sum(tuple(a for a in range(T) if a != ax))
        mu = float((mg * grids[ax]).sum())
        out.append((mu, float((mg * (grids[ax] - mu) ** 2).sum()), float((mg * (grids[ax] - mu) ** 3).sum())))
    return np.array(out)


@functools.lru_cache(maxsize=None)
def _exact(y, m, m0, P0, F, Q, b):
    n1, n2 = (101, 201) if len(y) == 3 else (401, 801)
    exact, finer = logistic_posterior_by_quadrature(y, m, m0, P0, F, Q, b, n=n1), logistic_posterior_by_quadrature(y, m, m0, P0, F, Q, b, n=n2)
    npt.assert_allclose(exact, finer, rtol=1e-7, atol=1e-9)   # converged: doubling n moves the moments by 4e-9 at most (the binary cell), 1e-4 of a standard error
    return finer


QUAD_C = 16384
NAN = float("nan")
# a scalar component: (y, size parameter (trials or r), m0, P0, F, Q, b)
QUAD_COMPONENTS = {
    ("binomial", "d1"): [((3.0, 0.0, 7.0), (5.0, 4.0, 7.0), 0.3, 0.2, 0.9, 0.04, 0.1)],
    ("binomial", "d1_missing"): [((3.0, NAN, 1.0), (12.0, NAN, 1.0), 0.3, 0.2, 0.9, 0.04, 0.1)],
    # binary data under a wide prior: three successes out of three single trials say only "the log-odds are not very negative" -- a one-sided, skewed posterior
    ("binomial", "d1_binary"): [((1.0, 1.0, 1.0), (1.0, 1.0, 1.0), 0.0, 4.0, 0.9, 1.0, 0.0)],
    ("binomial", "d2"): [((3.0, 0.0), (5.0, 4.0), 0.3, 0.2, 0.9, 0.04, 0.1), ((1.0, NAN), (1.0, 1.0), -0.5, 0.3, 0.8, 0.09, 0.2)],
    ("negbinomial", "d1"): [((3.0, 0.0, 7.0), (3.0, 3.0, 3.0), 0.3, 0.2, 0.9, 0.04, 0.1)],
    ("negbinomial", "d1_missing"): [((12.0, NAN, 1.0), (0.5, 0.5, 0.5), 0.3, 0.2, 0.9, 0.04, 0.1)],
    ("negbinomial", "d2"): [((3.0, 0.0), (3.0, 3.0), 0.3, 0.2, 0.9, 0.04, 0.1), ((12.0, NAN), (0.5, 0.5), 1.0, 0.3, 0.8, 0.09, 0.2)],
}


def _check(step, read, exact, burn, M):
    """tests/test_gpu_kalman_poisson.py::_check: step(i) = one sweep of all chains, read() -> (C, T d) current states.  The standard error is empirical (the chains
    are independent): means and second moments within 5 standard errors; the standard error of a mean is below 1 % of the posterior sd, so that the band is a
    twentieth of it."""
    s1, s2 = np.zeros((QUAD_C, exact.shape[0])), np.zeros((QUAD_C, exact.shape[0]))
    for i in range(burn + M):
        step(i)
        if i >= burn:
            xs = read()
            s1 += xs
            s2 += xs * xs
    m1, m2 = s1 / M, s2 / M
    mean, se_mean = m1.mean(0), m1.std(0, ddof=1) / np.sqrt(QUAD_C)
    sec, se_sec = m2.mean(0), m2.std(0, ddof=1) / np.sqrt(QUAD_C)
    sd = np.sqrt(exact[:, 1])
    exact_sec = exact[:, 1] + exact[:, 0] ** 2
    print("means z", np.round((mean - exact[:, 0]) / se_mean, 2), "second moments z", np.round((sec - exact_sec) / se_sec, 2), "se / sd", np.round(se_mean / sd, 4))
    assert np.all(se_mean < 0.01 * sd), (se_mean / sd)
    assert np.all(np.abs(mean - exact[:, 0]) < 5 * se_mean), ((mean - exact[:, 0]) / se_mean, se_mean / sd)
    assert np.all(np.abs(sec - exact_sec) < 5 * se_sec), ((sec - exact_sec) / se_sec)


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("family,variant", sorted(QUAD_COMPONENTS))
def test_sampler_targets_the_exact_posterior_by_quadrature(family, variant, order):
    """16 384 resident chains (chain-minor), Threefry noise.  d1*: T = 3, one component; d2: T = 2, two independent scalar models (diagonal F, Q) with different
    parameters, sizes and data in one state -- the D = 2 kernels on a non-Gaussian target, truth = two quadratures.  d1_binary is visibly non-Gaussian: its
    standardised third moment is asserted to exceed 0.25."""
    from aux_ssm_samplers_amd import _lib, random as R
    from aux_ssm_samplers_amd.kalman import get_kernel
    from aux_ssm_samplers_amd.kalman.generic import DeviceChains, KalmanSampler
    comps = QUAD_COMPONENTS[(family, variant)]
    d, T = len(comps), len(comps[0][0])
    size = lambda c: tuple(np.array(c[1]) if family == "binomial" else np.array(c[0]) + np.array(c[1]))
    exact = np.stack([_exact(c[0], size(c), *c[2:]) for c in comps], axis=1).reshape(T * d, 3)     # rows (t, k), as the state (T, d) flattens
    if variant == "d1_binary":
        skew = exact[:, 2] / exact[:, 1] ** 1.5
        assert np.all(np.abs(skew) > 0.25), skew
    y = np.array([c[0] for c in comps]).T
    par = np.array([c[1] for c in comps]).T
    m0, P0, F, Q, b = (np.array([c[i] for c in comps]) for i in range(2, 7))
    model = LC.make_model(family, y, par, m0, np.diag(P0), np.diag(F), np.diag(Q), b, order)
    init, kernel = get_kernel(*fns(model), True)
    rng = np.random.default_rng(1)
    chains = DeviceChains(_lib.default_handle(), exact[:, 0].reshape(1, T, d) + np.sqrt(exact[:, 1]).reshape(1, T, d) * rng.standard_normal((QUAD_C, T, d)))
    assert chains.chain_minor
    state = KalmanSampler(x=chains, updated=None)
    # the step size, from the model alone: of the order of the posterior variance (the proposal then moves a chain by about a posterior sd); first order needs
    # delta / 2 * lam < 1, lam <= max(size) / 4
    delta = 2.0 if variant == "d1_binary" else 0.5
    burn, M = 40, 160
    keys = R.split(R.PRNGKey(41 + order), burn + M)
    acc = []
    _check(lambda i: (kernel(keys[i], state, delta), acc.append(chains.accepted.to_host().mean()) if i % 40 == 0 else None),
           lambda: chains.to_host().reshape(QUAD_C, T * d), exact[:, :2], burn, M)
    assert 0.2 < np.mean(acc) <= 1.0, np.mean(acc)


# ---- ground truth: sequential particle Gibbs on the same density, stated as a user program -----------------------------------------------------------------------
# y row of the program: [y_1 .. y_D | m_1 .. m_D] (p = 2 D); a NaN y_k drops its component, whatever m_k is.  No cSMC potential kind is added for this density.
LOGISTIC_PROGRAM = r"""
template <typename R, int D> __device__ R log_g(int t, const R* x, const R* xprev, const R* y, const R* theta) {
    R acc = 0;
    for (int k = 0; k < D; ++k) {
        const R xk = x[k], e = exp(-fabs(xk));
        const R v = y[k] * xk - y[D + k] * ((xk > (R)0 ? xk : (R)0) + log1p(e));
        acc += (y[k] - y[k] == 0) ? v : (R)0;
    }
    return acc;
}
"""
PG_T, PG_D, PG_C = 12, 2, 1024


@functools.lru_cache(maxsize=None)
def _pg_model(family):
    """d = 2, T = 12: AR(1) log-odds per component (F = 0.9, Q = 0.3, P0 = 0.5), binomial trials 1 .. 12 with a binary component, or r = 3 / 0.5; one missing entry.
    -> (y, par, size, (m0, P0, F, Q, b), delta): delta = 2 / lam with lam the largest curvature of the negative log-target, at most
    1 / P0 + 1 / Q + F^2 / Q + max(size) / 4 (tests/test_gpu_poisson.py's rule)."""
    rng = np.random.default_rng(77)
    T, d = PG_T, PG_D
    F, Q, P0 = 0.9, 0.3, 0.5
    x = np.zeros((T, d))
    x[0] = np.sqrt(P0) * rng.standard_normal(d)
    for t in range(1, T):
        x[t] = F * x[t - 1] + np.sqrt(Q) * rng.standard_normal(d)
    if family == "binomial":
        par = rng.integers(1, 13, size=(T, d)).astype(np.float64)
        par[:, 0] = 1.0
        y = rng.binomial(par.astype(np.int64), 1.0 / (1.0 + np.exp(-x))).astype(np.float64)
        size = par.copy()
    else:
        par = np.tile(np.array([0.5, 3.0]), (T, 1))
        y = rng.poisson(rng.gamma(par, np.exp(x))).astype(np.float64)
        size = y + par
    y[5, 1] = np.nan
    lam = 1.0 / P0 + 1.0 / Q + F * F / Q + float(np.nanmax(size)) / 4.0
    return y, par, size, (np.zeros(d), P0 * np.eye(d), F * np.eye(d), Q * np.eye(d), np.zeros(d)), 2.0 / lam


@functools.lru_cache(maxsize=None)
def _pg_particle_gibbs(family):
    """posterior means and their standard errors (T, d) from sequential particle Gibbs (auxiliary cSMC, independent proposals, backward sampling) on the user program"""
    from aux_ssm_samplers_amd.csmc import DevicePotential, GaussianInit, LinearGaussianDynamics, get_independent_kernel
    from tests.potential_gpu import gibbs_moments
    y, par, size, (m0, P0, F, Q, b), delta = _pg_model(family)
    rows = np.concatenate([y, np.nan_to_num(size)], axis=1)
    M0, Mt = GaussianInit(m0=m0, P0=P0), LinearGaussianDynamics(F=F, b=b, Q=Q)
    G0, Gt = DevicePotential(LOGISTIC_PROGRAM, y=rows[0], p=2 * PG_D), DevicePotential(LOGISTIC_PROGRAM, params=rows[1:], p=2 * PG_D)
    kernel = get_independent_kernel(M0, G0, Mt, Gt, 32, backward=True, Pt=Mt)[1]
    m1, se1, _, _ = gibbs_moments(kernel, PG_T, PG_D, delta, 7000, Cn=PG_C, burn=200, iters=240)
    return m1, se1


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("family", LC.FAMILIES)
def test_posterior_means_agree_with_sequential_particle_gibbs(family, order):
    """1024 resident chains each: the Kalman sampler's posterior means at d = 2, T = 12 within 5 combined standard errors of particle Gibbs's on the same density"""
    from aux_ssm_samplers_amd import _lib, random as R
    from aux_ssm_samplers_amd.kalman import get_kernel
    from aux_ssm_samplers_amd.kalman.generic import DeviceChains, KalmanSampler
    y, par, size, (m0, P0, F, Q, b), delta = _pg_model(family)
    pg_mean, pg_se = _pg_particle_gibbs(family)
    model = LC.make_model(family, y, par, m0, P0, F, Q, b, order)
    init, kernel = get_kernel(*fns(model), True)
    chains = DeviceChains(_lib.default_handle(), np.zeros((PG_C, PG_T, PG_D)))
    state = KalmanSampler(x=chains, updated=None)
    burn, M = 200, 240
    keys = R.split(R.PRNGKey(90 + order), burn + M)
    s1 = np.zeros((PG_C, PG_T, PG_D))
    for i in range(burn + M):
        kernel(keys[i], state, delta)
        if i >= burn:
            s1 += chains.to_host()
    m1 = s1 / M
    mean, se = m1.mean(0), m1.std(0, ddof=1) / np.sqrt(PG_C)
    z = (mean - pg_mean) / np.sqrt(se ** 2 + pg_se ** 2)
    print(f"{family} order {order}: delta = {delta:.3f}; worst z {np.abs(z).max():.2f}; se Kalman {se.max():.4f}, se particle Gibbs {pg_se.max():.4f}; "
          f"means in [{pg_mean.min():.2f}, {pg_mean.max():.2f}]")
    assert np.all(np.isfinite(z)) and np.abs(z).max() < 5
    # power: the two samplers would be told apart if one of them targeted the prior (its mean is 0 everywhere)
    assert np.abs(pg_mean / np.sqrt(se ** 2 + pg_se ** 2)).max() > 10
