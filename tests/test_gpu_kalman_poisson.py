"""kalman.PoissonModel on the device (AUXSSM_KMODEL_POISSON_FIRST / _SECOND: the SV sweep's kernels instantiated for the Poisson potential) against the oracle's
sweep (oracle.kalman_np.kalman_sweep) driven by the model's own NumPy factories, on identical explicit noise and in fp64, at the tolerances of
tests/test_gpu_nonlinear_kalman.py: x at rtol 1e-9 / atol 1e-10, the four log terms at rtol 1e-9, log alpha at rtol 1e-6 / atol 1e-7.  The cells, their
missing counts and the placed acceptance uniforms are tests/kalman_poisson_cases.py's: every chain the oracle ran has a margin |log alpha - log u| >= 0.05, so an
accept flag that differs is a defect.  Then: the layouts against each other, the host-factory path, loop() with the step size on the device, the C entry points,
fp32 against the fp64 oracle (bars from measured errors), and the sampler against the exact posterior by quadrature."""
import ctypes as C
import functools

import numpy as np
import numpy.testing as npt
import pytest

from tests import kalman_poisson_cases as PC

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


def check_against_oracle(ref, x, flags, logs, u_index=0):
    """the oracle's chains of one resident sweep"""
    cell, idx = ref["cell"], ref["chains"]
    npt.assert_allclose(logs[idx, 1:], ref["logs"][:, 1:], rtol=1e-9)
    npt.assert_allclose(logs[idx, 0], ref["logs"][:, 0], rtol=1e-6, atol=1e-7)
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


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("d,T", PC.DENSE_SHAPES)
@pytest.mark.parametrize("parallel", [True, False])
def test_dense_one_chain_vs_oracle(order, d, T, parallel):
    """One chain, dense layout, through get_kernel's host-state form: both scan forms, both orders; (1, 2) and (4, 3) are the pathwise sampler's first and only
    interior step, (2, 257) crosses the 256-element tile, (6, 60) and (30, 24) take the wide path.  Two sweeps on the same noise, one uniform on each side of the
    oracle's log alpha."""
    from aux_ssm_samplers_amd.kalman import get_kernel
    ref = PC.reference(d, T, 1, order, parallel)
    cell = ref["cell"]
    y = cell["model"].yobs
    assert (y == 0).any() and np.nanmax(y) > 100 and (T <= 3 or np.isnan(y).sum() == d + 2)
    init, kernel = get_kernel(*fns(cell["model"]), parallel)
    for k, u in enumerate(ref["us"]):
        out = kernel(None, init(cell["x"][0]), cell["delta"], noise=dict(eps_aux=cell["eps_aux"][0], eps_samp=cell["eps_samp"][0], u_accept=float(u[0])))
        npt.assert_allclose(out.logs[0, 1:], ref["logs"][0, 1:], rtol=1e-9)
        npt.assert_allclose(out.log_alpha, ref["logs"][0, 0], rtol=1e-6, atol=1e-7)
        assert out.updated == bool(ref["accepted"][k][0])
        npt.assert_allclose(out.x, ref["x_prop"][0] if out.updated else cell["x"][0], rtol=1e-9, atol=1e-10)


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("d,T,Cn", PC.CM_SHAPES)
@pytest.mark.parametrize("share", [1, 0])
def test_chain_minor_vs_dense_and_oracle(order, d, T, Cn, share):
    """>= 32 chains chain-minor: order 2, and order 1 with sharing off, run the array-free passes (FilterOpFlySV / k_sv_logpdf_cm instantiated for the Poisson
    potential); order 1 with sharing on runs the chain-shared tables.  Chain-minor == dense on every chain, every seventh chain against its own oracle sweep (those
    chains carry the placed uniforms and hold both outcomes; the others are swept at u = 0.5 and their flags compared between the layouts away from the margin)."""
    ref = PC.reference(d, T, Cn, order, True, 7)
    cell, u = ref["cell"], ref["us"][0]
    assert ref["accepted"][0].any() and not ref["accepted"][0].all()
    cm = with_share(share, lambda: resident_sweep(cell, u, chain_minor=True))
    dense = with_share(share, lambda: resident_sweep(cell, u, chain_minor=False))
    npt.assert_allclose(cm[0], dense[0], rtol=1e-9, atol=1e-10)
    npt.assert_allclose(cm[2][:, 1:], dense[2][:, 1:], rtol=1e-9)
    npt.assert_allclose(cm[2][:, 0], dense[2][:, 0], rtol=1e-6, atol=1e-7)
    clear = np.abs(np.minimum(dense[2][:, 0], 0.0) - np.log(u)) > 1e-3
    npt.assert_array_equal(cm[1][clear], dense[1][clear])
    check_against_oracle(ref, *cm)
    check_against_oracle(ref, *dense)


@pytest.mark.parametrize("d,T,Cn", PC.WIDE_SHAPES)
@pytest.mark.parametrize("share", [1, 0])
def test_wide_several_chains_vs_oracle(d, T, Cn, share):
    """dx > 4, first order, three chains: with sharing on the chain-shared wide filter is told the observation pattern by the carrier of zeros (Poisson's first-order
    pseudo-observations are finite by construction too) and keeps one copy of the filtered covariances; with sharing off every chain runs the general wide path."""
    ref = PC.reference(d, T, Cn, 1, True)
    assert ref["accepted"][0].any() and not ref["accepted"][0].all()
    check_against_oracle(ref, *with_share(share, lambda: resident_sweep(ref["cell"], ref["us"][0])))


@pytest.mark.parametrize("order", [1, 2])
def test_host_factory_path_equals_device_sweep(order):
    """Hiding the model behind lambdas forces the generic host-factory path (NumPy factories + GPU primitives)."""
    from aux_ssm_samplers_amd.kalman import get_kernel
    ref = PC.reference(2, 257, 1, order, True)
    cell, model = ref["cell"], ref["cell"]["model"]
    init, kdev = get_kernel(*fns(model), True)
    init2, khost = get_kernel(lambda z: model.dynamics_factory(z), lambda z, u, dl: model.observations_factory(z, u, dl), lambda z: model.log_likelihood_fn(z), True)
    noise = dict(eps_aux=cell["eps_aux"][0], eps_samp=cell["eps_samp"][0], u_accept=float(ref["us"][0][0]))
    a = kdev(None, init(cell["x"][0]), cell["delta"], noise=noise)
    b = khost(None, init2(cell["x"][0]), cell["delta"], noise=noise)
    npt.assert_allclose(a.x, b.x, rtol=1e-9, atol=1e-10)
    npt.assert_allclose(a.log_alpha, b.log_alpha, rtol=1e-6, atol=1e-7)
    assert a.updated == b.updated


@pytest.mark.parametrize("order", [1, 2])
def test_loop_with_the_step_size_on_the_device_equals_three_kernel_calls(order):
    """loop() under common.delta_adaptation keeps the step size on the device (auxssm_kalman_sweep_dd through the keyed sweep); with an adaptation rate of 0 the rule
    leaves it where it is, so three sweeps of loop() are three kernel calls on the same keys with the host step size -- bit for bit, state and log terms."""
    from aux_ssm_samplers_amd import _lib, random as R
    from aux_ssm_samplers_amd.common import delta_adaptation
    from aux_ssm_samplers_amd.kalman import get_kernel
    from aux_ssm_samplers_amd.kalman.generic import DeviceChains, KalmanSampler
    from aux_ssm_samplers_amd.loop import loop
    cell = PC.reference(1, 300, 40, order, True, 7)["cell"]
    init, kernel = get_kernel(*fns(cell["model"]), True)
    h = _lib.default_handle()
    key, delta = R.PRNGKey(3 + order), 0.0625
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


def test_jax_compat_sweep_is_the_explicit_sweep_on_the_references_draws():
    from aux_ssm_samplers_amd import random as R
    from aux_ssm_samplers_amd.kalman import get_kernel
    cell = PC.reference(4, 150, 1, 2, True)["cell"]
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


def test_c_entry_points():
    """auxssm_kalman_sweep_keyed runs kind 7; auxssm_kalman_sweep_fused goes on refusing everything but LG_CONCAT, with its message, and enqueues nothing; kind 9 is
    refused as unknown kinds are."""
    from aux_ssm_samplers_amd import _lib
    from aux_ssm_samplers_amd.kalman.generic import DeviceChains
    cell = PC.reference(2, 129, 33, 1, True, 7)["cell"]
    model, x0 = cell["model"], cell["x"]
    assert model.kmodel == 7
    h = _lib.default_handle()
    dims = _lib.Dims(cell["C"], cell["T"], 1, cell["d"], cell["d"])
    keys = (C.c_uint32 * 6)(1, 2, 3, 4, 5, 6)

    def call(kind, fused):
        ch = DeviceChains(h, x0, chain_minor=True)
        dl, _, yarr = model.device(h, ch.dtype)
        head = (h.h, _lib.dtype_code(ch.dtype), kind, C.byref(dims), C.byref(dl.c), C.byref(yarr))
        if fused:
            ch.x_alt, ch.sel = h.zeros(ch.x.shape, ch.dtype), h.zeros((ch.C,), np.int32)
            rc = h.lib.auxssm_kalman_sweep_fused(*head, 0.05, None, keys, 1, _lib.NAN_REFERENCE, ch.layout, ch.x.ptr, ch.x_alt.ptr, ch.sel.ptr, ch.u_acc.ptr,
                                                 ch.accepted.ptr, ch.logs.ptr)
        else:
            rc = h.lib.auxssm_kalman_sweep_keyed(*head, 0.05, None, keys, 1, _lib.NAN_REFERENCE, ch.layout, ch.x.ptr, ch.eps_aux.ptr, ch.eps_samp.ptr, ch.u_acc.ptr,
                                                 ch.accepted.ptr, ch.logs.ptr)
        return rc, ch

    def untouched(ch):
        npt.assert_array_equal(ch.to_host(), x0)
        assert not ch.accepted.to_host().any() and not ch.logs.to_host().any()

    rc, ch = call(_lib.KMODEL_POISSON_FIRST, fused=True)
    assert rc == _lib.ERR_UNSUPPORTED
    assert h.lib.auxssm_last_error().decode() == "auxssm_kalman_sweep_fused runs AUXSSM_KMODEL_LG_CONCAT (model_kind 7: use auxssm_kalman_sweep_keyed)"
    untouched(ch)
    assert not ch.x_alt.to_host().any() and not ch.sel.to_host().any()
    for fused in (False, True):
        rc, ch = call(9, fused)
        assert rc == (_lib.ERR_UNSUPPORTED if fused else _lib.ERR_ARG)
        assert "model_kind 9" in h.lib.auxssm_last_error().decode()
        untouched(ch)
    for kind in (_lib.KMODEL_POISSON_FIRST, _lib.KMODEL_POISSON_SECOND):
        rc, ch = call(kind, fused=False)
        assert rc == 0, h.lib.auxssm_last_error().decode()
        logs = ch.logs.to_host()
        assert np.isfinite(logs).all() and logs.any() and np.abs(ch.to_host() - x0).max() > 1e-3


# ---- fp32 ----------------------------------------------------------------------------------------------------------------------------------------------
# The bars are twice the worst error observed on the MI355X over the cases below, rounded up (the smoother's rule): see the test's docstring.
F32_X_BAR = 6e-7     # observed 2.6e-7
F32_LA_BAR = 1e-3    # observed 5.0e-4
F32_CELLS = [("dense", 1, 2, 1), ("dense", 4, 3, 1), ("dense", 1, 400, 1), ("dense", 4, 150, 1), ("dense", 30, 24, 1), ("cm", 1, 300, 40), ("cm", 4, 70, 64)]
F32_CASES = [c + (order,) for c in F32_CELLS for order in (1, 2)] + [("dense", 30, 24, 3, 1)]   # (the wide several-chain cell is first order)


@pytest.mark.parametrize("layout,d,T,Cn,order", F32_CASES)
def test_fp32_against_the_fp64_oracle(layout, d, T, Cn, order):
    """The cells above at d in {1, 4, 30} in float32, against the float64 oracle on the float32-rounded inputs (model, state and noise).  Measured: max |error| /
    max |value| of x_prop and the absolute error of log alpha.  Accept flags are asserted only for chains whose margin exceeds the log alpha bar.
    Observed on the MI355X (worst over the 15 cases): x_prop 2.58e-7 (dense d = 4, T = 3, order 2; the others 2.8e-8 .. 2.6e-7), log alpha 5.00e-4 (dense d = 30,
    T = 24, order 2; the others 1.1e-5 .. 3.0e-4, with |log alpha| up to 78).  Bars: twice that, rounded up -- 6e-7 and 1e-3."""
    ref = PC.reference(d, T, Cn, order, True, 7 if layout == "cm" else 1, True)
    cell, idx = ref["cell"], ref["chains"]
    # every chain is made to accept, so that the state that comes back is x_prop
    x, _, logs = resident_sweep(cell, np.zeros(Cn), np.float32, chain_minor=layout == "cm")
    ex = np.abs(x[idx].astype(np.float64) - ref["x_prop"]).max() / np.abs(ref["x_prop"]).max()
    ela = np.abs(logs[idx, 0].astype(np.float64) - ref["logs"][:, 0]).max()
    print(f"fp32 {layout} d={d} T={T} C={Cn} order={order}: x_prop rel err {ex:.3e}  log alpha abs err {ela:.3e}  (log alpha in [{ref['logs'][:, 0].min():.1f}, "
          f"{ref['logs'][:, 0].max():.1f}])")
    assert ex < F32_X_BAR and ela < F32_LA_BAR
    for k, u in enumerate(ref["us"]):
        _, flags, _ = resident_sweep(cell, u, np.float32, chain_minor=layout == "cm")
        sure = np.abs(np.minimum(ref["logs"][:, 0], 0.0) - np.log(u[idx])) > F32_LA_BAR
        npt.assert_array_equal(flags[idx][sure], ref["accepted"][k][sure])


# ---- ground truth without a restatement ------------------------------------------------------------------------------------------------------------------
def poisson_posterior_by_quadrature(y, m0, P0, F, Q, b, n=151, width=7.0):
    """posterior mean / variance of each x_t of the scalar Poisson model with T = 3 by a tensor-product grid over (x_0, x_1, x_2) (tests/helpers.py::
    sv_posterior_by_quadrature's grid, centred on m0): pi(x) ~ N(x_0; m0, P0) prod_t N(x_t; F x_{t-1} + b, Q) prod_t exp(y_t x_t - e^{x_t}), a NaN y_t
    contributing nothing.  Independent of every sampler and of the oracle."""
    s0 = np.sqrt(P0)
    g = m0 + np.linspace(-width * s0, width * s0, n)
    x0, x1, x2 = np.meshgrid(g, g, g, indexing="ij", sparse=True)
    lp = -0.5 * (x0 - m0) ** 2 / P0 - 0.5 * (x1 - F * x0 - b) ** 2 / Q - 0.5 * (x2 - F * x1 - b) ** 2 / Q
    for xt, yt in ((x0, y[0]), (x1, y[1]), (x2, y[2])):
        if np.isfinite(yt):
            lp = lp + yt * xt - np.exp(xt)
    w = np.exp(lp - lp.max())
    w /= w.sum()
    out = []
    for ax in range(3):
        m = w.sum(tuple(a for a in range(3) if a != ax))
        mean = float((m * g).sum())
        out.append((mean, float((m * (g - mean) ** 2).sum())))
    return np.array(out)


@functools.lru_cache(maxsize=None)
def _exact(y, m0, P0, F, Q, b):
    exact, finer = poisson_posterior_by_quadrature(y, m0, P0, F, Q, b, n=101), poisson_posterior_by_quadrature(y, m0, P0, F, Q, b, n=201)
    npt.assert_allclose(exact, finer, rtol=1e-12, atol=1e-13)   # converged: doubling n moves nothing (measured: 6e-15)
    return finer


QUAD_C = 16384


def _check(step, read, exact, burn, M):
    """tests/test_gpu_posterior_precision.py::_check for a state of any width: step(i) = one sweep of all chains, read() -> (C, T d) current states.  The standard
    error is empirical (the chains are independent): means and second moments within 5 standard errors, the standard error below 0.4 % of the posterior sd."""
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
    assert np.all(se_mean < 0.004 * sd), (se_mean / sd)
    assert np.all(np.abs(mean - exact[:, 0]) < 5 * se_mean), ((mean - exact[:, 0]) / se_mean, se_mean / sd)
    assert np.all(np.abs(sec - exact_sec) < 5 * se_sec), ((sec - exact_sec) / se_sec)


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("variant", ["d1", "d1_missing", "d2"])
def test_sampler_targets_the_exact_posterior_by_quadrature(variant, order):
    """T = 3, 16 384 resident chains (chain-minor), Threefry noise.  d1: counts (3, 0, 7); d1_missing: the count at t = 1 missing; d2: two independent scalar
    models (diagonal F, Q) with different parameters and data in one state -- the D = 2 kernels on a non-Gaussian target, truth = two quadratures."""
    from aux_ssm_samplers_amd import _lib, random as R
    from aux_ssm_samplers_amd.kalman import get_kernel, PoissonModel
    from aux_ssm_samplers_amd.kalman.generic import DeviceChains, KalmanSampler
    T = 3
    comps = {"d1": [((3.0, 0.0, 7.0), 1.0, 0.2, 0.9, 0.04, 0.1)],
             "d1_missing": [((3.0, np.nan, 7.0), 1.0, 0.2, 0.9, 0.04, 0.1)],
             "d2": [((3.0, 0.0, 7.0), 1.0, 0.2, 0.9, 0.04, 0.1), ((12.0, 5.0, np.nan), 2.0, 0.3, 0.8, 0.09, 0.4)]}[variant]
    d = len(comps)
    exact = np.stack([_exact(*c) for c in comps], axis=1).reshape(T * d, 2)     # rows (t, k), as the state (T, d) flattens
    y = np.array([c[0] for c in comps]).T
    m0, P0, F, Q, b = (np.array([c[i] for c in comps]) for i in range(1, 6))
    model = PoissonModel(y, m0, np.diag(P0), np.diag(F), np.diag(Q), b, order=order)
    init, kernel = get_kernel(*fns(model), True)
    rng = np.random.default_rng(1)
    chains = DeviceChains(_lib.default_handle(), exact[:, 0].reshape(1, T, d) + 0.3 * rng.standard_normal((QUAD_C, T, d)))
    assert chains.chain_minor
    state = KalmanSampler(x=chains, updated=None)
    burn, M, delta = 40, 160, 0.5
    keys = R.split(R.PRNGKey(41 + order), burn + M)
    acc = []
    _check(lambda i: (kernel(keys[i], state, delta), acc.append(chains.accepted.to_host().mean()) if i % 40 == 0 else None),
           lambda: chains.to_host().reshape(QUAD_C, T * d), exact, burn, M)
    assert 0.2 < np.mean(acc) <= 1.0, np.mean(acc)
