"""kalman.MVTModel on the device (csrc/kalman_mvt.hip: model kinds MVT_FIRST / MVT_SECOND) against oracle.kalman_np.kalman_sweep driven by the model's own NumPy
factories, on the cells of tests/kalman_mvt_cases.py (their oracle results are computed once and shared).  fp64 bars are those of tests/test_gpu_nonlinear_kalman.py
for the SV kinds: x' and the state 1e-9 / 1e-10, the four log terms 1e-9 relative, log alpha 1e-7, flags equal, a rejected chain's state bit-identical.

fp32, measured on one MI355X over the case list (first three chains of a cell through the host-factory path; fewer chains can only lower b):
    b = max |log alpha(fp32 host-factory path) - log alpha(fp64 oracle)| = 1.84e-3; the device sweep is held to 4 b = 7.4e-3 and measures at most 2.0e-4."""
import ctypes as C
import functools

import numpy as np
import numpy.testing as npt
import pytest

from aux_ssm_samplers_amd import _lib, random as R
from aux_ssm_samplers_amd.kalman import MVTModel, get_kernel
from aux_ssm_samplers_amd.kalman.generic import DeviceChains, KalmanSampler
from tests import kalman_mvt_cases as CS

pytestmark = pytest.mark.gpu
NCELL = len(CS.CELLS)


def fns(model, lambdas=False):
    if lambdas:   # the same methods, not recognisable: the host-factory path
        return (lambda x: model.dynamics_factory(x), lambda x, u, d: model.observations_factory(x, u, d), lambda x: model.log_likelihood_fn(x))
    return model.dynamics_factory, model.observations_factory, model.log_likelihood_fn


def host_state(c, dtype):
    """the cell's state and noise in one of the accepted host shapes: one chain (T, d, 1); three chains (C, T, d, 1); seventy (C, T, d)"""
    x, ea, es = (c[k].astype(dtype) for k in ("x", "eps_aux", "eps_samp"))
    if c["C"] == 1:
        return x[0][..., None], ea[0][..., None], es[0][..., None]
    if c["C"] == 3:
        return x[..., None], ea[..., None], es[..., None]
    return x, ea, es


def device_sweep(c, u, dtype=np.float64, parallel=None):
    """one device sweep of the whole cell -> (x (C, T, d), flags (C,), logs (C, 5))"""
    init, kernel = get_kernel(*fns(c["model"]), c["parallel"] if parallel is None else parallel)
    x, ea, es = host_state(c, dtype)
    out = kernel(None, init(x), c["delta"], noise=dict(eps_aux=ea, eps_samp=es, u_accept=float(u[0]) if c["C"] == 1 else u))
    assert out.x.shape == x.shape and out.x.dtype == dtype
    shape = (c["C"], c["T"], c["d"])
    return out.x.reshape(shape), np.atleast_1d(out.updated), out.logs.reshape(c["C"], 5)


def host_path_sweep(c, k, u, dtype=np.float64):
    """chain k through the host-factory path (the methods behind lambdas) -> (x (T, d), flag, log alpha)"""
    init, kernel = get_kernel(*fns(c["model"], lambdas=True), c["parallel"])
    e = lambda a: a[k].astype(dtype)[..., None]
    out = kernel(None, init(e(c["x"])), c["delta"], noise=dict(eps_aux=e(c["eps_aux"]), eps_samp=e(c["eps_samp"]), u_accept=float(u[k])))
    return out.x[..., 0], bool(out.updated), out.log_alpha


def check_against_oracle(c, ref, u, acc, got):
    x, flags, logs = got
    npt.assert_array_equal(flags, acc)
    want = np.where(acc[:, None, None], ref["x_prop"], c["x"])
    npt.assert_allclose(x, want, rtol=1e-9, atol=1e-10)
    npt.assert_array_equal(x[~acc], c["x"][~acc])                 # a rejected chain's state is untouched
    npt.assert_allclose(logs[:, 1:], ref["logs"][:, 1:], rtol=1e-9)
    npt.assert_allclose(logs[:, 0], ref["logs"][:, 0], rtol=1e-7, atol=1e-7)


@pytest.mark.parametrize("i", range(NCELL), ids=CS.IDS)
def test_fp64_sweep_against_the_oracle(i):
    c, ref = CS.build(i), CS.reference(i)
    for u, acc in zip(ref["us"], ref["accepted"]):
        got = device_sweep(c, u)
        check_against_oracle(c, ref, u, acc, got)
    other = device_sweep(c, u, parallel=not c["parallel"])        # `parallel` is accepted and changes no bit
    for a, b in zip(got, other):
        npt.assert_array_equal(a, b)


@pytest.mark.parametrize("i", range(NCELL), ids=CS.IDS)
def test_device_path_is_the_host_factory_path(i):
    c, ref = CS.build(i), CS.reference(i)
    u = ref["us"][-1]
    x, flags, logs = device_sweep(c, u)
    for k in range(min(c["C"], 3)):
        hx, hflag, hla = host_path_sweep(c, k, u)
        assert hflag == flags[k]
        npt.assert_allclose(x[k], hx, rtol=1e-9, atol=1e-10)
        npt.assert_allclose(logs[k, 0], hla, rtol=1e-7, atol=1e-7)


@functools.lru_cache(maxsize=None)
def fp32_host_bound():
    """b: the fp32 host-factory path (code of before this model existed) against the fp64 oracle, over the case list"""
    b = 0.0
    for i in range(NCELL):
        c, ref = CS.build(i), CS.reference(i)
        for k in range(min(c["C"], 3)):
            b = max(b, abs(host_path_sweep(c, k, ref["us"][0], np.float32)[2] - ref["logs"][k, 0]))
    print(f"fp32 host-factory path: b = max |log alpha - oracle| = {b:.3e}")
    return b


@pytest.mark.parametrize("i", range(NCELL), ids=CS.IDS)
def test_fp32_sweep_stays_within_four_times_the_host_paths_error(i):
    b = fp32_host_bound()
    c, ref = CS.build(i), CS.reference(i)
    for u, acc in zip(ref["us"], ref["accepted"]):
        x, flags, logs = device_sweep(c, u, np.float32)
        err = np.max(np.abs(logs[:, 0] - ref["logs"][:, 0]))
        print(f"{CS.IDS[i]}: fp32 device max |log alpha - oracle| = {err:.3e}  (b = {b:.3e})")
        assert err <= 4 * b
        npt.assert_array_equal(flags, acc)                        # every chain: the cells keep |log alpha - log u| >= 0.05
        npt.assert_array_equal(x[~acc], c["x"].astype(np.float32)[~acc])


def test_fp32_filter_at_delta_1e_5_keeps_one_minus_the_gain():
    """d = 64, T = 70 at the example's starting step size: R = delta / 2 = 5e-6 beside P ~ 1, so P / S rounds to 1 in fp32 and a filter that formed 1 - K as
    1 - P / S would carry zero variances (the proposal would collapse onto the filtered means).  x' against the fp64 device sweep at 1e-3 absolute."""
    from aux_ssm_samplers_amd.workloads import spatial_kalman_setup
    model, x0 = spatial_kalman_setup(70, 8, seed=2)
    rng = np.random.default_rng(5)
    noise = dict(eps_aux=rng.standard_normal(x0.shape), eps_samp=rng.standard_normal(x0.shape), u_accept=0.0)   # u = 0: accepted unless alpha is 0 or NaN
    out = {}
    for dt in (np.float64, np.float32):
        init, kernel = get_kernel(*fns(model), True)
        o = kernel(None, init(x0.astype(dt)), 1e-5, noise={k: np.asarray(v, dt) for k, v in noise.items()})
        assert o.updated and np.isfinite(o.logs).all()
        out[dt] = o.x
    assert np.abs(out[np.float64] - x0).max() > 1e-3              # the proposal moved: nothing collapsed
    npt.assert_allclose(out[np.float32], out[np.float64], rtol=0, atol=1e-3)


def resident_pair(c, dtype):
    h = _lib.default_handle()
    x = c["x"].astype(dtype)
    return h, DeviceChains(h, x, chain_minor=False), DeviceChains(h, x, chain_minor=False)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("i", [3, 5, 11, 12], ids=lambda i: CS.IDS[i])
def test_keyed_sweep_is_the_explicit_sweep_on_the_drawn_arrays(i, dtype):
    c = CS.build(i)
    h, a, b = resident_pair(c, dtype)
    init, kernel = get_kernel(*fns(c["model"]), True)
    key = R.PRNGKey(40 + i)
    kernel(key, KalmanSampler(x=a, updated=None), c["delta"])
    h.kalman_draw(*R.split(key, 3), b.eps_aux, b.eps_samp, b.u_acc)
    noise = dict(eps_aux=b.eps_aux.to_host(), eps_samp=b.eps_samp.to_host(), u_accept=b.u_acc.to_host())
    kernel(None, KalmanSampler(x=b, updated=None), c["delta"], noise=noise)
    npt.assert_array_equal(a.to_host(), b.to_host())
    npt.assert_array_equal(a.accepted.to_host(), b.accepted.to_host())
    npt.assert_array_equal(a.logs.to_host(), b.logs.to_host())
    assert np.isfinite(a.logs.to_host()).all()
    if dtype == np.float32:   # (a float32 device scalar is not the host's double step size)
        return
    # and the device-resident step size (what loop() hands over while it adapts) is the host one, bit for bit
    h2, d1, _ = resident_pair(c, dtype)
    kernel(None, KalmanSampler(x=d1, updated=None), h.to_device(np.full(1, c["delta"], dtype), dtype), noise=noise)
    npt.assert_array_equal(d1.to_host(), b.to_host())
    npt.assert_array_equal(d1.logs.to_host(), b.logs.to_host())


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("i", [5, 8, 11, 22], ids=lambda i: CS.IDS[i])
def test_seventy_chains_in_one_launch_equal_each_chain_alone(i, dtype):
    c, ref = CS.build(i), CS.reference(i)
    assert c["C"] == 70
    u = ref["us"][0]
    x, flags, logs = device_sweep(c, u, dtype)
    init, kernel = get_kernel(*fns(c["model"]), c["parallel"])
    for k in range(70):
        o = kernel(None, init(c["x"][k].astype(dtype)), c["delta"],
                   noise=dict(eps_aux=c["eps_aux"][k].astype(dtype), eps_samp=c["eps_samp"][k].astype(dtype), u_accept=u[k]))
        assert o.x.shape == (c["T"], c["d"])
        npt.assert_array_equal(o.x, x[k])
        assert o.updated == flags[k]
        npt.assert_array_equal(o.logs[0], logs[k])


@pytest.mark.parametrize("i", [6, 9], ids=lambda i: CS.IDS[i])
def test_three_sweeps_on_resident_chains(i):
    c = CS.build(i)
    h, ch, _ = resident_pair(c, np.float64)
    init, kernel = get_kernel(*fns(c["model"]), c["parallel"])
    rng = np.random.default_rng(i)
    xs = c["x"].copy()
    state = KalmanSampler(x=ch, updated=None)
    n_acc = 0
    for s in range(3):
        shape = xs.shape
        noise = dict(eps_aux=rng.standard_normal(shape), eps_samp=rng.standard_normal(shape), u_accept=rng.random(c["C"]) ** 8)
        state = kernel(None, state, c["delta"], noise=noise)
        assert state.x is ch
        flags = []
        for k in range(c["C"]):
            o = CS.oracle_sweep(c["model"], xs[k], c["delta"], c["parallel"], noise["eps_aux"][k], noise["eps_samp"][k], noise["u_accept"][k])
            assert abs(min(o["log_alpha"], 0.0) - np.log(noise["u_accept"][k])) > 1e-6
            xs[k] = o["x"][..., 0]
            flags.append(o["accepted"])
        n_acc += sum(flags)
        npt.assert_array_equal(ch.accepted.to_host() != 0, flags)
        npt.assert_allclose(ch.to_host(), xs, rtol=1e-9, atol=1e-10)
    assert n_acc > 0


@pytest.mark.parametrize("order", [1, 2])
def test_loop_drives_the_kernel_on_resident_chains(order, monkeypatch):
    """loop() with delta_adaptation for 30 sweeps (the step size lives on the device: auxssm_kalman_sweep_dd), then 30 sampling sweeps, against oracle/loop_np.py chain
    by chain on the noise the device draws; bars of tests/test_gpu_loop.py.  No device-to-host copy happens between the first and the last sweep of a run."""
    from aux_ssm_samplers_amd.common import delta_adaptation
    from aux_ssm_samplers_amd.loop import loop
    from oracle import loop_np as L
    from tests.test_gpu_loop import _device_noise
    T, grid, Cn = 6, 2, 3
    d = grid * grid
    rng = np.random.default_rng(order)
    from aux_ssm_samplers_amd.workloads import spatial_precision
    y = np.cumsum(rng.standard_normal((T, d)), 0) + rng.standard_normal((T, d))
    model = MVTModel(y, np.zeros(d), np.ones(d), np.ones(d), np.ones(d), np.zeros(d), 3.0, spatial_precision(grid), order=order)
    init, kernel = get_kernel(*fns(model), True)
    h = _lib.default_handle()
    x0 = y[None] + 0.5 * rng.standard_normal((Cn, T, d))
    chains = DeviceChains(h, x0, chain_minor=False)
    copies = [0]
    real = _lib.DeviceArray.to_host
    monkeypatch.setattr(_lib.DeviceArray, "to_host", lambda self: (copies.__setitem__(0, copies[0] + 1), real(self))[1])
    beta, target_alpha, lr = 0.2, 0.5, 0.6
    xs = x0.copy()
    state, delta = KalmanSampler(x=chains, updated=True), 0.8
    for phase, (key, delta_fn) in enumerate(((R.PRNGKey(5), functools.partial(delta_adaptation, min_delta=1e-3, max_delta=10.0)), (R.PRNGKey(6), None))):
        n_iter = 30
        seen = []
        n, stats, state, delta_out, window, avg = loop(key, delta, state, kernel, delta_fn, n_iter, target_alpha=target_alpha, lr=lr, beta=beta,
                                                       callback=lambda i, s: seen.append(copies[0]))
        assert len(seen) == n_iter and seen[0] == seen[-1]          # nothing came back to the host inside the run
        keys = R.split(key, n_iter)
        upd0 = np.ones((Cn, 1)) if phase == 0 else upd.astype(float)
        st = [L.stats_fn(xs[c], xs[c]) for c in range(Cn)]
        avg_h, win_h = upd0.copy(), upd0.copy()
        dl, n_acc = delta, 0
        for i in range(n_iter):
            ea, es, ua = _device_noise(h, keys[i], None, Cn, np.float64, chains)
            upd = np.zeros((Cn, 1), bool)
            for c in range(Cn):
                ref = CS.oracle_sweep(model, xs[c], dl, True, ea[c], es[c], ua[c])
                xn = ref["x"][..., 0]
                st[c] = tuple(L.fold(i, u_, v_) for u_, v_ in zip(st[c], L.stats_fn(xs[c], xn)))
                xs[c] = xn
                upd[c, 0] = ref["accepted"]
            n_acc += upd.sum()
            avg_h, win_h = L.accept_update(i, beta, upd, avg_h, win_h)
            if delta_fn is not None:
                dl = float(L.pooled_delta_adaptation(dl, target_alpha, win_h, (n_iter - i) * lr / n_iter, 1e-3, 10.0)[0])
        assert 0 < n_acc < Cn * n_iter
        npt.assert_allclose(chains.to_host(), xs, rtol=1e-8, atol=1e-9)
        for k in range(3):
            npt.assert_allclose(chains.stats_to_host(stats[k]), np.stack([st[c][k] for c in range(Cn)]), rtol=1e-8, atol=1e-9)
        npt.assert_array_equal(avg.to_host().reshape(Cn, 1), avg_h)
        npt.assert_array_equal(window.to_host().reshape(Cn, 1), win_h)
        npt.assert_allclose(delta_out, dl, rtol=1e-12)
        delta = delta_out


def test_jax_compat_sweep_is_the_explicit_sweep_on_the_references_draws():
    c = CS.build(6)
    init, kernel = get_kernel(*fns(c["model"]), True)
    x = c["x"][0][..., None]
    key = np.array([2024, 11], np.uint32)
    prev = R.set_compat("jax")
    try:
        got = kernel(key, init(x), c["delta"])
        nz = R.jax_kalman_noise(key[None], c["T"], c["d"], np.float64)
    finally:
        R.set_compat(prev)
    want = kernel(None, init(x), c["delta"], noise=dict(eps_aux=nz["eps_aux"][0], eps_samp=nz["eps_samp"][0], u_accept=float(nz["u_accept"][0])))
    assert got.x.shape == x.shape
    npt.assert_array_equal(got.x, want.x)
    npt.assert_array_equal(got.logs, want.logs)
    assert got.updated == want.updated and np.isfinite(got.logs).all()


def _c_sweep(h, model, ch, dims, layout, fused=False):
    dl, _, yarr = model.device(h, ch.dtype)
    head = (h.h, _lib.dtype_code(ch.dtype), model.kmodel, C.byref(dims), C.byref(dl.c), C.byref(yarr))
    keys = (C.c_uint32 * 6)(1, 2, 3, 4, 5, 6)
    if fused:
        ch.x_alt, ch.sel = h.zeros(ch.x.shape, ch.dtype), h.zeros((ch.C,), np.int32)
        return h.lib.auxssm_kalman_sweep_fused(*head, 0.5, None, keys, 1, _lib.NAN_REFERENCE, layout, ch.x.ptr, ch.x_alt.ptr, ch.sel.ptr, ch.u_acc.ptr,
                                               ch.accepted.ptr, ch.logs.ptr)
    return h.lib.auxssm_kalman_sweep_keyed(*head, 0.5, None, keys, 1, _lib.NAN_REFERENCE, layout, ch.x.ptr, ch.eps_aux.ptr, ch.eps_samp.ptr, ch.u_acc.ptr,
                                           ch.accepted.ptr, ch.logs.ptr)


@pytest.mark.parametrize("order", [1, 2])
def test_refusals_enqueue_nothing(order):
    h = _lib.default_handle()
    T, d, Cn = 4, 4, 34
    model = MVTModel(np.zeros((T, d)), np.zeros(d), np.ones(d), np.ones(d), np.ones(d), np.zeros(d), 3.0, np.eye(d), order=order)
    x0 = np.random.default_rng(0).standard_normal((Cn, T, d))

    def untouched(ch):
        npt.assert_array_equal(ch.to_host(), x0)
        assert not ch.accepted.to_host().any() and not ch.logs.to_host().any()

    # the fused entry keeps refusing everything but LG_CONCAT, with its message
    ch = DeviceChains(h, x0, chain_minor=False)
    assert _c_sweep(h, model, ch, _lib.Dims(Cn, T, 1, d, d), _lib.LAYOUT_DENSE, fused=True) == _lib.ERR_UNSUPPORTED
    assert h.lib.auxssm_last_error().decode() == f"auxssm_kalman_sweep_fused runs AUXSSM_KMODEL_LG_CONCAT (model_kind {model.kmodel}: use auxssm_kalman_sweep_keyed)"
    untouched(ch)
    assert not ch.x_alt.to_host().any() and not ch.sel.to_host().any()
    # the chain-minor layout
    ch = DeviceChains(h, x0, chain_minor=False)
    assert _c_sweep(h, model, ch, _lib.Dims(Cn, T, 1, d, d), _lib.LAYOUT_CHAIN_MINOR) == _lib.ERR_UNSUPPORTED
    assert "dx <= 64" in h.lib.auxssm_last_error().decode() and "dense" in h.lib.auxssm_last_error().decode()
    untouched(ch)
    # d = 65: the model's arrays are never read (the refusal comes first), so the d = 4 model stands in
    x65 = np.zeros((2, T, 65))
    ch65 = DeviceChains(h, x65, chain_minor=False)
    assert _c_sweep(h, model, ch65, _lib.Dims(2, T, 1, 65, 65), _lib.LAYOUT_DENSE) == _lib.ERR_UNSUPPORTED
    assert "dx <= 64" in h.lib.auxssm_last_error().decode() and "65" in h.lib.auxssm_last_error().decode()
    assert not ch65.to_host().any() and not ch65.logs.to_host().any()
    # the masked NaN policy is refused, not silently read as the reference one
    dl, _, yarr = model.device(h, ch.dtype)
    dims = _lib.Dims(Cn, T, 1, d, d)
    rc = h.lib.auxssm_kalman_sweep(h.h, _lib.dtype_code(ch.dtype), model.kmodel, C.byref(dims), C.byref(dl.c), C.byref(yarr), 0.5, 1, _lib.NAN_MASKED, _lib.LAYOUT_DENSE,
                                   ch.x.ptr, ch.eps_aux.ptr, ch.eps_samp.ptr, ch.u_acc.ptr, ch.accepted.ptr, ch.logs.ptr)
    assert rc == _lib.ERR_UNSUPPORTED and "nan_policy" in h.lib.auxssm_last_error().decode()
    untouched(ch)
    # and through Python: chain-minor resident chains
    init, kernel = get_kernel(*fns(model), True)
    with pytest.raises(ValueError, match="chain_minor=False"):
        kernel(R.PRNGKey(0), KalmanSampler(x=DeviceChains(h, x0, chain_minor=True), updated=None), 0.5)


# ---- ground truth without a restatement --------------------------------------------------------------------------------------------------------------
def quadrature_moments(y, nu, prec, n, half=9.0):
    """first and second moments (and the second moments' standard deviations) of x = (x_00, x_01, x_10, x_11) under
    p(x) ~ N(x_0; 0, I) N(x_1; x_0, I) g_0(x_0) g_1(x_1), by the trapezoid rule on the tensor grid of n^4 points, [-half, half]^4: the integrand factorises as
    M[a, b] Q[a, c] Q[b, d] N[c, d], so the 4-dimensional sums are evaluated as matrix products"""
    g = np.linspace(-half, half, n)
    A, B = np.meshgrid(g, g, indexing="ij")

    def pot(t):
        r0, r1 = y[t, 0] - A, y[t, 1] - B
        q = prec[0, 0] * r0 * r0 + 2 * prec[0, 1] * r0 * r1 + prec[1, 1] * r1 * r1
        return (1 + q / nu) ** (-0.5 * (nu + 2))

    M = np.exp(-0.5 * (A * A + B * B)) * pot(0)
    N = pot(1)
    Q = np.exp(-0.5 * (g[:, None] - g[None, :]) ** 2)
    fwd = Q.T @ M @ Q            # [c, d] = sum_ab M[a, b] Q[a, c] Q[b, d]
    bwd = Q @ N @ Q.T            # [a, b]
    p0, p1 = M * bwd, fwd * N    # the marginals of (x_00, x_01) and (x_10, x_11), unnormalised
    out = []
    for p, ax in ((p0, A), (p0, B), (p1, A), (p1, B)):
        z = p.sum()
        m1, m2, m4 = (p * ax).sum() / z, (p * ax ** 2).sum() / z, (p * ax ** 4).sum() / z
        out.append((m1, m2, np.sqrt(m2 - m1 ** 2), np.sqrt(m4 - m2 ** 2)))
    return np.array(out)


@pytest.mark.parametrize("order", [1, 2])
def test_posterior_moments_against_quadrature(order):
    """d = 2, T = 2, nu = 3, prec = [[1, -0.25], [-0.25, 1]]: 1024 resident chains, 60 burn-in + 400 sampling sweeps through loop(); every first and second moment
    within 5 empirical standard errors (the spread of the per-chain time averages over sqrt(chains)) of the quadrature's, each standard error below 2 % of that
    quantity's posterior standard deviation (x: sd(x); x^2: sd(x^2))."""
    from aux_ssm_samplers_amd.loop import loop
    y = np.array([[0.5, -0.3], [1.0, 0.4]])
    nu, prec = 3.0, np.array([[1.0, -0.25], [-0.25, 1.0]])
    coarse, fine = quadrature_moments(y, nu, prec, 241), quadrature_moments(y, nu, prec, 361)
    assert np.max(np.abs(coarse - fine)) < 1e-8                       # refined until the moments stand still
    model = MVTModel(y, np.zeros(2), np.ones(2), np.ones(2), np.ones(2), np.zeros(2), nu, prec, order=order)
    init, kernel = get_kernel(*fns(model), True)
    h = _lib.default_handle()
    Cn = 1024
    chains = DeviceChains(h, np.random.default_rng(order).standard_normal((Cn, 2, 2)), chain_minor=False)
    delta = 1.5
    *_, state, _, _, _ = loop(R.PRNGKey(10 + order), delta, KalmanSampler(x=chains, updated=True), kernel, None, 60)
    _, stats, state, _, _, avg = loop(R.PRNGKey(20 + order), delta, state, kernel, None, 400)
    acc = float(avg.to_host().mean())
    assert 0.1 < acc < 0.99, acc
    m1 = chains.stats_to_host(stats[1]).reshape(Cn, 4)                # per-chain time averages of x and x^2, coordinates in the order of `fine`
    m2 = chains.stats_to_host(stats[2]).reshape(Cn, 4)
    for est, truth, sd in ((m1, fine[:, 0], fine[:, 2]), (m2, fine[:, 1], fine[:, 3])):
        se = est.std(axis=0, ddof=1) / np.sqrt(Cn)
        print(f"order {order}: acceptance {acc:.3f}  estimate {est.mean(0)}  truth {truth}  se {se}  sd {sd}")
        assert np.all(se < 0.02 * sd), (se, sd)
        assert np.all(np.abs(est.mean(axis=0) - truth) < 5 * se), (est.mean(0), truth, se)
