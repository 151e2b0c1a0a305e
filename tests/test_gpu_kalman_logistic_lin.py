"""kalman.BinomialLinearModel / NegBinomialLinearModel on the device (AUXSSM_KMODEL_LOGISTIC_LIN_FIRST / _SECOND: csrc/kalman_plin.hip::k_plin_obs_logistic behind
api.hip::sweep_ss) against the oracle's sweep (oracle.kalman_np.kalman_sweep) driven by the model's own NumPy factories, on identical explicit noise and in fp64,
at the tolerances of tests/test_gpu_kalman_logistic.py: x at rtol 1e-9 / atol 1e-10, the four log terms at rtol 1e-9, log alpha at 1e-9 of the largest of them
(a start at |eta| = 30 puts them at 1e4 .. 1e5), accept flags exact.  The cells, their special entries and the placed acceptance uniforms are
tests/kalman_logistic_lin_cases.py's: every chain the oracle ran has a margin |log alpha - log u| >= 0.05, so an accept flag that differs is a defect.  Then: the
reduction to the pointwise logistic sweep at H = I, the host-factory path, loop() with the step size on the device, jax compatibility, the C entry points, fp32
against the fp64 oracle (bars from measured errors), and the sampler against the exact posterior by quadrature."""
import ctypes as C

import numpy as np
import numpy.testing as npt
import pytest

from tests import kalman_logistic_lin_cases as LC

pytestmark = pytest.mark.gpu


def fns(model):
    return model.dynamics_factory, model.observations_factory, model.log_likelihood_fn


def resident_sweep(cell, u, dtype=np.float64, parallel=True):
    """one sweep of all the cell's chains on dense resident buffers -> (x (C, T, d), flags (C,) bool, logs (C, 5))"""
    from aux_ssm_samplers_amd import _lib
    from aux_ssm_samplers_amd.kalman import get_kernel
    from aux_ssm_samplers_amd.kalman.generic import DeviceChains, KalmanSampler
    init, kernel = get_kernel(*fns(cell["model"]), parallel)
    chains = DeviceChains(_lib.default_handle(), cell["x"].astype(dtype), chain_minor=False)
    kernel(None, KalmanSampler(x=chains, updated=None), cell["delta"], noise=dict(eps_aux=cell["eps_aux"], eps_samp=cell["eps_samp"], u_accept=u))
    return chains.to_host(), chains.accepted.to_host() != 0, chains.logs.to_host()


def la_atol(ref_logs):
    """log alpha is a difference of the four log terms: 1e-9 relative to the largest of them (tests/test_gpu_kalman_logistic.py's rule)"""
    return 1e-9 * np.maximum(1.0, np.abs(ref_logs[:, 1:]).max(axis=1))


def check_against_oracle(ref, x, flags, logs, u_index=0):
    """the oracle's chains of one resident sweep"""
    cell, idx = ref["cell"], ref["chains"]
    npt.assert_allclose(logs[idx, 1:], ref["logs"][:, 1:], rtol=1e-9)
    assert np.all(np.abs(logs[idx, 0] - ref["logs"][:, 0]) <= la_atol(ref["logs"]) + 1e-9 * np.abs(ref["logs"][:, 0]))
    npt.assert_array_equal(flags[idx], ref["accepted"][u_index])
    want = np.where(ref["accepted"][u_index][:, None, None], ref["x_prop"], cell["x"][idx])
    npt.assert_allclose(x[idx], want, rtol=1e-9, atol=1e-10)


@pytest.mark.parametrize("family", LC.FAMILIES)
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("dx,dy,T", LC.ONE_CHAIN_SHAPES)
@pytest.mark.parametrize("parallel", [True, False])
def test_one_chain_vs_oracle(family, order, dx, dy, T, parallel):
    """One chain through get_kernel's host-state form: both scan forms, both orders, both families.  (1, 1, 2) and (1, 3, 3) are the pathwise sampler's first and
    only interior step, (2, 7, 257) has two step tiles, the second with one live lane, (4, 65, 150) is one channel past a 64-column block, (3, 130, 40) has a
    ragged third block, (1, 257, 24) a ragged fifth on a scalar state.  The chain starts at |eta| = 30 in one channel.  Two sweeps on the same noise, one uniform
    on each side of the oracle's log alpha."""
    from aux_ssm_samplers_amd.kalman import get_kernel
    ref = LC.reference(family, dx, dy, T, 1, order, parallel)
    cell = ref["cell"]
    model, (ts, ks) = cell["model"], cell["sat"]
    assert (model.yobs == 0).any() and abs(cell["x"][0, ts] @ model.H[ks] + model.c[ks]) >= 30 - 1e-9 and (dy == 1 or np.isnan(model.yobs).sum() >= dy + 1)
    init, kernel = get_kernel(*fns(model), parallel)
    for k, u in enumerate(ref["us"]):
        out = kernel(None, init(cell["x"][0]), cell["delta"], noise=dict(eps_aux=cell["eps_aux"][0], eps_samp=cell["eps_samp"][0], u_accept=float(u[0])))
        npt.assert_allclose(out.logs[0, 1:], ref["logs"][0, 1:], rtol=1e-9)
        assert abs(out.log_alpha - ref["logs"][0, 0]) <= la_atol(ref["logs"])[0] + 1e-9 * abs(ref["logs"][0, 0])
        assert out.updated == bool(ref["accepted"][k][0])
        npt.assert_allclose(out.x, ref["x_prop"][0] if out.updated else cell["x"][0], rtol=1e-9, atol=1e-10)


@pytest.mark.parametrize("family", LC.FAMILIES)
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("dx,dy,T,Cn,every", LC.CHAIN_SHAPES)
def test_dense_resident_chains_vs_oracle(family, order, dx, dy, T, Cn, every):
    """Several dense resident chains in one launch: 33 and 5 chains end in a ragged group of the factory's four chains per workgroup, (1, 3, 300, 40) has two time
    tiles per chain.  The oracle's chains carry the placed uniforms and hold both outcomes; every third chain starts at the saturated point."""
    ref = LC.reference(family, dx, dy, T, Cn, order, True, every)
    assert ref["accepted"][0].any() and not ref["accepted"][0].all()
    check_against_oracle(ref, *resident_sweep(ref["cell"], ref["us"][0]))


@pytest.mark.parametrize("family", LC.FAMILIES)
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("d,T,Cn", [(1, 300, 40), (4, 70, 64)])
def test_identity_loadings_reduce_to_the_pointwise_logistic_sweep(family, order, d, T, Cn):
    """H = I, c = 0, dx = dy: one sweep equals BinomialModel's / NegBinomialModel's dense sweep (kinds 13 / 14, pinned by tests/test_gpu_kalman_logistic.py) on the
    same data and noise, with one size per component (the largest of the pointwise cell's, the data clipped to it)."""
    from aux_ssm_samplers_amd import kalman
    from tests import kalman_logistic_cases as PC
    from tests.test_gpu_kalman_logistic import resident_sweep as pointwise_sweep
    cell = dict(PC._build(family, d, T, Cn, order, 0))
    pm = cell["model"]
    par = np.where(np.isfinite(pm.size), pm.trials if family == "binomial" else pm.r, 1.0).max(axis=0)
    y = np.minimum(pm.yobs, par) if family == "binomial" else pm.yobs
    lin_cls, pw_cls = ((kalman.BinomialLinearModel, kalman.BinomialModel) if family == "binomial" else (kalman.NegBinomialLinearModel, kalman.NegBinomialModel))
    dyn = (pm.m0, pm.P0, pm.F, pm.Q, pm.b)
    u = np.random.default_rng(5).random(Cn)
    want = pointwise_sweep(dict(cell, model=pw_cls(y, par, *dyn, order=order)), u, chain_minor=False)
    got = resident_sweep(dict(cell, model=lin_cls(y, par, np.eye(d), 0.0, *dyn, order=order)), u)
    npt.assert_allclose(got[0], want[0], rtol=1e-9, atol=1e-10)
    npt.assert_allclose(got[2][:, 1:], want[2][:, 1:], rtol=1e-9)
    assert np.all(np.abs(got[2][:, 0] - want[2][:, 0]) <= la_atol(want[2]) + 1e-9 * np.abs(want[2][:, 0]))
    sure = np.abs(np.minimum(want[2][:, 0], 0.0) - np.log(u)) > 1e-4
    npt.assert_array_equal(got[1][sure], want[1][sure])
    assert sure.sum() >= Cn - 2 and np.isfinite(want[2]).all() and np.abs(got[0] - cell["x"]).max() > 1e-3


@pytest.mark.parametrize("family", LC.FAMILIES)
@pytest.mark.parametrize("order", [1, 2])
def test_host_factory_path_equals_device_sweep(family, order):
    """Hiding the model behind lambdas forces the generic host-factory path (NumPy factories + GPU primitives)."""
    from aux_ssm_samplers_amd.kalman import get_kernel
    ref = LC.reference(family, 2, 7, 257, 1, order, True)
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
def test_loop_with_the_step_size_on_the_device_equals_three_kernel_calls(family, order):
    """loop() under common.delta_adaptation keeps the step size on the device (auxssm_kalman_sweep_dd through the keyed sweep); with an adaptation rate of 0 the rule
    leaves it where it is, so three sweeps of loop() are three kernel calls on the same keys with the host step size -- bit for bit, state and log terms: the
    per-chain totals are reduced in a fixed order."""
    from aux_ssm_samplers_amd import _lib, random as R
    from aux_ssm_samplers_amd.common import delta_adaptation
    from aux_ssm_samplers_amd.kalman import get_kernel
    from aux_ssm_samplers_amd.kalman.generic import DeviceChains, KalmanSampler
    from aux_ssm_samplers_amd.loop import loop
    cell = LC.reference(family, 1, 3, 300, 40, order, True, 7)["cell"]
    init, kernel = get_kernel(*fns(cell["model"]), True)
    h = _lib.default_handle()
    key, delta = R.PRNGKey(3 + order), cell["delta"]
    a = DeviceChains(h, cell["x"], chain_minor=False)
    _, _, state, delta_out, _, _ = loop(key, delta, KalmanSampler(x=a, updated=True), kernel, delta_adaptation, 3, target_alpha=0.5, lr=0.0)
    assert delta_out == delta
    b = DeviceChains(h, cell["x"], chain_minor=False)
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


@pytest.mark.parametrize("family", LC.FAMILIES)
def test_jax_compat_sweep_is_the_explicit_sweep_on_the_references_draws(family):
    from aux_ssm_samplers_amd import random as R
    from aux_ssm_samplers_amd.kalman import get_kernel
    cell = LC.reference(family, 4, 65, 150, 1, 2, True)["cell"]
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
    """auxssm_kalman_sweep_keyed runs kinds 15 and 16; auxssm_kalman_sweep_fused goes on refusing everything but LG_CONCAT, with its message, and enqueues nothing;
    the chain-minor layout, dx = 5 and dy = 1025 are refused with their codes, their limits and this model's name, a NULL Hs / cs / yobs as an argument error --
    state, flags and logs untouched."""
    from aux_ssm_samplers_amd import _lib
    from aux_ssm_samplers_amd.kalman.generic import DeviceChains
    cell = LC.reference("negbinomial", 2, 7, 129, 33, 1, True, 7)["cell"]
    model, x0 = cell["model"], cell["x"]
    assert model.kmodel == 15
    h = _lib.default_handle()
    keys = (C.c_uint32 * 6)(1, 2, 3, 4, 5, 6)
    err = lambda: h.lib.auxssm_last_error().decode()

    def call(kind, fused=False, chain_minor=False, dx=None, dy=None, null=None):
        xs = x0 if dx is None else np.zeros((cell["C"], cell["T"], dx))
        ch = DeviceChains(h, xs, chain_minor=chain_minor)
        dl, _, yarr = model.device(h, ch.dtype)
        lg = _lib.Lgssm.from_buffer_copy(dl.c)
        ya = _lib.Arr.from_buffer_copy(yarr)
        if null in ("Hs", "cs"):
            setattr(lg, null, _lib.Arr(None, 0, 0, 0))
        if null == "yobs":
            ya = _lib.Arr(None, 0, 0, 0)
        dims = _lib.Dims(cell["C"], cell["T"], 1, ch.dx, cell["dy"] if dy is None else dy)
        head = (h.h, _lib.dtype_code(ch.dtype), kind, C.byref(dims), C.byref(lg), C.byref(ya))
        if fused:
            ch.x_alt, ch.sel = h.zeros(ch.x.shape, ch.dtype), h.zeros((ch.C,), np.int32)
            rc = h.lib.auxssm_kalman_sweep_fused(*head, 0.005, None, keys, 1, _lib.NAN_REFERENCE, ch.layout, ch.x.ptr, ch.x_alt.ptr, ch.sel.ptr, ch.u_acc.ptr,
                                                 ch.accepted.ptr, ch.logs.ptr)
        else:
            rc = h.lib.auxssm_kalman_sweep_keyed(*head, 0.005, None, keys, 1, _lib.NAN_REFERENCE, ch.layout, ch.x.ptr, ch.eps_aux.ptr, ch.eps_samp.ptr, ch.u_acc.ptr,
                                                 ch.accepted.ptr, ch.logs.ptr)
        return rc, ch, xs

    def untouched(ch, xs):
        npt.assert_array_equal(ch.to_host(), xs)
        assert not ch.accepted.to_host().any() and not ch.logs.to_host().any()

    for kind in (_lib.KMODEL_LOGISTIC_LIN_FIRST, _lib.KMODEL_LOGISTIC_LIN_SECOND):
        rc, ch, xs = call(kind, fused=True, chain_minor=True)
        assert rc == _lib.ERR_UNSUPPORTED
        assert err() == f"auxssm_kalman_sweep_fused runs AUXSSM_KMODEL_LG_CONCAT (model_kind {kind}: use auxssm_kalman_sweep_keyed)"
        untouched(ch, xs)
        assert not ch.x_alt.to_host().any() and not ch.sel.to_host().any()
        rc, ch, xs = call(kind, chain_minor=True)
        assert rc == _lib.ERR_UNSUPPORTED and "logistic-linear" in err() and "dense" in err() and "dx <= 4" in err() and "dy <= 1024" in err(), err()
        untouched(ch, xs)
        rc, ch, xs = call(kind, dx=5)
        assert rc == _lib.ERR_UNSUPPORTED and "logistic-linear" in err() and "dx <= 4" in err() and "dx = 5" in err(), err()
        untouched(ch, xs)
        rc, ch, xs = call(kind, dy=1025)
        assert rc == _lib.ERR_UNSUPPORTED and "logistic-linear" in err() and "dy <= 1024" in err() and "dy = 1025" in err(), err()
        untouched(ch, xs)
        for null in ("Hs", "cs", "yobs"):
            rc, ch, xs = call(kind, null=null)
            assert rc == _lib.ERR_ARG and "logistic-linear" in err() and "[c; s; w] (3, dy)" in err(), (null, rc, err())
            untouched(ch, xs)
        rc, ch, xs = call(kind)
        assert rc == 0, err()
        logs = ch.logs.to_host()
        assert np.isfinite(logs).all() and logs.any() and np.abs(ch.to_host() - x0).max() > 1e-3


# ---- fp32 ----------------------------------------------------------------------------------------------------------------------------------------------
# The bars are twice the worst error observed on the MI355X over the cases below, rounded up to one digit (the project's standing rule): see the
# test's docstring.
F32_X_BAR = 2e-6     # observed 5.88e-7
F32_LA_BAR = 5e-2    # observed 2.03e-2
F32_CASES = ([(f,) + s + (1, 1, order) for f in LC.FAMILIES for s in LC.ONE_CHAIN_SHAPES for order in (1, 2)]
             + [(f,) + s + (order,) for f in LC.FAMILIES for s in LC.CHAIN_SHAPES for order in (1, 2)])


@pytest.mark.parametrize("family,dx,dy,T,Cn,every,order", F32_CASES)
def test_fp32_against_the_fp64_oracle(family, dx, dy, T, Cn, every, order):
    """Every cell in float32, against the float64 oracle on the float32-rounded inputs (model, state and noise).  Measured: max |error| / max |value| of x_prop and
    the absolute error of log alpha.  Accept flags are asserted only for chains whose margin exceeds the log alpha bar.
    Observed on the MI355X (one run, the 40 cases), x_prop relative error / log alpha absolute error, binomial first order | second order | negative binomial
    first order | second order:
        (1, 1, 2)        5.7e-08 / 1.4e-03 | 2.1e-07 / 1.4e-03 | 1.6e-07 / 3.2e-03 | 1.4e-07 / 2.3e-03
        (1, 3, 3)        2.7e-08 / 5.5e-04 | 2.5e-07 / 1.2e-03 | 1.8e-07 / 1.1e-04 | 7.1e-08 / 1.4e-03
        (2, 7, 257)      1.3e-07 / 3.1e-03 | 2.6e-07 / 8.1e-03 | 4.1e-07 / 5.6e-03 | 2.0e-07 / 2.1e-03
        (3, 5, 70)       1.6e-07 / 1.0e-03 | 9.4e-08 / 9.0e-04 | 8.4e-08 / 1.5e-03 | 2.3e-07 / 1.7e-04
        (4, 65, 150)     2.3e-07 / 3.1e-03 | 2.9e-07 / 1.1e-02 | 1.5e-07 / 1.3e-04 | 1.5e-07 / 6.5e-03
        (3, 130, 40)     9.5e-08 / 1.6e-03 | 2.1e-07 / 3.9e-03 | 1.2e-07 / 3.0e-04 | 2.7e-07 / 1.1e-04
        (1, 257, 24)     2.3e-07 / 1.0e-03 | 6.0e-08 / 3.8e-03 | 2.4e-07 / 1.1e-03 | 7.0e-08 / 5.2e-03
        (2, 7, 129, 33)  1.5e-07 / 4.7e-03 | 1.6e-07 / 4.7e-03 | 1.3e-07 / 3.6e-03 | 5.9e-07 / 6.2e-03
        (4, 65, 70, 5)   1.3e-07 / 3.3e-03 | 2.0e-07 / 1.2e-02 | 4.5e-07 / 3.6e-03 | 2.5e-07 / 1.1e-02
        (1, 3, 300, 40)  1.1e-07 / 7.1e-03 | 2.3e-07 / 1.1e-02 | 1.8e-07 / 2.0e-02 | 2.5e-07 / 1.4e-02
    Worst: x_prop 5.88e-7 (negative binomial (2, 7, 129, 33), order 2), log alpha 2.03e-2 (negative binomial (1, 3, 300, 40), order 1).  Bars: twice that,
    rounded up to one digit -- 2e-6 and 5e-2.  The log alpha error is absolute on four log terms of 8e3 .. 1.8e5 (every third chain starts at |eta| = 30, a few
    hundred prior standard deviations out): 2e-2 is 5e-7 of the largest term of its cell, a few float32 ulp, as x_prop's error is of the state."""
    ref = LC.reference(family, dx, dy, T, Cn, order, True, every, True)
    cell, idx = ref["cell"], ref["chains"]
    # every chain is made to accept, so that the state that comes back is x_prop
    x, _, logs = resident_sweep(cell, np.zeros(Cn), np.float32)
    ex = np.abs(x[idx].astype(np.float64) - ref["x_prop"]).max() / np.abs(ref["x_prop"]).max()
    ela = np.abs(logs[idx, 0].astype(np.float64) - ref["logs"][:, 0]).max()
    print(f"fp32 {family} dx={dx} dy={dy} T={T} C={Cn} order={order}: x_prop rel err {ex:.3e}  log alpha abs err {ela:.3e}  (log alpha in "
          f"[{ref['logs'][:, 0].min():.1f}, {ref['logs'][:, 0].max():.1f}], largest log term {np.abs(ref['logs'][:, 1:]).max():.3g}, delta {cell['delta']:.3g})")
    assert np.isfinite(x).all() and np.isfinite(logs).all()
    assert ex < F32_X_BAR and ela < F32_LA_BAR
    for k, u in enumerate(ref["us"]):
        _, flags, _ = resident_sweep(cell, u, np.float32)
        sure = np.abs(np.minimum(ref["logs"][:, 0], 0.0) - np.log(u[idx])) > F32_LA_BAR
        npt.assert_array_equal(flags[idx][sure], ref["accepted"][k][sure])


# ---- ground truth without a restatement ------------------------------------------------------------------------------------------------------------------
QUAD_C = 16384


def _check(step, read, exact, burn, M):
    """tests/test_gpu_kalman_poisson_lin.py::_check, its tolerances unchanged: step(i) = one sweep of all chains, read() -> (C, T d) current states.  The standard
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


# (a-priori first-order bounds 4 / lambda_max(H' diag(m) H): 2.63 and 0.63; the CPU oracle accepts 0.93 .. 1.00 at these)
QUAD_DELTA = {("scalar", 1): 1.0, ("scalar", 2): 1.0, ("planar", 1): 0.5, ("planar", 2): 0.8}


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("name", ["scalar", "planar"])
def test_sampler_targets_the_exact_posterior_by_quadrature(name, order):
    """16 384 dense resident chains, Threefry noise, both orders, as many sweeps as the Poisson-linear quadrature test runs (40 + 160).  scalar: dx = 1, dy = 3,
    T = 3, binary data, one entry missing (a 3-D grid); planar: dx = 2, dy = 3, T = 2, negative binomial with r = 0.5 and a dense H, so that Omega is truly
    non-diagonal (a 4-D grid).  Each grid agrees with its refinement to 1e-6 relative (tests/test_kalman_logistic_lin_model.py checks that on the CPU; asserted
    here again, from the cache)."""
    from aux_ssm_samplers_amd import _lib, random as R
    from aux_ssm_samplers_amd.kalman import get_kernel
    from aux_ssm_samplers_amd.kalman.generic import DeviceChains, KalmanSampler
    coarse, exact = LC.quad_exact(name)
    npt.assert_allclose(coarse, exact, rtol=1e-6, atol=1e-9)
    model = LC.quad_model(name, order)
    T, d = model.T, model.dx
    init, kernel = get_kernel(*fns(model), True)
    rng = np.random.default_rng(1)
    chains = DeviceChains(_lib.default_handle(), exact[:, 0].reshape(1, T, d) + 0.3 * rng.standard_normal((QUAD_C, T, d)), chain_minor=False)
    state = KalmanSampler(x=chains, updated=None)
    burn, M, delta = 40, 160, QUAD_DELTA[name, order]
    keys = R.split(R.PRNGKey(41 + order), burn + M)
    acc = []
    _check(lambda i: (kernel(keys[i], state, delta), acc.append(chains.accepted.to_host().mean()) if i % 40 == 0 else None),
           lambda: chains.to_host().reshape(QUAD_C, T * d), exact, burn, M)
    print(f"quadrature {name} order {order}: delta {delta}, acceptance {np.mean(acc):.3f}")
    assert 0.2 < np.mean(acc) <= 1.0, np.mean(acc)
