"""GPU: the conjugate step on linear-Gaussian dynamics (csrc/dynamics_theta.hip, loop.DynamicsThetaStep) against the literal restatement
tests/dynamics_theta_np.py.  Cells (tests/dynamics_theta_cases.py): d = 1 .. 4; T = 2, 3, a segment less one, a segment plus one / two, three segments and a
ragged tail; C = 1, 3, 33, 70; each layout forced through DeviceChains(chain_minor=...); float64 and float32 states.
  1. auxssm_dynamics_stats and post_out                       fp64 at 1e-9 relative (to the largest entry of each matrix); fp32 states against the restatement
  2. explicit-noise draws (F, b, Q), Q symmetric bit for bit,   on the same float32-rounded inputs, at FP32_*_BAR (measured: see there)
     a chain alone = the chain in its batch bit for bit, a degenerate chain keeps its parameters and raises its flag
  3. auxssm_rng_gamma at 1e-10 relative on keys whose restatement takes no decision within 1e-9 of its threshold, every draw compared; moments of the device's draws
  4. moments of the step: 4096 chains on one trajectory, one keyed call
  5. the sweep behind the step, per model class, order and layout: the C-chain sweep on per-chain parameters = one-chain sweeps of fresh models built from them
  6. joint ground truth: loop() over (x, F, b, Q) against quadrature (LGConcatModel, d = 1, T = 6)"""
import numpy as np
import numpy.testing as npt
import pytest

from tests import dynamics_theta_cases as DC, dynamics_theta_np as NP

SHAPES, moments_within = DC.GAMMA_SHAPES, DC.moments_within

pytestmark = pytest.mark.gpu

# float32 states against the restatement on the same float32-rounded inputs; each bar is twice the worst error measured over every cell, rounded up.  The sums are
# formed in double from the float32 values, so the statistics and the posterior are as accurate as for float64 states: measured worst 4.6e-15 (statistics) and
# 3.0e-13 (posterior; float64 states: 3.8e-15 and 3.7e-13).  The draws are rounded to float32 on the way out: measured 0 -- every entry equal to the restatement's
# rounded to float32 -- so that bar is rounded up to 2^-24 of the largest entry, one float32 rounding step, the smallest error above 0 the comparison can show.
FP32_STATS_BAR = 1e-14
FP32_POST_BAR = 6e-13
FP32_DRAW_BAR = 2.0 ** -24


@pytest.fixture(scope="module")
def handle():
    from aux_ssm_samplers_amd import _lib
    return _lib.default_handle()


def _prior(p, chi_scale=1.0, **over):
    from aux_ssm_samplers_amd.loop import MNIWPrior
    q = dict(p, **over)
    return MNIWPrior(q["M0"], q["K0"], q["nu0"], q["Psi0"]).struct(chi_scale)


def _device_update(handle, p, x, dtype, chain_minor, chi, prior=None):
    """-> (stats, post, flags, F, b, Q) as host arrays for the chains x (C, T, d) with the cell's explicit noise"""
    from aux_ssm_samplers_amd.kalman.generic import DeviceChains
    C, T, d = x.shape
    n = d + 1
    chains = DeviceChains(handle, x, dtype, chain_minor=chain_minor)
    assert chains.chain_minor == chain_minor
    stats = handle.dynamics_stats(chains.x, chains.layout).to_host()
    rep = lambda a: handle.to_device(np.repeat(a[None], C, axis=0), dtype)
    F, b, Q = rep(p["F0"]), rep(p["b0"]), rep(p["Q0"])
    post = handle.zeros((C, d * n + n * n + 1 + d * d), np.float64)
    flags = handle.to_device(np.full(C, -1, np.int32))
    handle.dynamics_theta_update(chains.x, prior or _prior(p), handle.to_device(chi[:C], dtype), handle.to_device(p["ew"][:C], dtype),
                                 handle.to_device(p["ea"][:C], dtype), F.arr(d * d, 0, 0), b.arr(d, 0, 0), Q.arr(d * d, 0, 0), flags, post_out=post,
                                 layout=chains.layout)
    return stats, post.to_host(), flags.to_host(), F.to_host(), b.to_host(), Q.to_host()


@pytest.mark.parametrize("chain_minor", [False, True], ids=["dense", "chain_minor"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("d", DC.D_CASES)
def test_statistics_posterior_and_draws(handle, d, dtype, chain_minor):
    """tests 1 and 2 on every (T, C) of the cell list"""
    f32 = dtype == np.float32
    p = DC.problem(d, f32)
    sb, pb = DC.blocks(d)
    worst = dict(stats=0.0, post=0.0, draw=0.0)
    for T in DC.T_CASES:
        want_stats, want_post, want_Q, want_A = DC.reference(d, T, f32)
        chi = DC.chi_for(p, T, f32)
        for C in DC.C_CASES:
            stats, post, flags, F, b, Q = _device_update(handle, p, p["x"][:C, :T], dtype, chain_minor, chi)
            assert not flags.any(), (T, C, flags)
            for s in sb:
                worst["stats"] = max(worst["stats"], DC.rel(stats[:, s], want_stats[:C, s], 1))
            for s in pb:
                worst["post"] = max(worst["post"], DC.rel(post[:, s], want_post[:C, s], 1))
            A = np.concatenate([F, b[:, :, None]], axis=2)
            wQ, wA = (want_Q[:C].astype(dtype), want_A[:C].astype(dtype)) if f32 else (want_Q[:C], want_A[:C])
            worst["draw"] = max(worst["draw"], DC.rel(Q, wQ, (1, 2)), DC.rel(A, wA, (1, 2)))
            npt.assert_array_equal(Q, np.swapaxes(Q, 1, 2))
            assert Q.dtype == dtype and np.all(np.isfinite(Q)) and np.all(np.isfinite(A))
    print(f"dynamics_theta d={d} {np.dtype(dtype).name} {'chain-minor' if chain_minor else 'dense'}: worst relative error stats {worst['stats']:.2e} "
          f"post {worst['post']:.2e} draw {worst['draw']:.2e}")
    assert worst["stats"] <= (FP32_STATS_BAR if f32 else DC.FP64_BAR)
    assert worst["post"] <= (FP32_POST_BAR if f32 else DC.FP64_BAR)
    assert worst["draw"] <= (FP32_DRAW_BAR if f32 else DC.FP64_BAR)


@pytest.mark.parametrize("chain_minor", [False, True], ids=["dense", "chain_minor"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_a_chain_alone_is_the_chain_in_its_batch(handle, dtype, chain_minor):
    d, T = 4, 3 * DC.L + 38
    p = DC.problem(d, dtype == np.float32)
    chi = DC.chi_for(p, T, dtype == np.float32)
    batch = _device_update(handle, p, p["x"][:, :T], dtype, chain_minor, chi)
    for c in (0, 33, DC.C_MAX - 1):
        q = dict(p, ew=p["ew"][c:c + 1], ea=p["ea"][c:c + 1])
        alone = _device_update(handle, q, p["x"][c:c + 1, :T], dtype, chain_minor, chi[c:c + 1])
        for got, want in zip(alone, batch):
            npt.assert_array_equal(got[0], want[c])


@pytest.mark.parametrize("chain_minor", [False, True], ids=["dense", "chain_minor"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("d", [1, 4])
def test_a_degenerate_chain_keeps_its_parameters(handle, d, dtype, chain_minor):
    """chain 1 of 3 never moves; with a tiny Psi0 and a prior mean that reproduces the constant its Psi_n is rounding noise: flag 2, F / b / Q untouched, and the
    restatement says the same.  With a vanishing K0 as well, K_n has rank one: flag 1.  The other chains are drawn as usual."""
    p = DC.problem(d, dtype == np.float32)
    T = 40
    const = np.asarray(1.75 + np.arange(d), np.float64)
    x = p["x"][:3, :T].copy()
    x[1] = const
    M0 = np.concatenate([np.zeros((d, d)), const[:, None]], axis=1)
    chi = DC.chi_for(p, T, dtype == np.float32)
    for K0, want in ((np.eye(d + 1), 2), (1e-200 * np.eye(d + 1), 1)):
        over = dict(M0=M0, K0=K0, Psi0=1e-200 * np.eye(d))
        assert NP.step(x[1], M0, K0, p["nu0"], over["Psi0"], chi[1], p["ew"][1], p["ea"][1])[0] == want
        stats, post, flags, F, b, Q = _device_update(handle, p, x, dtype, chain_minor, chi, prior=_prior(p, **over))
        assert flags[1] == want
        npt.assert_array_equal(F[1], p["F0"].astype(dtype))
        npt.assert_array_equal(b[1], p["b0"].astype(dtype))
        npt.assert_array_equal(Q[1], p["Q0"].astype(dtype))
        for a in (post, F, b, Q):
            assert np.all(np.isfinite(a))
        if want == 2:
            assert flags[0] == 0 and flags[2] == 0 and not np.array_equal(F[0], p["F0"].astype(dtype))


def test_refusals_name_the_limit(handle):
    from aux_ssm_samplers_amd.kalman.generic import DeviceChains
    p = DC.problem(2)
    with pytest.raises(ValueError, match="T >= 2"):
        _device_update(handle, p, p["x"][:2, :1], np.float64, False, DC.chi_for(p, 2))
    bad = _prior(p)
    bad.nu0 = 0.5
    with pytest.raises(ValueError, match="nu0 > dx - 1"):
        _device_update(handle, p, p["x"][:2, :5], np.float64, False, DC.chi_for(p, 5), prior=bad)
    bad = _prior(p)
    bad.Psi0[0] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        _device_update(handle, p, p["x"][:2, :5], np.float64, False, DC.chi_for(p, 5), prior=bad)
    x5 = handle.zeros((2, 6, 5), np.float64)
    with pytest.raises(ValueError, match="dx <= 4"):
        handle.dynamics_stats(x5)
    with pytest.raises(ValueError, match="m <= 8"):
        handle.rng_gamma_into((1, 2), 0, [1.0] * 9, handle.zeros((9,), np.float64))
    with pytest.raises(ValueError, match="positive and finite"):
        handle.rng_gamma_into((1, 2), 0, [1.0, -2.0], handle.zeros((2,), np.float64))


def test_the_entry_points_refuse_before_anything_is_enqueued(handle):
    """the C ABI itself (handle.lib), past the host-side validation of MNIWPrior: NULL arguments, a prior that is not symmetric or not positive definite, and
    the launch limit of the chain-minor statistics pass -- each ERR_ARG with its reason, the outputs untouched"""
    import ctypes as C
    from aux_ssm_samplers_amd import _lib
    p = DC.problem(2)
    Cn, T, d, n = 3, 9, 2, 3
    lib, h = handle.lib, handle.h
    x = handle.to_device(p["x"][:Cn, :T])
    stats = handle.to_device(np.full((Cn, n * n + d * n + d * d), 7.0))
    chi, ew, ea = handle.to_device(DC.chi_for(p, T)[:Cn]), handle.to_device(p["ew"][:Cn]), handle.to_device(p["ea"][:Cn])
    rep = lambda a: handle.to_device(np.repeat(a[None], Cn, axis=0))
    F, b, Q = rep(p["F0"]), rep(p["b0"]), rep(p["Q0"])
    flags = handle.to_device(np.full(Cn, -1, np.int32))
    Fa, ba, Qa = F.arr(d * d, 0, 0), b.arr(d, 0, 0), Q.arr(d * d, 0, 0)

    def refused(rc, why):
        assert rc == _lib.ERR_ARG, rc
        assert why in lib.auxssm_last_error().decode(), lib.auxssm_last_error().decode()

    refused(lib.auxssm_dynamics_stats(h, _lib.F64, Cn, T, d, 0, None, stats.ptr), "x must be non-NULL")
    refused(lib.auxssm_dynamics_stats(h, _lib.F64, Cn, T, d, 0, x.ptr, None), "stats_out must be non-NULL")
    refused(lib.auxssm_dynamics_stats(h, _lib.F64, Cn, T, d, 7, x.ptr, stats.ptr), "layout must be")
    # more than 65535 blocks of 64 chains in the chain-minor pass (refused on the sizes alone: x is not read)
    refused(lib.auxssm_dynamics_stats(h, _lib.F64, 65535 * 64 + 1, 2, 1, _lib.LAYOUT_CHAIN_MINOR, x.ptr, stats.ptr), "C <= 4194240")

    def update(prior=None, chi_=chi, F_=Fa, flags_=flags, null_prior=False, **kw):
        pr = prior or _prior(p)
        return lib.auxssm_dynamics_theta_update(h, _lib.F64, Cn, T, d, 0, x.ptr, None if null_prior else C.byref(pr), chi_.ptr if chi_ is not None else None,
                                                ew.ptr, ea.ptr, C.byref(F_) if F_ is not None else None, C.byref(ba), C.byref(Qa), None,
                                                flags_.ptr if flags_ is not None else None)

    refused(update(null_prior=True), "must be non-NULL")
    refused(update(chi_=None), "must be non-NULL")
    refused(update(F_=None), "must be non-NULL")
    refused(update(flags_=None), "must be non-NULL")
    refused(update(F_=F.arr(d * d, 1, 0)), "time strides of F, b and Q must be 0")
    refused(update(F_=F.arr(0, 0, 0)), "every chain needs its own F, b, Q")
    skew = _prior(p)
    skew.K0[1] += 0.25                       # K0[0, 1] != K0[1, 0]
    refused(update(prior=skew), "must be symmetric")
    indef = _prior(p)
    indef.Psi0[0], indef.Psi0[1], indef.Psi0[2], indef.Psi0[3] = 1.0, 2.0, 2.0, 1.0
    refused(update(prior=indef), "must be positive definite")
    scale = _prior(p)
    scale.chi_scale = 0.0
    refused(update(prior=scale), "chi_scale must be positive")
    handle.sync()
    npt.assert_array_equal(stats.to_host(), 7.0)
    npt.assert_array_equal(flags.to_host(), -1)
    npt.assert_array_equal(F.to_host(), np.repeat(p["F0"][None], Cn, axis=0))
    assert update() == 0 and not flags.to_host().any()     # (and the same call with nothing wrong goes through)


def test_a_sweep_refuses_another_chain_count_after_the_step(handle):
    """the step made the model's dynamics per-chain for 3 chains: a sweep of that model with 5 chains (resident, or a host state) would read past the end of the
    (3, d, d) / (3, d) buffers -- refused with the reason, before any launch; 3 chains still sweep"""
    from aux_ssm_samplers_amd.kalman import get_kernel
    from aux_ssm_samplers_amd.kalman.generic import DeviceChains
    from aux_ssm_samplers_amd.loop import DynamicsThetaStep, MNIWPrior
    T, d = 30, 2
    p = DC.problem(d)
    model, m = _lg_model(T, d)
    init, kernel = get_kernel(model.dynamics_factory, model.observations_factory, model.log_likelihood_fn, True)
    three = DeviceChains(handle, p["x"][:3, :T], np.float64, chain_minor=False)
    DynamicsThetaStep(model, MNIWPrior(p["M0"], p["K0"], p["nu0"], p["Psi0"]))(np.array([1, 2], np.uint32), three)
    five = DeviceChains(handle, p["x"][:5, :T], np.float64, chain_minor=False)
    before = five.to_host()
    key = np.array([5, 6], np.uint32)
    with pytest.raises(ValueError, match="per-chain dynamics .* of 3 chains .* the chains are 5"):
        kernel(key, init(five), 0.5)
    with pytest.raises(ValueError, match="per-chain dynamics .* of 3 chains .* the chains are 5"):
        kernel(key, init(p["x"][:5, :T]), 0.5)
    with pytest.raises(ValueError, match="per-chain dynamics .* of 3 chains .* the chains are 1"):
        kernel(key, init(p["x"][0, :T]), 0.5)
    npt.assert_array_equal(five.to_host(), before)
    kernel(key, init(three), 0.5)
    assert np.all(np.isfinite(three.to_host()))


# ---- 3. the gamma generator ------------------------------------------------------------------------------------------------------------
def _safe_key(stream, n):
    """a key on which no acceptance decision of the restatement lies within 1e-9 of its threshold (chosen on the CPU), and the restatement's draws"""
    for k0 in range(20):
        key = (1000 + k0, 77)
        want, margin = NP.gamma(key, stream, n, SHAPES, with_margin=True)
        if margin > 1e-9:
            return key, want
    raise AssertionError("no key with a safe margin")


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_gamma_against_the_restatement(handle, dtype):
    n, stream = 4099, 3          # (not a multiple of the workgroup; every one of the n x 5 draws is compared)
    key, want = _safe_key(stream, n)
    out = handle.zeros((n, len(SHAPES)), dtype)
    handle.rng_gamma_into(key, stream, SHAPES, out)
    got = out.to_host()
    assert np.all(np.isfinite(got))
    if dtype == np.float64:
        err = float(np.max(np.abs(got - want) / want))
        print(f"gamma f64: worst relative error {err:.2e}")
        assert err <= 1e-10
    else:   # the double value rounded to float32: half an ulp of float32 beside the 1e-10
        npt.assert_allclose(got, want, rtol=2.0 ** -24 + 1e-10)


def test_gamma_eight_shapes_is_a_function_of_the_flat_index(handle):
    shapes = [0.05, 0.5, 1.0, 1.5, 4.0, 30.0, 1e3, 1e6]
    key = (5, 6)
    out = handle.zeros((37, 8), np.float64)
    handle.rng_gamma_into(key, 0, shapes, out)
    got = out.to_host()
    npt.assert_allclose(got, NP.gamma(key, 0, 37, shapes), rtol=1e-10)
    again = handle.zeros((5, 8), np.float64)
    handle.rng_gamma_into(key, 0, shapes, again)
    npt.assert_array_equal(again.to_host(), got[:5])


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_gamma_moments_on_the_device(handle, dtype):
    out = handle.zeros((60_000, len(SHAPES)), dtype)
    handle.rng_gamma_into((99, 100), 1, SHAPES, out)
    g = out.to_host().astype(np.float64)
    assert np.all(np.isfinite(g)) and np.all(g > 0)
    for i, a in enumerate(SHAPES):
        ok, info = moments_within(g[:, i], a)
        assert ok, (a, info)


# ---- 4. moments of the step -------------------------------------------------------------------------------------------------------------
def _lg_model(T, d, seed=0):
    from aux_ssm_samplers_amd.workloads import lg_model
    from aux_ssm_samplers_amd.kalman import LGConcatModel
    m = lg_model(T, d, seed) if seed else lg_model(T, d)
    bt = np.broadcast_to
    model = LGConcatModel(m["m0"], m["P0"], bt(m["F"], (T - 1, d, d)), bt(m["Q"], (T - 1, d, d)), bt(m["b"], (T - 1, d)), bt(m["Hobs"], (T, d, d)),
                          bt(m["Robs"], (T, d, d)), bt(m["cobs"], (T, d)), m["y"])
    return model, m


@pytest.mark.parametrize("chain_minor", [False, True], ids=["dense", "chain_minor"])
def test_one_keyed_call_has_the_posterior_means(handle, chain_minor):
    from aux_ssm_samplers_amd.kalman.generic import DeviceChains
    from aux_ssm_samplers_amd.loop import DynamicsThetaStep, MNIWPrior
    N, T, d = 4096, 50, 3
    p = DC.problem(d)
    model, m = _lg_model(T, d)
    x = p["x"][0, :T]
    chains = DeviceChains(handle, np.broadcast_to(x, (N, T, d)), np.float64, chain_minor=chain_minor)
    step = DynamicsThetaStep(model, MNIWPrior(p["M0"], p["K0"], p["nu0"], p["Psi0"]))
    step(np.array([11, 12], np.uint32), chains)
    assert not step.flags(chains).any()
    F, b, Q = step.params(chains)
    Mn, Kn, nun, Psi = NP.posterior(NP.stats(x), T - 1, p["M0"], p["K0"], p["nu0"], p["Psi0"])
    A = np.concatenate([F, b[:, :, None]], axis=2)
    for got, want in ((A, Mn), (Q, Psi / (nun - d - 1))):
        se = got.std(axis=0, ddof=1) / np.sqrt(N)
        z = np.abs(got.mean(axis=0) - want) / se
        assert np.all(z <= 5), z.max()
    npt.assert_array_equal(Q, np.swapaxes(Q, 1, 2))
    with pytest.raises(ValueError, match="per-chain parameters of 4096 chains"):
        step(np.array([1, 2], np.uint32), DeviceChains(handle, np.broadcast_to(x, (3, T, d)), np.float64, chain_minor=False))


# ---- 5. the sweep behind the step ---------------------------------------------------------------------------------------------------------
def _sweep_models():
    """name -> (builder(order) -> (model, path (T, d), delta), orders, dense only)"""
    from tests import kalman_logistic_cases as LG, kalman_poisson_cases as PC, kalman_poisson_lin_cases as PL, kalman_logistic_lin_cases as LL
    T, d = 40, 2

    def lg(order):
        model, m = _lg_model(T, d)
        return model, m["x_true"], 0.5

    def sv(order):
        from aux_ssm_samplers_amd.kalman import SVModel
        rng = np.random.default_rng(3)
        F, Q, b = 0.9 * np.eye(d), 0.1 * np.eye(d) + 0.02, np.array([0.05, -0.05])
        x = np.zeros((T, d))
        for t in range(1, T):
            x[t] = F @ x[t - 1] + b + np.linalg.cholesky(Q) @ rng.standard_normal(d)
        y = np.exp(0.5 * x) * rng.standard_normal((T, d))
        return SVModel(y, np.zeros(d), np.eye(d), F, Q, b, order=order), x, 0.1

    def poisson(order):
        cell = PC._build(d, T, 1, order, 0)
        return cell["model"], cell["x"][0], cell["delta"]

    def logistic(family):
        def f(order):
            cell = LG._build(family, d, T, 1, order, 0)
            return cell["model"], cell["x"][0], cell["delta"]
        return f

    def plin(order):
        cell = PL._build(d, 3, T, 1, order, 0)
        return cell["model"], cell["x"][0], cell["delta"]

    def llin(family):
        def f(order):
            cell = LL._build(family, d, 3, T, 1, order, 0)
            return cell["model"], cell["x"][0], cell["delta"]
        return f

    return {"LGConcatModel": (lg, (1,), False), "SVModel": (sv, (1, 2), False), "PoissonModel": (poisson, (1, 2), False),
            "BinomialModel": (logistic("binomial"), (1, 2), False), "NegBinomialModel": (logistic("negbinomial"), (1, 2), False),
            "PoissonLinearModel": (plin, (1, 2), True), "BinomialLinearModel": (llin("binomial"), (1, 2), True),
            "NegBinomialLinearModel": (llin("negbinomial"), (1, 2), True)}


SWEEP_CELLS = [(name, order, cm) for name, orders, dense_only in
               [("LGConcatModel", (1,), False), ("SVModel", (1, 2), False), ("PoissonModel", (1, 2), False), ("BinomialModel", (1, 2), False),
                ("NegBinomialModel", (1, 2), False), ("PoissonLinearModel", (1, 2), True), ("BinomialLinearModel", (1, 2), True),
                ("NegBinomialLinearModel", (1, 2), True)]
               for order in orders for cm in ((False,) if dense_only else (False, True))]


@pytest.mark.parametrize("name,order,chain_minor", SWEEP_CELLS, ids=[f"{n}-o{o}-{'cm' if c else 'dense'}" for n, o, c in SWEEP_CELLS])
def test_the_sweep_reads_per_chain_dynamics(handle, name, order, chain_minor):
    """after one step, an explicit-noise sweep of the C chains = a one-chain sweep of a fresh model built from step.params(chains)[c], chain by chain"""
    from aux_ssm_samplers_amd.kalman import get_kernel
    from aux_ssm_samplers_amd.kalman.generic import DeviceChains
    from aux_ssm_samplers_amd.loop import DynamicsThetaStep, MNIWPrior
    build = _sweep_models()[name][0]
    model, path, delta = build(order)
    model = DC.with_dynamics(model, *(np.asarray(a)[0] for a in (model.Fs, model.Qs, model.bs)))   # (the cell's model may be cached: no device state of another test)
    T, d = path.shape
    C = 34 if chain_minor else 3
    rng = np.random.default_rng(17)
    x = path[None] + 0.05 * rng.standard_normal((C, T, d))
    noise = dict(eps_aux=rng.standard_normal((C, T, d)), eps_samp=rng.standard_normal((C, T, d)), u_accept=np.full(C, 0.5))
    F0, Q0, b0 = (np.asarray(a)[0] for a in (model.Fs, model.Qs, model.bs))
    prior = MNIWPrior(np.concatenate([F0, b0[:, None]], axis=1), 50.0 * np.eye(d + 1), d + 60.0, 60.0 * Q0)   # (keeps the draws near the cell's dynamics)
    init, kernel = get_kernel(model.dynamics_factory, model.observations_factory, model.log_likelihood_fn, True)
    chains = DeviceChains(handle, x, np.float64, chain_minor=chain_minor)
    step = DynamicsThetaStep(model, prior)
    step(np.array([3, 4], np.uint32), chains)
    assert not step.flags(chains).any()
    Fc, bc, Qc = step.params(chains)
    assert np.ptp(Fc, axis=0).max() > 0        # (the chains really hold different parameters)
    kernel(None, init(chains), delta, noise=noise)
    got_x, got_la = chains.to_host(), chains.logs.to_host()[:, 0]
    worst = 0.0
    for c in range(C):
        fresh = DC.with_dynamics(model, Fc[c], Qc[c], bc[c])
        i1, k1 = get_kernel(fresh.dynamics_factory, fresh.observations_factory, fresh.log_likelihood_fn, True)
        one = DeviceChains(handle, x[c:c + 1], np.float64, chain_minor=False)
        k1(None, i1(one), delta, noise={k: v[c:c + 1] for k, v in noise.items()})
        want_x, want_la = one.to_host()[0], one.logs.to_host()[0, 0]
        worst = max(worst, float(np.max(np.abs(got_x[c] - want_x)) / np.max(np.abs(want_x))), abs(got_la[c] - want_la) / max(1.0, abs(want_la)))
    print(f"sweep behind the step {name} order {order} {'chain-minor' if chain_minor else 'dense'}: worst error {worst:.2e}")
    assert worst <= DC.FP64_BAR


# ---- 6. joint ground truth ---------------------------------------------------------------------------------------------------------------
def test_gibbs_over_state_and_dynamics_matches_quadrature(handle):
    """LGConcatModel, d = 1, T = 6, 2048 independent chains, loop() with the step: the posterior means of F, b, log Q, x_0 and x_5 against quadrature over
    (F, b, log Q) with the state integrated out by a NumPy Kalman filter / smoother.  Standard errors from the spread of the per-chain averages; 5 of them.
    The grid: halving it moves every mean by less than a tenth of that bar."""
    from aux_ssm_samplers_amd.kalman import LGConcatModel, get_kernel
    from aux_ssm_samplers_amd.kalman.generic import DeviceChains
    from aux_ssm_samplers_amd.loop import DynamicsThetaStep, MNIWPrior, loop
    j = DC.joint_model()
    T, C, burn, keep = j["T"], 2048, 150, 250
    bt = np.broadcast_to
    one = lambda v, shape: bt(np.array(v, np.float64).reshape(shape[1:]), shape)
    model = LGConcatModel(np.array([j["m0"]]), np.array([[j["P0"]]]), one(j["F"], (T - 1, 1, 1)), one(j["Q"], (T - 1, 1, 1)), one(j["b"], (T - 1, 1)),
                          one(1.0, (T, 1, 1)), one(j["R"], (T, 1, 1)), one(0.0, (T, 1)), j["y"][:, None])
    init, kernel = get_kernel(model.dynamics_factory, model.observations_factory, model.log_likelihood_fn, True)
    rng = np.random.default_rng(8)
    chains = DeviceChains(handle, j["y"][None, :, None] + 0.3 * rng.standard_normal((C, T, 1)), np.float64)
    step = DynamicsThetaStep(model, MNIWPrior(j["M0"], j["K0"], j["nu0"], j["Psi0"]))
    acc = np.zeros((C, 5))
    flagged = [0]

    def collect(i, state):
        if i < burn:
            return
        F, b, Q = step.params(chains)
        x = chains.to_host()
        acc[:, 0] += F[:, 0, 0]
        acc[:, 1] += b[:, 0]
        acc[:, 2] += np.log(Q[:, 0, 0])
        acc[:, 3] += x[:, 0, 0]
        acc[:, 4] += x[:, T - 1, 0]
        flagged[0] += int(step.flags(chains).any())

    loop(np.array([21, 22], np.uint32), 1.5, init(chains), kernel, None, burn + keep, theta_step=step, callback=collect)
    assert flagged[0] == 0
    per_chain = acc / keep
    mean, se = per_chain.mean(axis=0), per_chain.std(axis=0, ddof=1) / np.sqrt(C)
    fine, coarse = DC.joint_quadrature(j, 160), DC.joint_quadrature(j, 80)
    z = np.abs(mean - fine) / se
    print("joint ground truth (F, b, log Q, x_0, x_5): chains", mean, "quadrature", fine, "se", se, "z", z, "grid halving moves", np.abs(fine - coarse))
    assert np.all(np.abs(fine - coarse) <= 0.1 * 5 * se), np.abs(fine - coarse) / se
    assert np.all(z <= 5), z
