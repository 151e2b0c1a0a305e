#!/usr/bin/env python3
"""Secondary measurements on the BASELINE configs that are not the headline (bench.py measures C2 and, with --workload csmc, C3):
   C3k  stochastic volatility d=1 T=65536, auxiliary-Kalman sweep (first / second order), fp64
   C4   Lorenz-63 T=16384 dt=1.25e-4 obs every 80 steps, fp32: Kalman sweep (extended linearisation) + cSMC sweep N=512 (bootstrap, backward sampling)
   C5   dense d = p = 64 T=8192 fp32: filter + sampler + joint log-density of one chain (wide-state path)
   guided  guided proposals beside the independent ones: C3's shape and the reference's SV protocol (D = 30, N = 25), 256 chains
   spatial  the spatial example on the 5 x 5 grid (dx = 25, T = 1024, N = 25, multivariate Student-t potential) beside the SV potential at the same shape, 256 chains
   lingauss  a partially observed linear-Gaussian model (dx = 24, dy = 12, T = 1024, N = 25, linear-Gaussian observation potential) beside GaussianObsPotential
             at the same shape, 256 chains
   poisson  multivariate counts with a log link (Poisson potential) beside SVPotential at the SV protocol's shape (D = 30, T = 250, N = 25, fp32), 1 / 16 / 256
             chains: independent, gradient, guided and parallel-in-time sweeps
   logistic  binomial data with a logit link (logistic potential) beside PoissonPotential at the SV protocol's shape (D = 30, T = 250, N = 25, fp32), 1 / 16 / 256
             chains: independent, gradient, guided and parallel-in-time sweeps
   spatial_kalman  the spatial example's default sampler: the auxiliary Kalman sampler on the batched 8 x 8 model (d = 64, T = 1024, nu = 1, fp32, both orders), device
             sweep at 1 / 16 / 256 chains beside the host-factory path
   poisson_kalman  count data under the auxiliary Kalman sampler (kalman.PoissonModel, fp32, both orders) at T = 250, dx = 30 and T = 16384, dx = 1, 1 / 64 / 256 /
             1024 chains, beside SVModel at the same shapes, the host-factory path and the Poisson cSMC sweep
   logistic_kalman  binomial and negative-binomial data under the auxiliary Kalman sampler (kalman.BinomialModel / NegBinomialModel, fp32) at T = 16384, dx = 1 (both
             orders) and T = 250, dx = 30 (first order), 1 / 64 / 256 / 1024 chains, beside PoissonModel at the same shapes and the host-factory path
   poisson_lin_kalman  Poisson counts through a loading matrix under the auxiliary Kalman sampler (kalman.PoissonLinearModel, T = 16384, dx = 4, dy = 128, fp32, both
             orders) at 1 / 64 / 256 dense resident chains, beside kalman.PoissonModel at T = 16384, dx = 4 on dense chains and the host-factory path of the new
             model; then the library's kernel-group times of one sweep.  poisson_lin_trace: a few sweeps alone, for a kernel trace taken from outside
   logistic_lin_kalman  binomial / negative-binomial channels through a loading matrix (kalman.BinomialLinearModel / NegBinomialLinearModel), poisson_lin_kalman's
             shape and protocol, beside PoissonLinearModel in the same process; then the library's kernel-group times of one sweep of either new model
   pit30  the reference's SV experiment at its defaults (--parallel, D = 30, N = 25, T = 250): the parallel-in-time sweep beside the sequential wide sweep, 1 / 16 / 256 chains
   smoother  the RTS smoother (auxssm_kalman_smooth) beside the pathwise sampler (auxssm_kalman_sample) on the same resident filtered moments: C2's model at
             T = 65536, d = 4, fp64, 1 and 256 sequences, and T = 16384, d = 3, fp32, 64 sequences; parallel scan, at one sequence also the sequential recursion
   observation_theta  the conjugate step on (H, c, R) (loop.ObservationThetaStep) beside one keyed sweep of the same LGConcatModel with a per-chain observation
                   model, the statistics entry alone in both layouts, auxssm_dynamics_stats on the same state and a device copy: dynamics_theta's four rows
   dynamics_theta  the conjugate step on (F, b, Q) (loop.DynamicsThetaStep) beside one keyed sweep of the same LGConcatModel with per-chain parameters: C2's shape
             (T = 65536, d = 4, fp64) at 1 / 16 / 256 chains and T = 16384, d = 1, fp32 at 1024 chains; the statistics pass alone as bytes/s beside a device copy
   csmc_theta  per-chain dynamics in the sequential cSMC sweep (particle Gibbs over (x, F, b, Q)): the chain-shared, per-chain and time-varying sweeps of the same
             values in one process, then loop.DynamicsThetaStep + auxssm_csmc_dynamics_commit on the CsmcChains: C3's shape and SV d = 4, N = 64, 256 chains, fp32
   em   one EM iteration of a time-invariant LGSSM (_primitives.kalman.fit_em's four calls: filter, smoother, auxssm_kalman_smooth_stats, auxssm_lgssm_em_mstep)
             beside the statistics entry alone, filter + smoother alone and a device copy of the bytes the statistics pass reads: C2's shape (T = 65536, dx = dy = 4,
             fp64) at 1 and 16 sequences, and T = 16384, d = 1, fp32 at 64 sequences
   loop the MCMC loop around the sweeps (aux_ssm_samplers_amd.loop: running moments, acceptance averages, adaptation, Lorenz theta step) on C2 / C3 / C4
Prints one JSON line per measurement.  Inputs are resident in HBM (DeviceChains) where the API allows it; device Threefry noise."""
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from aux_ssm_samplers_amd import _lib, random as R  # noqa: E402
from aux_ssm_samplers_amd.kalman import get_kernel, SVModel, LorenzModel  # noqa: E402
from aux_ssm_samplers_amd.kalman.generic import DeviceChains, KalmanSampler  # noqa: E402


def timed_sweeps(kernel, chains, delta, steps=5, warmup=2, seed=1):
    h = chains.handle
    state = KalmanSampler(x=chains, updated=None)
    keys = R.split(R.PRNGKey(seed), steps + warmup)
    for k in range(warmup):
        kernel(keys[k], state, delta)
    h.sync()
    t0 = time.perf_counter()
    for k in range(steps):
        kernel(keys[warmup + k], state, delta)
    h.sync()
    el = time.perf_counter() - t0
    return chains.C * steps / el, el / steps * 1e3, float(chains.accepted.to_host().mean())


def c3_kalman(order, chains=64, T=65536, chain_minor=None):
    from aux_ssm_samplers_amd.workloads import sv_setup
    from aux_ssm_samplers_amd.common import delta_adaptation
    from aux_ssm_samplers_amd.loop import loop
    y, xtrue, (m0, P0, F, Q, b) = sv_setup(T, 1, rho=0.0)
    model = SVModel(y, m0, P0, F, Q, b, order=order)
    init, kernel = get_kernel(model.dynamics_factory, model.observations_factory, model.log_likelihood_fn, True)
    h = _lib.default_handle()
    ch = DeviceChains(h, np.repeat(xtrue[None], chains, axis=0), chain_minor=chain_minor)
    # burn-in with the reference's adaptation rule so that the timed sweeps run at a step size that moves (target 0.234)
    out = loop(R.PRNGKey(0), 0.05, KalmanSampler(x=ch, updated=True), kernel, delta_adaptation, 400, target_alpha=0.234, lr=0.3, beta=0.2)
    delta = out[3]
    v, ms, acc = timed_sweeps(kernel, ch, delta, steps=10)
    print(json.dumps(dict(config=f"C3 SV d=1 T={T}, aux-Kalman order {order}, fp64, {'chain-minor' if ch.chain_minor else 'dense'} layout", chains=chains,
                          delta=float(f"{delta:.3g}"), sweeps_per_s=round(v, 1), ms_per_step=round(ms, 2), accept=acc)), flush=True)


def c4(chains=8, T=16384, N=512):
    from aux_ssm_samplers_amd.workloads import lorenz_kalman_setup
    from aux_ssm_samplers_amd.workloads import lorenz_setup
    from aux_ssm_samplers_amd.csmc import _device
    model, xtrue = lorenz_kalman_setup(T, every=80, dt=1.25e-4)
    init, kernel = get_kernel(model.dynamics_factory, model.observations_factory, model.log_likelihood_fn, True)
    h = _lib.default_handle()
    ch = DeviceChains(h, np.repeat(xtrue[None], chains, axis=0).astype(np.float32), chain_minor=False)
    v, ms, acc = timed_sweeps(kernel, ch, 1e-4)
    print(json.dumps(dict(config=f"C4 Lorenz-63 T={T} dt=1.25e-4 obs/80, aux-Kalman (extended linearisation), fp32", chains=chains,
                          sweeps_per_s=round(v, 1), ms_per_step=round(ms, 2), accept=acc)))
    from aux_ssm_samplers_amd.csmc import CsmcChains, CSMCState
    from aux_ssm_samplers_amd._primitives.csmc import get_kernel as get_csmc_kernel
    M0, Mt, G0, Gt, xt, y, sig_y = lorenz_setup(T, every=80, dt=1.25e-4)
    init, ck = get_csmc_kernel(M0, G0, Mt, Gt, N, backward=True, Pt=Mt)
    cc = CsmcChains(h, np.repeat(xt[None], chains, axis=0).astype(np.float32))
    st = CSMCState(x=cc, updated=None)
    ck(0, st)
    h.sync()
    t0 = time.perf_counter()
    reps = 3
    for k in range(reps):
        ck(1 + k, st)
    h.sync()
    el = time.perf_counter() - t0
    print(json.dumps(dict(config=f"C4 Lorenz-63 T={T}, cSMC N={N} bootstrap + backward sampling, fp32, resident chains", chains=chains,
                          sweeps_per_s=round(chains * reps / el, 1), ms_per_step=round(el / reps * 1e3, 2),
                          updated=float((cc.ancestors.to_host() != 0).mean()))))


def c5(T=8192):
    from aux_ssm_samplers_amd.workloads import c5_model
    import aux_ssm_samplers_amd._primitives.kalman as P
    u, lg64, x = c5_model(T, 64)
    lg = P.LGSSM(*[np.ascontiguousarray(a, np.float32) for a in lg64])
    u = u.astype(np.float32)
    h = _lib.default_handle()
    eps = np.random.default_rng(0).standard_normal((T, 64)).astype(np.float32)
    for rep in range(2):
        for kid, name in ((_lib.K_FILTER_INIT, "init"), (_lib.K_FILTER_SCAN, "scan (incl. log-likelihood)")):
            h.prof_enable(kid, 4)
            ms, Ps, ell = P.filtering(u, lg, True)
            n, t = h.prof_read()
            h.prof_disable()
            if rep:
                print(json.dumps(dict(config=f"C5 dense d=p=64 T={T} fp32, 1 chain, filter {name} kernels", ms=round(t, 2))))
        for kid, name in ((_lib.K_SAMPLE_INIT, "sampler init"), (_lib.K_SAMPLE_SCAN, "sampler scan")):
            h.prof_enable(kid, 4)
            xs = P.sampling(None, ms, Ps, lg, True, eps=eps)
            n, t = h.prof_read()
            h.prof_disable()
            if rep:
                print(json.dumps(dict(config=f"C5 dense d=p=64 T={T} fp32, 1 chain, {name} kernels", ms=round(t, 2))))
        h.prof_enable(_lib.K_LOGPDF, 4)
        lp = P.posterior_logpdf(u, xs, ell, lg)
        n, t = h.prof_read()
        h.prof_disable()
        if rep:
            print(json.dumps(dict(config=f"C5 dense d=p=64 T={T} fp32, 1 chain, joint log-density kernel", ms=round(t, 2), lp=float(lp))))


def timed_loop(label, kernel, state, delta, n_iter=40, **kw):
    """loop() twice (first run warms code objects and the workspace); wall time of the second, host-synchronised at the end only"""
    from aux_ssm_samplers_amd.loop import loop
    chains = state.x
    h = chains.handle
    delta_fn = kw.pop("delta_fn", None)
    for rep in range(2):
        out = None  # frees the previous run's moment arrays outside the timed region
        h.sync()
        t0 = time.perf_counter()
        out = loop(R.PRNGKey(5 + rep), delta, state, kernel, delta_fn, n_iter, **kw)
        h.sync()
        el = time.perf_counter() - t0
    print(json.dumps(dict(config=label, chains=chains.C, sweeps_per_s=round(chains.C * n_iter / el, 1), ms_per_step=round(el / n_iter * 1e3, 3),
                          avg_accept=round(float(out[5].to_host().mean()), 3))))
    return out


def loops():
    import bench
    from aux_ssm_samplers_amd.common import delta_adaptation
    from aux_ssm_samplers_amd.loop import LorenzThetaStep
    h = _lib.default_handle()
    # C2: 256 chains, chain-minor, chain-shared model
    T, d, C = 65536, 4, 256
    m, model = bench.build_model(T, d, np.float64)
    init, kernel = get_kernel(model.dynamics_factory, model.observations_factory, model.log_likelihood_fn, True)
    x0 = m["x_true"][None] + 0.3 * np.random.default_rng(0).standard_normal((C, T, d))
    ch = DeviceChains(h, x0)
    v, ms, acc = timed_sweeps(kernel, ch, 0.5, steps=20, warmup=3)
    print(json.dumps(dict(config="C2 LG-SSM T=65536 d=4 fp64, bare sweeps (no statistics)", chains=C, sweeps_per_s=round(v, 1), ms_per_step=round(ms, 3))))
    timed_loop("C2 LG-SSM T=65536 d=4 fp64, loop(): sweeps + running sq-jump/mean/sq-mean + acceptance averages, no host sync", kernel,
               KalmanSampler(x=ch, updated=True), 0.5, beta=0.01)
    timed_loop("C2 ..., loop() while adapting delta (one 2 KB read-back per sweep)", kernel, KalmanSampler(x=ch, updated=True), 0.5, beta=0.01,
               delta_fn=delta_adaptation, target_alpha=0.5, lr=0.1)
    del ch
    # C4: the (x, theta) Gibbs sampler of the Lorenz example, 8 chains each with its own theta
    from aux_ssm_samplers_amd.workloads import lorenz_kalman_setup
    from aux_ssm_samplers_amd.workloads import lorenz_setup
    T, C = 16384, 8
    model, xtrue = lorenz_kalman_setup(T, every=80, dt=1.25e-4)
    init, kernel = get_kernel(model.dynamics_factory, model.observations_factory, model.log_likelihood_fn, True)
    ch = DeviceChains(h, np.repeat(xtrue[None], C, axis=0).astype(np.float32), chain_minor=False)
    v, ms, acc = timed_sweeps(kernel, ch, 1e-4, steps=20, warmup=3)
    print(json.dumps(dict(config="C4 Lorenz-63 T=16384 fp32, bare Kalman sweeps", chains=C, sweeps_per_s=round(v, 1), ms_per_step=round(ms, 3))))
    step = LorenzThetaStep(model, 1e3 ** 0.5)  # sigma_theta of examples/lorenz/experiment.py:75
    timed_loop("C4 Lorenz-63 T=16384 fp32, loop(): Kalman sweep + theta | x draw per chain + running statistics, no host sync", kernel,
               KalmanSampler(x=ch, updated=True), 1e-4, beta=0.01, theta_step=step)
    print(json.dumps(dict(theta_after=np.round(step.theta(ch), 3).tolist())))
    # C3 / C4 cSMC on resident chains
    from aux_ssm_samplers_amd.csmc import CsmcChains, CSMCState, get_independent_kernel, GaussianInit, LinearGaussianDynamics, SVPotential
    from aux_ssm_samplers_amd._primitives.csmc import get_kernel as get_csmc_kernel
    M0, Mt, G0, Gt, xt, y, sig_y = lorenz_setup(T, every=80, dt=1.25e-4)
    init, ck = get_csmc_kernel(M0, G0, Mt, Gt, 512, backward=True, Pt=Mt)
    cc = CsmcChains(h, np.repeat(xt[None], C, axis=0).astype(np.float32))
    timed_loop("C4 Lorenz-63 T=16384 fp32, loop(): cSMC N=512 bootstrap + backward sampling + per-step statistics, resident chains", lambda k, s, dl: ck(k, s),
               CSMCState(x=cc, updated=np.ones(T, bool)), None, n_iter=4, beta=0.01)
    T3, C3 = 65536, 16
    phi, q, xsv, ysv = bench.sv_data(T3, 0)
    M0 = GaussianInit(m0=[0.0], P0=[[q]])
    Mt = LinearGaussianDynamics(F=[[phi]], b=[0.0], Q=[[q]])
    init, ik = get_independent_kernel(M0, SVPotential(y=ysv[0]), Mt, SVPotential(params=ysv[1:]), 1024, backward=True, Pt=Mt)
    cc = CsmcChains(h, np.repeat(xsv.reshape(1, T3, 1), C3, axis=0).astype(np.float32))
    timed_loop("C3 SV T=65536 fp32, loop(): aux-cSMC N=1024 backward sampling + per-step statistics + per-step delta adaptation on device", ik,
               CSMCState(x=cc, updated=np.zeros(T3, bool)), 0.5, n_iter=4, beta=0.01, delta_fn=delta_adaptation, target_alpha=0.5, lr=0.1)


def pit(T=65536):
    """C3's model (SV, d = 1, T = 65536, fp32): parallel-in-time cSMC (auxssm_csmc_pit_sweep) vs the sequential sweep at the same N,
    few chains (where the sequential sweep is latency-bound: T dependent steps)"""
    import bench
    from aux_ssm_samplers_amd.csmc import CsmcChains, CSMCState, get_independent_kernel, GaussianInit, LinearGaussianDynamics, SVPotential
    h = _lib.default_handle()
    phi, q, xsv, ysv = bench.sv_data(T, 0)
    M0 = GaussianInit(m0=[0.0], P0=[[q]])
    Mt = LinearGaussianDynamics(F=[[phi]], b=[0.0], Q=[[q]])
    for N, chains in ((32, 1), (32, 16), (64, 1), (64, 16), (256, 1), (256, 8), (1024, 1), (1024, 4)):
        row = dict(config=f"C3 SV T={T} fp32, N={N}", chains=chains)
        for par in (True, False):
            init, k = get_independent_kernel(M0, SVPotential(y=ysv[0]), Mt, SVPotential(params=ysv[1:]), N, backward=not par, Pt=Mt, parallel=par)
            cc = CsmcChains(h, np.repeat(xsv.reshape(1, T, 1), chains, axis=0).astype(np.float32), delta=0.5)
            st = CSMCState(x=cc, updated=None)
            keys = R.split(R.PRNGKey(3), 8)
            k(keys[0], st, None)
            h.sync()
            reps = 5 if par else 2
            t0 = time.perf_counter()
            for i in range(reps):
                k(keys[1 + i], st, None)
            h.sync()
            el = (time.perf_counter() - t0) / reps
            name = "pit" if par else "sequential_backward_sampling"
            row[name + "_ms_per_sweep"] = round(el * 1e3, 2)
            row[name + "_updated"] = round(float((cc.ancestors.to_host() != 0).mean()), 3)
        row["speedup"] = round(row["sequential_backward_sampling_ms_per_sweep"] / row["pit_ms_per_sweep"], 1)
        print(json.dumps(row), flush=True)


def pit30(T=250, D=30, N=25):
    """the reference's stochastic-volatility experiment at its defaults (--parallel --D 30 --N 25: examples/stochastic_volatility/experiment.py:20-22), fp32,
    Threefry: the parallel-in-time sweep (csrc/pit_wide.hip) beside the sequential wide sweep with backward sampling (csrc/csmc_wide.hip), same run, at 1, 16 and
    256 chains.  Timing as the `pit` leg: wall time around several sweeps, ending in a device synchronise."""
    from aux_ssm_samplers_amd.workloads import sv_setup
    from aux_ssm_samplers_amd.csmc import CsmcChains, CSMCState, get_independent_kernel, GaussianInit, LinearGaussianDynamics, SVPotential
    h = _lib.default_handle()
    y, xtrue, (m0, P0, F, Q, b) = sv_setup(T, D)
    M0, Mt = GaussianInit(m0=m0, P0=P0), LinearGaussianDynamics(F=F, b=b, Q=Q)
    for chains in (1, 16, 256):
        row = dict(config=f"SV protocol D={D} T={T} N={N} fp32, Threefry, resident chains", chains=chains)
        for par in (True, False):
            init, k = get_independent_kernel(M0, SVPotential(y=y[0]), Mt, SVPotential(params=y[1:]), N, backward=not par, Pt=Mt, parallel=par)
            cc = CsmcChains(h, np.repeat(xtrue[None], chains, axis=0).astype(np.float32), delta=0.05)
            st = CSMCState(x=cc, updated=None)
            keys = R.split(R.PRNGKey(3), 12)
            for i in range(2):
                k(keys[i], st, None)
            h.sync()
            reps = 10
            t0 = time.perf_counter()
            for i in range(reps):
                k(keys[2 + i], st, None)
            h.sync()
            el = (time.perf_counter() - t0) / reps
            name = "pit" if par else "sequential_backward_sampling"
            row[name + "_ms_per_sweep"] = round(el * 1e3, 3)
            row[name + "_updated"] = round(float((cc.ancestors.to_host() != 0).mean()), 3)
        row["speedup"] = round(row["sequential_backward_sampling_ms_per_sweep"] / row["pit_ms_per_sweep"], 2)
        print(json.dumps(row), flush=True)


def c5_batched_scalar(T=8192, B=64):
    """C5 as the reference's spatial example actually runs it (examples/spatial/model.py:103-112, auxiliary_kalman.py:18-28): d^2 = 64
    INDEPENDENT scalar chains on the batch axis B, not one dense 64 x 64 state.  AR(1) rows of the grid model, first-order aux observations."""
    import aux_ssm_samplers_amd._primitives.kalman as P
    rng = np.random.default_rng(0)
    delta = 0.1
    f32 = np.float32
    lg = P.LGSSM(np.zeros((B, 1), f32), np.ones((B, 1, 1), f32), np.full((T - 1, B, 1, 1), 0.9, f32), np.ones((T - 1, B, 1, 1), f32),
                 np.zeros((T - 1, B, 1), f32), np.ones((T, B, 1, 1), f32), np.full((T, B, 1, 1), delta / 2, f32), np.zeros((T, B, 1), f32))
    u = rng.standard_normal((T, B, 1)).astype(f32)
    eps = rng.standard_normal((T, B, 1)).astype(f32)
    h = _lib.default_handle()
    for rep in range(2):
        out = {}
        for kid, name in ((_lib.K_FILTER_INIT, "filter_init_ms"), (_lib.K_FILTER_SCAN, "filter_scan_ms")):
            h.prof_enable(kid, 4)
            ms, Ps, ell = P.filtering(u, lg, True)
            out[name] = round(h.prof_read()[1], 4)
            h.prof_disable()
        for kid, name in ((_lib.K_SAMPLE_INIT, "sampler_init_ms"), (_lib.K_SAMPLE_SCAN, "sampler_scan_ms")):
            h.prof_enable(kid, 4)
            xs = P.sampling(None, ms, Ps, lg, True, eps=eps)
            out[name] = round(h.prof_read()[1], 4)
            h.prof_disable()
    print(json.dumps(dict(config=f"C5 as B = {B} independent scalar chains on the batch axis (the reference's spatial example), T={T} fp32, per-lane kernels",
                          **out)))


def sv30(T=250, D=30, N=25):
    """the reference's own timed stochastic-volatility protocol (examples/stochastic_volatility/experiment.sh:1-10: D = 30, T = 250, cSMC with N = 25
    particles, backward sampling): auxiliary cSMC sweeps per second at several chain counts, classical sweep (csrc/csmc_wide.hip)"""
    from aux_ssm_samplers_amd.workloads import sv_setup
    from aux_ssm_samplers_amd.csmc import CsmcChains, CSMCState, get_independent_kernel, GaussianInit, LinearGaussianDynamics, SVPotential
    h = _lib.default_handle()
    y, xtrue, (m0, P0, F, Q, b) = sv_setup(T, D)
    M0, Mt = GaussianInit(m0=m0, P0=P0), LinearGaussianDynamics(F=F, b=b, Q=Q)
    for gradient in (False, True, "exact"):  # (--gradient of the protocol: experiment.py:18-57; "exact" = the per-particle weighting, AUXSSM_GRAD_EXACT)
        init, kernel = get_independent_kernel(M0, SVPotential(y=y[0]), Mt, SVPotential(params=y[1:]), N, backward=True, Pt=Mt, gradient=gradient)
        for chains in (1, 256, 4096):
            cc = CsmcChains(h, np.repeat(xtrue[None], chains, axis=0).astype(np.float32))
            st = CSMCState(x=cc, updated=None)
            kernel(0, st, 0.05)
            h.sync()
            reps = 5
            t0 = time.perf_counter()
            for k in range(reps):
                kernel(1 + k, st, None)
            h.sync()
            el = time.perf_counter() - t0
            print(json.dumps(dict(config=f"SV protocol D={D} T={T}, aux-cSMC N={N} independent proposals (gradient={gradient}) + backward sampling, fp32, resident chains",
                                  chains=chains, sweeps_per_s=round(chains * reps / el, 1), ms_per_sweep_call=round(el / reps * 1e3, 3),
                                  updated=float((cc.ancestors.to_host() != 0).mean()))), flush=True)


def guided(chains=256, reps=5):
    """guided (locally optimal) proposals beside the independent ones of the same run, resident chains, backward sampling, fp32:
    config C3's shape (SV d = 1, T = 65536, N = 1024) and the reference's SV protocol (D = 30, T = 250, N = 25), with and without gradient"""
    import bench
    from aux_ssm_samplers_amd.workloads import sv_setup
    from aux_ssm_samplers_amd.csmc import (CsmcChains, CSMCState, get_independent_kernel, get_guided_kernel, GaussianInit, LinearGaussianDynamics,
                                           SVPotential)
    h = _lib.default_handle()
    T3 = 65536
    phi, q, xsv, ysv = bench.sv_data(T3, 0)
    y30, x30, (m0, P0, F, Q, b) = sv_setup(250, 30)
    shapes = (("C3 shape SV d=1 T=65536 N=1024", GaussianInit(m0=[0.0], P0=[[q]]), LinearGaussianDynamics(F=[[phi]], b=[0.0], Q=[[q]]), ysv.reshape(T3, 1),
               xsv.reshape(T3, 1), 1024, 0.5),
              ("SV protocol D=30 T=250 N=25", GaussianInit(m0=m0, P0=P0), LinearGaussianDynamics(F=F, b=b, Q=Q), y30, x30, 25, 0.05))
    for label, M0, Mt, y, x, N, delta in shapes:
        for name, get in (("independent", get_independent_kernel), ("guided", get_guided_kernel)):
            for gradient in (False, True):
                init, kernel = get(M0, SVPotential(y=y[0]), Mt, SVPotential(params=y[1:]), N, backward=True, Pt=Mt, gradient=gradient)
                cc = CsmcChains(h, np.repeat(x[None], chains, axis=0).astype(np.float32))
                st = CSMCState(x=cc, updated=None)
                kernel(0, st, delta)
                h.sync()
                t0 = time.perf_counter()
                for k in range(reps):
                    kernel(1 + k, st, None)
                h.sync()
                el = time.perf_counter() - t0
                print(json.dumps(dict(config=f"{label}, aux-cSMC {name} proposals (gradient={gradient}) + backward sampling, fp32, resident chains", chains=chains,
                                      sweeps_per_s=round(chains * reps / el, 1), ms_per_sweep_call=round(el / reps * 1e3, 3),
                                      updated=float((cc.ancestors.to_host() != 0).mean()))), flush=True)
                del cc, st


def spatial(grid=5, T=1024, N=25, chains=256, reps=5, runs=3):
    """the reference's spatial example (examples/spatial: random walk on a grid x grid lattice, multivariate Student-t observations with a banded precision
    matrix, nu = 1, N = 25, T = 1024) on the 5 x 5 grid, the largest the wide cSMC kernels hold (dx <= 32; the reference's own D = 8 is beyond them): independent
    proposals, independent with gradient and guided proposals, resident chains, backward sampling, fp32, Threefry noise -- each beside the SAME sweep with the
    stochastic-volatility potential on the same dynamics and data (what the multivariate-t potential costs: one more row product and one logarithm per particle
    and step instead of dx exponentials).  `runs` measurements per leg, potentials alternating."""
    from aux_ssm_samplers_amd.workloads import spatial_setup
    from aux_ssm_samplers_amd.csmc import CsmcChains, CSMCState, get_independent_kernel, get_guided_kernel, SVPotential
    h = _lib.default_handle()
    M0, Mt, G0, Gt, x, y, prec = spatial_setup(T, grid)
    pots = (("multivariate-t", G0, Gt), ("SV", SVPotential(y=y[0]), SVPotential(params=y[1:])))
    for name, get, gradient in (("independent", get_independent_kernel, False), ("independent", get_independent_kernel, True), ("guided", get_guided_kernel, False)):
        ms = {p[0]: [] for p in pots}
        upd = {}
        for run in range(runs):
            for pname, g0, gt in pots:
                init, kernel = get(M0, g0, Mt, gt, N, backward=True, Pt=Mt, gradient=gradient)
                cc = CsmcChains(h, np.repeat(x[None], chains, axis=0).astype(np.float32))
                st = CSMCState(x=cc, updated=None)
                kernel(0, st, 0.02)
                h.sync()
                t0 = time.perf_counter()
                for k in range(reps):
                    kernel(1 + k, st, None)
                h.sync()
                ms[pname].append((time.perf_counter() - t0) / reps * 1e3)
                upd[pname] = float((cc.ancestors.to_host() != 0).mean())
                del cc, st
        best = {k: min(v) for k, v in ms.items()}
        print(json.dumps(dict(config=f"spatial {grid}x{grid} grid dx={grid * grid} T={T}, aux-cSMC N={N} {name} proposals (gradient={gradient}) + backward sampling, fp32, "
                                     "resident chains", chains=chains, ms_per_sweep_call={k: [round(v_, 3) for v_ in v] for k, v in ms.items()},
                              sweeps_per_s={k: round(chains / v * 1e3, 1) for k, v in best.items()},
                              mvt_over_sv_rate=round(best["SV"] / best["multivariate-t"], 3), updated=upd)), flush=True)


def lingauss(dx=24, dy=12, T=1024, N=25, chains=256, reps=5, runs=3):
    """a partially observed linear-Gaussian model (workloads.lgssm_tracking_setup: dx = 24 states seen through dy = 12 dense linear mixtures with correlated
    noise, T = 1024, N = 25) through the wide cSMC kernels with the linear-Gaussian observation potential: independent proposals, independent with gradient and
    guided proposals, resident chains, backward sampling, fp32, Threefry noise -- each beside the SAME sweep with GaussianObsPotential (every component observed
    directly, one isotropic scale) on the same dynamics and a data array of the same shape as the device holds it (what the new potential costs: one more
    dx x dx row product per particle and step).  `runs` measurements per leg, potentials alternating."""
    from aux_ssm_samplers_amd.workloads import lgssm_tracking_setup
    from aux_ssm_samplers_amd.csmc import CsmcChains, CSMCState, get_independent_kernel, get_guided_kernel, GaussianObsPotential
    h = _lib.default_handle()
    M0, Mt, G0, Gt, x, y, H, Rm = lgssm_tracking_setup(T, dx, dy)
    yd = x + 0.7 * np.random.Generator(np.random.PCG64(1)).standard_normal(x.shape)
    pots = (("linear-Gaussian", G0, Gt), ("Gaussian-obs", GaussianObsPotential(sig=0.7, y=yd[0]), GaussianObsPotential(sig=0.7, params=yd[1:])))
    for name, get, gradient in (("independent", get_independent_kernel, False), ("independent", get_independent_kernel, True), ("guided", get_guided_kernel, False)):
        ms = {p[0]: [] for p in pots}
        upd = {}
        for run in range(runs):
            for pname, g0, gt in pots:
                init, kernel = get(M0, g0, Mt, gt, N, backward=True, Pt=Mt, gradient=gradient)
                cc = CsmcChains(h, np.repeat(x[None], chains, axis=0).astype(np.float32))
                st = CSMCState(x=cc, updated=None)
                kernel(0, st, 0.02)
                h.sync()
                t0 = time.perf_counter()
                for k in range(reps):
                    kernel(1 + k, st, None)
                h.sync()
                ms[pname].append((time.perf_counter() - t0) / reps * 1e3)
                upd[pname] = float((cc.ancestors.to_host() != 0).mean())
                del cc, st
        best = {k: min(v) for k, v in ms.items()}
        print(json.dumps(dict(config=f"lingauss dx={dx} dy={dy} T={T}, aux-cSMC N={N} {name} proposals (gradient={gradient}) + backward sampling, fp32, "
                                     "resident chains", chains=chains, ms_per_sweep_call={k: [round(v_, 3) for v_ in v] for k, v in ms.items()},
                              sweeps_per_s={k: round(chains / v * 1e3, 1) for k, v in best.items()},
                              lingauss_over_gaussobs_rate=round(best["Gaussian-obs"] / best["linear-Gaussian"], 3), updated=upd)), flush=True)


def poisson(D=30, T=250, N=25, chain_counts=(1, 16, 256), reps=5, runs=3):
    """multivariate counts with a log link (workloads.poisson_setup: a stable banded linear-Gaussian log-intensity, y ~ Poisson(exp(x))) through the wide cSMC
    kernels with the Poisson potential at the SV protocol's shape (D = 30, T = 250, N = 25, fp32, resident chains, Threefry noise): independent proposals,
    independent with gradient, guided proposals (backward sampling) and the parallel-in-time sweep -- each beside the SAME sweep with SVPotential on the same
    dynamics and a data array of the same shape (per component and particle the Poisson term is one det_exp and one fma where SV's is one det_exp and two fma).
    `runs` measurements per leg, potentials alternating."""
    from aux_ssm_samplers_amd.workloads import poisson_setup
    from aux_ssm_samplers_amd.csmc import CsmcChains, CSMCState, get_independent_kernel, get_guided_kernel, SVPotential
    h = _lib.default_handle()
    M0, Mt, G0, Gt, x, y = poisson_setup(T, D)
    ysv = np.exp(0.5 * x) * np.random.Generator(np.random.PCG64(1)).standard_normal(x.shape)
    pots = (("Poisson", G0, Gt), ("SV", SVPotential(y=ysv[0]), SVPotential(params=ysv[1:])))
    legs = (("independent", get_independent_kernel, dict(backward=True, gradient=False)), ("independent", get_independent_kernel, dict(backward=True, gradient=True)),
            ("guided", get_guided_kernel, dict(backward=True, gradient=False)), ("parallel-in-time", get_independent_kernel, dict(parallel=True)))
    for name, get, kw in legs:
        for chains in chain_counts:
            ms = {p[0]: [] for p in pots}
            upd = {}
            for run in range(runs):
                for pname, g0, gt in pots:
                    init, kernel = get(M0, g0, Mt, gt, N, Pt=Mt, **kw)
                    cc = CsmcChains(h, np.repeat(x[None], chains, axis=0).astype(np.float32))
                    st = CSMCState(x=cc, updated=None)
                    kernel(0, st, 0.01)
                    h.sync()
                    t0 = time.perf_counter()
                    for k in range(reps):
                        kernel(1 + k, st, None)
                    h.sync()
                    ms[pname].append((time.perf_counter() - t0) / reps * 1e3)
                    upd[pname] = float((cc.ancestors.to_host() != 0).mean())
                    del cc, st
            best = {k: min(v) for k, v in ms.items()}
            print(json.dumps(dict(config=f"poisson D={D} T={T}, aux-cSMC N={N} {name} proposals ({', '.join(f'{k}={v}' for k, v in kw.items())}), fp32, resident chains",
                                  chains=chains, ms_per_sweep_call={k: [round(v_, 3) for v_ in v] for k, v in ms.items()},
                                  sweeps_per_s={k: round(chains / v * 1e3, 1) for k, v in best.items()},
                                  poisson_over_sv_rate=round(best["SV"] / best["Poisson"], 3), updated=upd)), flush=True)


def logistic(D=30, T=250, N=25, chain_counts=(1, 16, 256), reps=5, runs=3, family="binomial"):
    """binomial data with a logit link (workloads.logistic_setup) through the wide cSMC kernels with the logistic potential at the SV protocol's shape (D = 30,
    T = 250, N = 25, fp32, resident chains, Threefry noise): independent proposals, independent with gradient, guided proposals (backward sampling) and the
    parallel-in-time sweep -- each beside the SAME sweep with PoissonPotential on the same dynamics and a data array of the same shape (per component and particle
    the logistic term is one det_exp, one det_log and an fma where Poisson's is one det_exp and an fma).  `runs` measurements per leg, potentials alternating."""
    from aux_ssm_samplers_amd.workloads import logistic_setup
    from aux_ssm_samplers_amd.csmc import CsmcChains, CSMCState, get_independent_kernel, get_guided_kernel, PoissonPotential
    h = _lib.default_handle()
    M0, Mt, G0, Gt, x, y, _ = logistic_setup(T, D, family)
    yp = np.random.Generator(np.random.PCG64(1)).poisson(np.exp(x)).astype(np.float64)
    pots = (("logistic", G0, Gt), ("Poisson", PoissonPotential(y=yp[0]), PoissonPotential(params=yp[1:])))
    legs = (("independent", get_independent_kernel, dict(backward=True, gradient=False)), ("independent", get_independent_kernel, dict(backward=True, gradient=True)),
            ("guided", get_guided_kernel, dict(backward=True, gradient=False)), ("parallel-in-time", get_independent_kernel, dict(parallel=True)))
    for name, get, kw in legs:
        for chains in chain_counts:
            ms = {p[0]: [] for p in pots}
            upd = {}
            for run in range(runs):
                for pname, g0, gt in pots:
                    init, kernel = get(M0, g0, Mt, gt, N, Pt=Mt, **kw)
                    cc = CsmcChains(h, np.repeat(x[None], chains, axis=0).astype(np.float32))
                    st = CSMCState(x=cc, updated=None)
                    kernel(0, st, 0.01)
                    h.sync()
                    t0 = time.perf_counter()
                    for k in range(reps):
                        kernel(1 + k, st, None)
                    h.sync()
                    ms[pname].append((time.perf_counter() - t0) / reps * 1e3)
                    upd[pname] = float((cc.ancestors.to_host() != 0).mean())
                    del cc, st
            best = {k: min(v) for k, v in ms.items()}
            print(json.dumps(dict(config=f"logistic ({family}) D={D} T={T}, aux-cSMC N={N} {name} proposals ({', '.join(f'{k}={v}' for k, v in kw.items())}), fp32, resident chains",
                                  chains=chains, ms_per_sweep_call={k: [round(v_, 3) for v_ in v] for k, v in ms.items()},
                                  sweeps_per_s={k: round(chains / v * 1e3, 1) for k, v in best.items()},
                                  logistic_over_poisson_rate=round(best["Poisson"] / best["logistic"], 3), updated=upd)), flush=True)


def sv30_kalman(T=250, D=30, chains=(1, 16, 64)):
    """the other sampler of the same protocol: the auxiliary Kalman sampler with first / second order linearisation of the SV observation model at D = 30
    (examples/stochastic_volatility/auxiliary_kalman.py:22-48), fp64 as the reference runs it, parallel scan; wide-state kernels (dx = 30)"""
    from aux_ssm_samplers_amd.workloads import sv_setup
    y, xtrue, (m0, P0, F, Q, b) = sv_setup(T, D)
    h = _lib.default_handle()
    for order in (1, 2):
        model = SVModel(y, m0, P0, F, Q, b, order=order)
        init, kernel = get_kernel(model.dynamics_factory, model.observations_factory, model.log_likelihood_fn, True)
        for C_ in chains:
            try:
                ch = DeviceChains(h, np.repeat(xtrue[None], C_, axis=0), chain_minor=False)
                v, ms, acc = timed_sweeps(kernel, ch, 0.01, steps=3, warmup=1)
                print(json.dumps(dict(config=f"SV protocol D={D} T={T}, aux-Kalman order {order}, fp64, parallel scan, wide-state kernels", chains=C_,
                                      sweeps_per_s=round(v, 1), ms_per_step=round(ms, 2), accept=acc)), flush=True)
            except Exception as e:  # noqa: BLE001
                print(json.dumps(dict(config=f"SV protocol D={D} T={T}, aux-Kalman order {order}", chains=C_, error=f"{type(e).__name__}: {e}")), flush=True)


def spatial_kalman(grid=8, T=1024, chains=(1, 16, 256), steps=50, host_reps=3):
    """the spatial example's own default sampler (examples/spatial/experiment.py --style kalman): the auxiliary Kalman sampler on the batched model, 8 x 8 grid
    (d = 64), T = 1024, nu = 1, fp32, both orders: the device sweep (kalman.MVTModel, csrc/kalman_mvt.hip) on 1 / 16 / 256 resident chains, keyed noise, beside the
    host-factory path of the same run (the same methods behind lambdas, one chain).  Step size: the reference's adaptation rule for 200 sweeps (target 0.5).
    Bytes: what the sweep's passes move, counted from the shapes (PASSES arrays of C T d reals), over the sweep time; beside the device-to-device copy rate of the
    same run (read + write of a 256 MiB buffer).  The kernel groups' shares come from a separate profiled pass."""
    import functools
    from aux_ssm_samplers_amd.common import delta_adaptation
    from aux_ssm_samplers_amd.loop import loop
    from aux_ssm_samplers_amd.workloads import spatial_kalman_setup
    # rng 2 | obs at x: 4 | filter: 3 | sampler: 7 | obs at x': 3 | reverse filter: 2 | select: 2
    PASSES = 23
    h = _lib.default_handle()
    a, b_ = h.zeros((64 << 20,), np.float32), h.zeros((64 << 20,), np.float32)
    b_.copy_from(a)
    h.sync()
    t0 = time.perf_counter()
    for _ in range(20):
        b_.copy_from(a)
    h.sync()
    copy_rate = 20 * 2 * a.nbytes / (time.perf_counter() - t0)
    del a, b_
    d = grid * grid
    for order in (1, 2):
        model, x0 = spatial_kalman_setup(T, grid, order=order)
        x0 = x0[..., 0].astype(np.float32)
        init, kernel = get_kernel(model.dynamics_factory, model.observations_factory, model.log_likelihood_fn, True)
        rule = functools.partial(delta_adaptation, min_delta=1e-6, max_delta=1.0)
        delta = None
        for C_ in chains:
            ch = DeviceChains(h, np.repeat(x0[None], C_, axis=0), chain_minor=False)
            if delta is None:
                delta = loop(R.PRNGKey(0), 1e-3, KalmanSampler(x=ch, updated=True), kernel, rule, 200, target_alpha=0.5, lr=0.3, beta=0.2)[3]
            v, ms, acc = timed_sweeps(kernel, ch, delta, steps=steps, warmup=5)
            h.prof_enable(_lib.K_ALL, 16 * 10)
            timed_sweeps(kernel, ch, delta, steps=10, warmup=0)
            groups = {k: round(t / 10, 4) for k, (n, t) in h.prof_read_groups().items()}
            h.prof_disable()
            nbytes = PASSES * C_ * T * d * 4
            print(json.dumps(dict(config=f"spatial {grid} x {grid} (d={d}) T={T} nu=1, aux-Kalman order {order}, fp32, device sweep (batched scalar), resident chains",
                                  chains=C_, delta=float(f"{delta:.3g}"), ms_per_sweep=round(ms, 4), sweeps_per_s=round(v, 1), accept=acc,
                                  algorithm_bytes_per_sweep=nbytes, achieved_GBps=round(nbytes / ms / 1e6, 1), copy_GBps=round(copy_rate / 1e9, 1),
                                  ms_per_sweep_by_kernel_group=groups)), flush=True)
        # the host-factory path: the same methods, not recognisable as a device model; one chain
        hinit, hkernel = get_kernel(lambda x: model.dynamics_factory(x), lambda x, u, dl: model.observations_factory(x, u, dl), lambda x: model.log_likelihood_fn(x), True)
        st = hinit(x0[..., None])
        keys = R.split(R.PRNGKey(3), host_reps + 1)
        st = hkernel(keys[0], st, delta)
        h.sync()
        t0 = time.perf_counter()
        for k in range(host_reps):
            st = hkernel(keys[1 + k], st, delta)
        h.sync()
        print(json.dumps(dict(config=f"spatial {grid} x {grid} (d={d}) T={T} nu=1, aux-Kalman order {order}, fp32, host-factory path", chains=1,
                              delta=float(f"{delta:.3g}"), ms_per_sweep=round((time.perf_counter() - t0) / host_reps * 1e3, 2))), flush=True)


def alternating_batches(h, calls, runs):
    """(best, median, worst) ms per call of each of `calls`, their batches alternating: a batch is as many back-to-back calls as fill ~0.2 s and ends in a stream
    synchronisation; `runs` batches each"""
    reps = []
    for call in calls:
        for _ in range(2):
            call()
        h.sync()
        t0 = time.perf_counter()
        call()
        h.sync()
        reps.append(int(min(2000, max(3, 0.2 / (time.perf_counter() - t0)))))
    ts = [[] for _ in calls]
    for _ in range(runs):
        for k, call in enumerate(calls):
            t0 = time.perf_counter()
            for _ in range(reps[k]):
                call()
            h.sync()
            ts[k].append((time.perf_counter() - t0) / reps[k] * 1e3)
    return [(min(t), float(np.median(t)), max(t)) for t in ts]


def poisson_kalman(shapes=((250, 30), (16384, 1)), chain_counts=(1, 64, 256, 1024), runs=5, host_reps=3, N=25):
    """count data under the auxiliary Kalman sampler (kalman.PoissonModel on workloads.poisson_kalman_setup), fp32, both orders, resident chains, keyed noise, at the
    cSMC Poisson leg's shape (T = 250, dx = 30: wide-state kernels, dense layout) and at the SV general-path shape (T = 16384, dx = 1: chain-minor from 32 chains).
    Beside every row, in the same process: SVModel at the same shape (workloads.sv_setup's data, the same step size), the two models' batches alternating -- a batch
    is as many back-to-back sweeps as fill ~0.2 s and ends in a stream synchronisation; best and median batch of `runs`.  Then, per shape and order, the
    host-factory path of the same model (the same methods behind lambdas, one chain), and for the first shape the Poisson cSMC sweep with independent proposals
    (N = 25, backward sampling) at the same chain counts."""
    from aux_ssm_samplers_amd.workloads import poisson_kalman_setup, poisson_setup, sv_setup
    h = _lib.default_handle()

    def batches(calls):
        return alternating_batches(h, calls, runs)

    for T, D in shapes:
        delta = 0.02 if D > 4 else 0.05
        for order in (1, 2):
            pm, xp = poisson_kalman_setup(T, D, order=order)
            ysv, xsv, (m0, P0, F, Q, b) = sv_setup(T, D)
            sm = SVModel(ysv, m0, P0, F, Q, b, order=order)
            kernels = [get_kernel(m.dynamics_factory, m.observations_factory, m.log_likelihood_fn, True)[1] for m in (pm, sm)]
            for C_ in chain_counts:
                chs = [DeviceChains(h, np.repeat(x[None], C_, axis=0).astype(np.float32)) for x in (xp, xsv)]
                states = [KalmanSampler(x=c, updated=None) for c in chs]
                count = [0]

                def sweep(k):
                    count[0] += 1
                    kernels[k](R.PRNGKey(count[0]), states[k], delta)

                (pb, pmed, pmax), (sb, smed, smax) = batches([lambda: sweep(0), lambda: sweep(1)])
                print(json.dumps(dict(config=f"poisson_kalman T={T} dx={D}, aux-Kalman order {order}, fp32, {'chain-minor' if chs[0].chain_minor else 'dense'} layout, "
                                             "resident chains", chains=C_, delta=delta,
                                      ms_per_sweep=dict(Poisson=round(pb, 4), SV=round(sb, 4)), ms_per_sweep_median=dict(Poisson=round(pmed, 4), SV=round(smed, 4)),
                                      ms_per_sweep_worst=dict(Poisson=round(pmax, 4), SV=round(smax, 4)),
                                      sweeps_per_s=dict(Poisson=round(C_ / pb * 1e3, 1), SV=round(C_ / sb * 1e3, 1)), poisson_over_sv_rate=round(sb / pb, 3),
                                      accept=dict(Poisson=float(chs[0].accepted.to_host().mean()), SV=float(chs[1].accepted.to_host().mean())))), flush=True)
                del chs, states
            hinit, hkernel = get_kernel(lambda x: pm.dynamics_factory(x), lambda x, u, dl: pm.observations_factory(x, u, dl), lambda x: pm.log_likelihood_fn(x), True)
            st = hinit(xp.astype(np.float32))
            keys = R.split(R.PRNGKey(3), host_reps + 1)
            st = hkernel(keys[0], st, delta)
            h.sync()
            t0 = time.perf_counter()
            for k in range(host_reps):
                st = hkernel(keys[1 + k], st, delta)
            h.sync()
            print(json.dumps(dict(config=f"poisson_kalman T={T} dx={D}, aux-Kalman order {order}, fp32, host-factory path", chains=1, delta=delta,
                                  ms_per_sweep=round((time.perf_counter() - t0) / host_reps * 1e3, 2))), flush=True)
    from aux_ssm_samplers_amd.csmc import CsmcChains, CSMCState, get_independent_kernel
    T, D = shapes[0]
    M0, Mt, G0, Gt, x, y = poisson_setup(T, D)
    init, kernel = get_independent_kernel(M0, G0, Mt, Gt, N, Pt=Mt, backward=True, gradient=False)
    for C_ in chain_counts:
        cc = CsmcChains(h, np.repeat(x[None], C_, axis=0).astype(np.float32))
        st = CSMCState(x=cc, updated=None)
        kernel(0, st, 0.01)
        count = [0]

        def csweep():
            count[0] += 1
            kernel(count[0], st, None)

        (cb, cmed, cmax), = batches([csweep])
        print(json.dumps(dict(config=f"poisson D={D} T={T}, aux-cSMC N={N} independent proposals + backward sampling, fp32, resident chains", chains=C_,
                              ms_per_sweep=round(cb, 4), ms_per_sweep_median=round(cmed, 4), sweeps_per_s=round(C_ / cb * 1e3, 1))), flush=True)
        del cc, st


def logistic_kalman(shapes=((16384, 1, (1, 2)), (250, 30, (1,))), chain_counts=(1, 64, 256, 1024), runs=5, host_reps=3):
    """binomial and negative-binomial data under the auxiliary Kalman sampler (kalman.BinomialModel / NegBinomialModel on workloads.logistic_kalman_setup), fp32,
    resident chains, keyed noise, at the SV general-path shape (T = 16384, dx = 1, both orders: chain-minor from 32 chains) and at T = 250, dx = 30 (first order:
    wide-state kernels, dense layout).  Beside every row, in the same process: PoissonModel at the same shape and step size (workloads.poisson_kalman_setup), the
    three models' batches alternating -- a batch is as many back-to-back sweeps as fill ~0.2 s and ends in a stream synchronisation; best, median and worst batch
    of `runs`.  Then, per shape and order, the host-factory path of the binomial model (the same methods behind lambdas, one chain).  Run the leg in several
    processes and take the median of their medians."""
    from aux_ssm_samplers_amd.workloads import logistic_kalman_setup, poisson_kalman_setup
    h = _lib.default_handle()
    names = ("Binomial", "NegBinomial", "Poisson")
    for T, D, orders in shapes:
        delta = 0.02 if D > 4 else 0.05
        for order in orders:
            models = [logistic_kalman_setup(T, D, "binomial", order=order), logistic_kalman_setup(T, D, "negbinomial", order=order), poisson_kalman_setup(T, D, order=order)]
            kernels = [get_kernel(m.dynamics_factory, m.observations_factory, m.log_likelihood_fn, True)[1] for m, _ in models]
            for C_ in chain_counts:
                chs = [DeviceChains(h, np.repeat(x[None], C_, axis=0).astype(np.float32)) for _, x in models]
                states = [KalmanSampler(x=c, updated=None) for c in chs]
                count = [0]

                def sweep(k):
                    count[0] += 1
                    kernels[k](R.PRNGKey(count[0]), states[k], delta)

                ts = alternating_batches(h, [lambda: sweep(0), lambda: sweep(1), lambda: sweep(2)], runs)
                print(json.dumps(dict(config=f"logistic_kalman T={T} dx={D}, aux-Kalman order {order}, fp32, {'chain-minor' if chs[0].chain_minor else 'dense'} layout, "
                                             "resident chains", chains=C_, delta=delta,
                                      ms_per_sweep={n: round(t[0], 4) for n, t in zip(names, ts)}, ms_per_sweep_median={n: round(t[1], 4) for n, t in zip(names, ts)},
                                      ms_per_sweep_worst={n: round(t[2], 4) for n, t in zip(names, ts)},
                                      sweeps_per_s_median={n: round(C_ / t[1] * 1e3, 1) for n, t in zip(names, ts)},
                                      rate_over_poisson_median={n: round(ts[2][1] / t[1], 3) for n, t in zip(names[:2], ts)},
                                      accept={n: float(c.accepted.to_host().mean()) for n, c in zip(names, chs)})), flush=True)
                del chs, states
            bm, xb = models[0]
            hinit, hkernel = get_kernel(lambda x: bm.dynamics_factory(x), lambda x, u, dl: bm.observations_factory(x, u, dl), lambda x: bm.log_likelihood_fn(x), True)
            st = hinit(xb.astype(np.float32))
            keys = R.split(R.PRNGKey(3), host_reps + 1)
            st = hkernel(keys[0], st, delta)
            h.sync()
            t0 = time.perf_counter()
            for k in range(host_reps):
                st = hkernel(keys[1 + k], st, delta)
            h.sync()
            print(json.dumps(dict(config=f"logistic_kalman T={T} dx={D}, aux-Kalman order {order}, fp32, binomial, host-factory path", chains=1, delta=delta,
                                  ms_per_sweep=round((time.perf_counter() - t0) / host_reps * 1e3, 2))), flush=True)


def _poisson_lin_models(T, dx, dy, order):
    """(model, start state, delta = 1 / max_t lambda_max(Lam_t) on the simulated path)"""
    from aux_ssm_samplers_amd.workloads import poisson_lin_setup
    model, x, _, _ = poisson_lin_setup(T, dx, dy, order=order)
    lam = model.grad_lam(x)[1]
    return model, x, 1.0 / float(np.max(np.linalg.eigvalsh(lam)))


def poisson_lin_kalman(T=16384, dx=4, dy=128, chain_counts=(1, 64, 256), runs=5, host_reps=3, prof_sweeps=10):
    """Poisson counts through a loading matrix (kalman.PoissonLinearModel on workloads.poisson_lin_setup), fp32, both orders, dense resident chains, keyed noise,
    step size 1 / max_t lambda_max(Lam_t) on the simulated path.  Beside every row, in the same process and in alternating batches (a batch is as many back-to-back
    sweeps as fill ~0.2 s and ends in a stream synchronisation; best, median and worst batch of `runs`): kalman.PoissonModel at T, dx on dense chains -- the same
    sweep without the channel reduction.  Per order the host-factory path of the new model (the same methods behind lambdas, one chain): what its users had
    before.  Then `prof_sweeps` sweeps per chain count under the library's own event brackets (auxssm_prof_enable, all groups): `factory` is the two launches of
    k_plin_obs and nothing else, `logpdf` the two joint densities and k_plin_terms; exp_per_s = 2 C T dy exponentials per sweep over the factory time."""
    from aux_ssm_samplers_amd.workloads import poisson_kalman_setup
    h = _lib.default_handle()

    def batches(calls):
        return alternating_batches(h, calls, runs)

    for order in (1, 2):
        lm, xl, delta = _poisson_lin_models(T, dx, dy, order)
        pm, xp = poisson_kalman_setup(T, dx, order=order)
        kernels = [get_kernel(m.dynamics_factory, m.observations_factory, m.log_likelihood_fn, True)[1] for m in (lm, pm)]
        for C_ in chain_counts:
            chs = [DeviceChains(h, np.repeat(x[None], C_, axis=0).astype(np.float32), chain_minor=False) for x in (xl, xp)]
            states = [KalmanSampler(x=c, updated=None) for c in chs]
            count = [0]

            def sweep(k):
                count[0] += 1
                kernels[k](R.PRNGKey(count[0]), states[k], delta)

            (lb, lmed, lmax), (pb, pmed, pmax) = batches([lambda: sweep(0), lambda: sweep(1)])
            h.prof_enable(_lib.K_ALL, 64 * prof_sweeps)
            for _ in range(prof_sweeps):
                sweep(0)
            h.sync()
            groups = h.prof_read_groups()
            h.prof_disable()
            g_ms = {k: round(v[1] / prof_sweeps, 4) for k, v in groups.items()}
            total = sum(g_ms.values())
            fac = g_ms.get("factory", 0.0)
            print(json.dumps(dict(config=f"poisson_lin_kalman T={T} dx={dx} dy={dy}, aux-Kalman order {order}, fp32, dense layout, resident chains", chains=C_,
                                  delta=round(delta, 6), ms_per_sweep=dict(PoissonLinear=round(lb, 4), Poisson=round(pb, 4)),
                                  ms_per_sweep_median=dict(PoissonLinear=round(lmed, 4), Poisson=round(pmed, 4)),
                                  ms_per_sweep_worst=dict(PoissonLinear=round(lmax, 4), Poisson=round(pmax, 4)),
                                  sweeps_per_s=dict(PoissonLinear=round(C_ / lb * 1e3, 1), Poisson=round(C_ / pb * 1e3, 1)), linear_over_pointwise_time=round(lb / pb, 3),
                                  accept=dict(PoissonLinear=float(chs[0].accepted.to_host().mean()), Poisson=float(chs[1].accepted.to_host().mean())),
                                  group_ms_per_sweep=g_ms, factory_share_of_groups=round(fac / total, 3) if total else None,
                                  exp_per_s=round(2.0 * C_ * T * dy / (fac * 1e-3), 1) if fac else None)), flush=True)
            del chs, states
        hinit, hkernel = get_kernel(lambda x: lm.dynamics_factory(x), lambda x, u, dl: lm.observations_factory(x, u, dl), lambda x: lm.log_likelihood_fn(x), True)
        st = hinit(xl.astype(np.float32))
        keys = R.split(R.PRNGKey(3), host_reps + 1)
        st = hkernel(keys[0], st, delta)
        h.sync()
        t0 = time.perf_counter()
        for k in range(host_reps):
            st = hkernel(keys[1 + k], st, delta)
        h.sync()
        print(json.dumps(dict(config=f"poisson_lin_kalman T={T} dx={dx} dy={dy}, aux-Kalman order {order}, fp32, host-factory path", chains=1, delta=round(delta, 6),
                              ms_per_sweep=round((time.perf_counter() - t0) / host_reps * 1e3, 2))), flush=True)


def poisson_lin_trace(T=16384, dx=4, dy=128, chains=64, sweeps=20):
    """`sweeps` sweeps per order of poisson_lin_kalman's model at `chains` dense resident chains and nothing else: the process a kernel trace is taken of (per-kernel
    times of k_plin_obs and k_plin_terms; a profile belongs in a run of its own)."""
    h = _lib.default_handle()
    for order in (1, 2):
        lm, xl, delta = _poisson_lin_models(T, dx, dy, order)
        kernel = get_kernel(lm.dynamics_factory, lm.observations_factory, lm.log_likelihood_fn, True)[1]
        ch = DeviceChains(h, np.repeat(xl[None], chains, axis=0).astype(np.float32), chain_minor=False)
        st = KalmanSampler(x=ch, updated=None)
        for k in range(sweeps):
            kernel(R.PRNGKey(k), st, delta)
        h.sync()
        print(json.dumps(dict(config=f"poisson_lin_trace T={T} dx={dx} dy={dy} order {order}", chains=chains, sweeps=sweeps, delta=round(delta, 6),
                              exp_per_sweep=2 * chains * T * dy, accept=float(ch.accepted.to_host().mean()))), flush=True)


def logistic_lin_kalman(T=16384, dx=4, dy=128, chain_counts=(1, 64, 256), runs=5, host_reps=3, prof_sweeps=10):
    """Binomial and negative-binomial channels through a loading matrix (kalman.BinomialLinearModel / NegBinomialLinearModel on workloads.logistic_lin_setup), fp32,
    both orders, dense resident chains, keyed noise, each at its a-priori first-order step size 4 / max_t lambda_max(H' diag(m_t) H) -- poisson_lin_kalman's
    protocol.  Beside every row, in the same process and in alternating batches (a batch is as many back-to-back sweeps as fill ~0.2 s and ends in a stream
    synchronisation; best, median and worst batch of `runs`): kalman.PoissonLinearModel at the same T, dx, dy and its own step size -- the same sweep with the
    Poisson channel body.  Per order the host-factory path of the binomial model (the same methods behind lambdas, one chain).  Then `prof_sweeps` sweeps of
    either new model per chain count under the library's own event brackets (auxssm_prof_enable, all groups): `factory` is the two launches of
    k_plin_obs_logistic and nothing else; channel_evals_per_s = 2 C T dy channel bodies (one exp, one reciprocal, one log each) per sweep over the factory time."""
    from aux_ssm_samplers_amd.workloads import logistic_lin_setup
    h = _lib.default_handle()
    names = ("BinomialLinear", "NegBinomialLinear", "PoissonLinear")
    for order in (1, 2):
        models, xs, deltas = [], [], []
        for family in ("binomial", "negbinomial"):
            m, x = logistic_lin_setup(T, dx, dy, family, order=order)[:2]
            models.append(m), xs.append(x), deltas.append(m.first_order_delta())
        pm, xp, pdelta = _poisson_lin_models(T, dx, dy, order)
        models.append(pm), xs.append(xp), deltas.append(pdelta)
        kernels = [get_kernel(m.dynamics_factory, m.observations_factory, m.log_likelihood_fn, True)[1] for m in models]
        for C_ in chain_counts:
            chs = [DeviceChains(h, np.repeat(x[None], C_, axis=0).astype(np.float32), chain_minor=False) for x in xs]
            states = [KalmanSampler(x=c, updated=None) for c in chs]
            count = [0]

            def sweep(k):
                count[0] += 1
                kernels[k](R.PRNGKey(count[0]), states[k], deltas[k])

            ts = alternating_batches(h, [lambda: sweep(0), lambda: sweep(1), lambda: sweep(2)], runs)
            g_ms, share, rate = {}, {}, {}
            for k in (0, 1):
                h.prof_enable(_lib.K_ALL, 64 * prof_sweeps)
                for _ in range(prof_sweeps):
                    sweep(k)
                h.sync()
                groups = h.prof_read_groups()
                h.prof_disable()
                g_ms[names[k]] = {n: round(v[1] / prof_sweeps, 4) for n, v in groups.items()}
                total, fac = sum(g_ms[names[k]].values()), g_ms[names[k]].get("factory", 0.0)
                share[names[k]] = round(fac / total, 3) if total else None
                rate[names[k]] = round(2.0 * C_ * T * dy / (fac * 1e-3), 1) if fac else None
            print(json.dumps(dict(config=f"logistic_lin_kalman T={T} dx={dx} dy={dy}, aux-Kalman order {order}, fp32, dense layout, resident chains", chains=C_,
                                  delta={n: round(d, 6) for n, d in zip(names, deltas)}, ms_per_sweep={n: round(t[0], 4) for n, t in zip(names, ts)},
                                  ms_per_sweep_median={n: round(t[1], 4) for n, t in zip(names, ts)}, ms_per_sweep_worst={n: round(t[2], 4) for n, t in zip(names, ts)},
                                  sweeps_per_s={n: round(C_ / t[0] * 1e3, 1) for n, t in zip(names, ts)},
                                  time_over_poisson_linear={n: round(t[0] / ts[2][0], 3) for n, t in zip(names[:2], ts)},
                                  accept={n: float(c.accepted.to_host().mean()) for n, c in zip(names, chs)}, group_ms_per_sweep=g_ms,
                                  factory_share_of_groups=share, channel_evals_per_s=rate)), flush=True)
            del chs, states
        bm, xb, bdelta = models[0], xs[0], deltas[0]
        hinit, hkernel = get_kernel(lambda x: bm.dynamics_factory(x), lambda x, u, dl: bm.observations_factory(x, u, dl), lambda x: bm.log_likelihood_fn(x), True)
        st = hinit(xb.astype(np.float32))
        keys = R.split(R.PRNGKey(3), host_reps + 1)
        st = hkernel(keys[0], st, bdelta)
        h.sync()
        t0 = time.perf_counter()
        for k in range(host_reps):
            st = hkernel(keys[1 + k], st, bdelta)
        h.sync()
        print(json.dumps(dict(config=f"logistic_lin_kalman T={T} dx={dx} dy={dy}, aux-Kalman order {order}, fp32, binomial, host-factory path", chains=1,
                              delta=round(bdelta, 6), ms_per_sweep=round((time.perf_counter() - t0) / host_reps * 1e3, 2))), flush=True)


def smoother(runs=5):
    """auxssm_kalman_smooth beside auxssm_kalman_sample of the same process on the same resident (ms, Ps): the filter runs once on the device (chain-shared model and
    data, dense layout), then the two entry points are timed in alternating batches of back-to-back calls (~0.2 s each, `runs` per entry point) that end in a stream synchronisation; best and
    median batch.  Bytes: what the call must move, counted from the shapes -- smoother: ms, Ps in, sms, sPs out = 2 (d + d^2) reals per step and sequence; sampler:
    ms, Ps, eps in, xs out = 3 d + d^2 -- over the best time (the model is chain-shared and time-invariant: its reads are not counted)."""
    import ctypes as C
    from aux_ssm_samplers_amd.workloads import lg_model
    from aux_ssm_samplers_amd._primitives.kalman.base import DeviceLGSSM
    h = _lib.default_handle()
    bt = np.broadcast_to

    def timed_pair(calls):
        """best and median ms per call of each of `calls`, their batches alternating; a batch is as many back-to-back calls as fill ~0.2 s"""
        reps = []
        for call in calls:
            for _ in range(3):
                call()
            h.sync()
            t0 = time.perf_counter()
            call()
            h.sync()
            reps.append(int(min(2000, max(10, 0.2 / (time.perf_counter() - t0)))))
        ts = [[] for _ in calls]
        for _ in range(runs):
            for k, call in enumerate(calls):
                t0 = time.perf_counter()
                for _ in range(reps[k]):
                    call()
                h.sync()
                ts[k].append((time.perf_counter() - t0) / reps[k] * 1e3)
        return [(min(t), float(np.median(t))) for t in ts]

    for T, d, dtype, seqs in ((65536, 4, np.float64, (1, 256)), (16384, 3, np.float32, (64,))):
        m = lg_model(T, d, dtype=dtype)
        lg = (m["m0"], m["P0"], bt(m["F"], (T - 1, d, d)), bt(m["Q"], (T - 1, d, d)), bt(m["b"], (T - 1, d)),
              bt(m["Hobs"], (T, d, d)), bt(m["Robs"], (T, d, d)), bt(m["cobs"], (T, d)))
        dl = DeviceLGSSM(h, lg, 1, T, 1, d, d, False, dtype)
        yd = h.to_device(np.asarray(m["y"], dtype))
        code, item = _lib.dtype_code(dtype), np.dtype(dtype).itemsize
        for S in seqs:
            dims = _lib.Dims(S, T, 1, d, d)
            ms, Ps, ell = h.empty((S, T, 1, d), dtype), h.empty((S, T, 1, d, d), dtype), h.empty((S,), dtype)
            yarr = yd.arr(0, d, 0)
            _lib.check(h.lib.auxssm_kalman_filter(h.h, code, C.byref(dims), C.byref(dl.c), C.byref(yarr), 1, ms.ptr, Ps.ptr, ell.ptr))
            eps = h.rng_normal(R.PRNGKey(S), 0, (S, T, 1, d), dtype)
            xs, sms, sPs = h.empty((S, T, 1, d), dtype), h.empty((S, T, 1, d), dtype), h.empty((S, T, 1, d, d), dtype)
            for parallel in ((1, 0) if S == 1 else (1,)):
                sm, sa = timed_pair([
                    lambda: _lib.check(h.lib.auxssm_kalman_smooth(h.h, code, C.byref(dims), C.byref(dl.c), ms.ptr, Ps.ptr, parallel, sms.ptr, sPs.ptr)),
                    lambda: _lib.check(h.lib.auxssm_kalman_sample(h.h, code, C.byref(dims), C.byref(dl.c), ms.ptr, Ps.ptr, eps.ptr, parallel, xs.ptr))])
                b_sm, b_sa = S * T * 2 * (d + d * d) * item, S * T * (3 * d + d * d) * item
                print(json.dumps(dict(config=f"RTS smoother beside the pathwise sampler, T={T} d={d} {np.dtype(dtype).name}, dense layout, resident moments",
                                      sequences=S, parallel=parallel, smooth_ms=round(sm[0], 4), smooth_ms_median=round(sm[1], 4), sample_ms=round(sa[0], 4),
                                      sample_ms_median=round(sa[1], 4), smooth_over_sample=round(sm[0] / sa[0], 3), smooth_bytes=b_sm, sample_bytes=b_sa,
                                      smooth_GBps=round(b_sm / sm[0] / 1e6, 1), sample_GBps=round(b_sa / sa[0] / 1e6, 1))), flush=True)
            del ms, Ps, eps, xs, sms, sPs


def dynamics_theta(runs=5):
    """loop.DynamicsThetaStep (gamma + two normal fills + statistics, reduce and finish kernels) beside one keyed sweep of the same LGConcatModel once its dynamics
    are per-chain (the general path: the fused chain-shared sweep no longer applies), auxssm_dynamics_stats alone, and a device-to-device copy of the state, all in
    one process in alternating batches (alternating_batches); best batch.  stats_GBps: the state's bytes (read once) over the statistics time; copy_GBps: twice
    the state's bytes (read + write) over the copy time -- an HBM rate only where the state exceeds the 256 MB last-level cache (the 256-chain row), a cache rate below that."""
    import ctypes as C
    from aux_ssm_samplers_amd.kalman import LGConcatModel
    from aux_ssm_samplers_amd.loop import DynamicsThetaStep, MNIWPrior
    from aux_ssm_samplers_amd.workloads import lg_model
    h = _lib.default_handle()
    bt = np.broadcast_to
    for T, d, dtype, counts in ((65536, 4, np.float64, (1, 16, 256)), (16384, 1, np.float32, (1024,))):
        m = lg_model(T, d, dtype=dtype)
        for chains_n in counts:
            model = LGConcatModel(m["m0"], m["P0"], bt(m["F"], (T - 1, d, d)), bt(m["Q"], (T - 1, d, d)), bt(m["b"], (T - 1, d)), bt(m["Hobs"], (T, d, d)),
                                  bt(m["Robs"], (T, d, d)), bt(m["cobs"], (T, d)), m["y"])
            init, kernel = get_kernel(model.dynamics_factory, model.observations_factory, model.log_likelihood_fn, True)
            rng = np.random.default_rng(chains_n)
            x0 = (np.asarray(m["x_true"])[None] + 0.1 * rng.standard_normal((chains_n, T, d))).astype(dtype)
            chains = DeviceChains(h, x0, dtype)
            del x0
            state = init(chains)
            prior = MNIWPrior(np.zeros((d, d + 1)), np.eye(d + 1), d + 2.0, np.eye(d))
            step = DynamicsThetaStep(model, prior)
            keys = R.split(R.PRNGKey(3), 4096)
            it = [0]

            def nk():
                it[0] = (it[0] + 1) % 4096
                return keys[it[0]]

            step(nk(), chains)   # the model's dynamics become per-chain here
            spare = h.empty(chains.x.shape, dtype)
            stats = h.empty((chains_n, (d + 1) * (d + 1) + d * (d + 1) + d * d), np.float64)
            code = _lib.dtype_code(dtype)

            def sweep():
                nonlocal state
                state = kernel(nk(), state, 0.5)

            def stats_only():
                _lib.check(h.lib.auxssm_dynamics_stats(h.h, code, chains_n, T, d, chains.layout, chains.x.ptr, stats.ptr))

            st, sw, ss, cp = alternating_batches(h, [lambda: step(nk(), chains), sweep, stats_only, lambda: spare.copy_from(chains.x)], runs)
            nbytes = chains.x.nbytes
            print(json.dumps(dict(config=f"dynamics theta step beside one keyed sweep, LGConcatModel T={T} d={d} {np.dtype(dtype).name}, per-chain (F, b, Q)",
                                  chains=chains_n, layout="chain-minor" if chains.chain_minor else "dense", step_ms=round(st[0], 4), step_ms_median=round(st[1], 4),
                                  sweep_ms=round(sw[0], 4), sweep_ms_median=round(sw[1], 4), step_over_sweep=round(st[0] / sw[0], 4), stats_ms=round(ss[0], 4),
                                  stats_GBps=round(nbytes / ss[0] / 1e6, 1), copy_ms=round(cp[0], 4), copy_GBps=round(2 * nbytes / cp[0] / 1e6, 1),
                                  flagged=int(step.flags(chains).any()))), flush=True)
            del chains, spare, state, step, model


def csmc_theta(chains=256, runs=3):
    """Per-chain dynamics in the sequential cSMC sweep (auxssm_csmc_sweep_chain_dynamics) beside the sweeps it must be judged against, in ONE process in alternating
    batches (alternating_batches; best batch): the chain-shared sweep, the per-chain sweep on C copies of the same (F, b, Q), and the time-varying sweep whose
    T - 1 rows repeat them -- the same arithmetic on the same values three ways -- then loop.DynamicsThetaStep on the CsmcChains (three fills, the conjugate
    update into staging, auxssm_csmc_dynamics_commit).  Independent proposals, backward sampling, fp32, resident chains: config C3's shape (SV d = 1, T = 65536,
    N = 1024) and SV d = 4, T = 4096, N = 64.  per_chain_over_shared should sit at 1 (the chain's row is read once, into scalar registers); a per-chain sweep
    slower than the time-varying one, which reloads a row every step, would mean the loads are still inside the time loop."""
    import bench
    from aux_ssm_samplers_amd.csmc import CsmcChains, CSMCState, GaussianInit, LinearGaussianDynamics, SVPotential, get_independent_kernel
    from aux_ssm_samplers_amd.csmc._device import ChainDynamics
    from aux_ssm_samplers_amd.loop import DynamicsThetaStep, MNIWPrior
    from aux_ssm_samplers_amd.workloads import sv_setup
    h = _lib.default_handle()
    T3 = 65536
    phi, q, xsv, ysv = bench.sv_data(T3, 0)
    y4, x4, (m0, P0, F, Q, b) = sv_setup(4096, 4)
    shapes = (("C3 shape SV d=1 T=65536 N=1024", np.zeros(1), np.array([[q]]), np.array([[phi]]), np.zeros(1), np.array([[q]]), ysv.reshape(T3, 1),
               xsv.reshape(T3, 1), 1024, 0.5),
              ("SV d=4 T=4096 N=64", m0, P0, F, b, Q, y4, x4, 64, 0.05))
    for label, m0_, P0_, F_, b_, Q_, y, x, N, delta in shapes:
        T, d = x.shape
        M0 = GaussianInit(m0=m0_, P0=P0_)
        Mt = LinearGaussianDynamics(F=F_, b=b_, Q=Q_)
        Mtv = LinearGaussianDynamics(F=np.broadcast_to(F_, (T - 1, d, d)), b=np.broadcast_to(b_, (T - 1, d)), Q=np.broadcast_to(Q_, (T - 1, d, d)))
        G0, Gt = SVPotential(y=y[0]), SVPotential(params=y[1:])
        _, k_shared = get_independent_kernel(M0, G0, Mt, Gt, N, backward=True, Pt=Mt)
        _, k_tv = get_independent_kernel(M0, G0, Mtv, Gt, N, backward=True, Pt=Mtv)
        x0 = np.repeat(x[None], chains, axis=0).astype(np.float32)
        states = []
        for per_chain in (False, True, False):
            cc = CsmcChains(h, x0, delta=delta)
            if per_chain:
                cc.dynamics = ChainDynamics(h, cc.dtype, chains, F_, b_, Q_)
            states.append(CSMCState(x=cc, updated=None))
        del x0
        it = [0]

        def sweep(kernel, st):
            def f():
                it[0] += 1
                kernel(it[0], st, None)
            return f

        sh, pc, tv = alternating_batches(h, [sweep(k_shared, states[0]), sweep(k_shared, states[1]), sweep(k_tv, states[2])], runs)
        step = DynamicsThetaStep(Mt, MNIWPrior(np.zeros((d, d + 1)), np.eye(d + 1), d + 2.0, np.eye(d)))
        keys = R.split(R.PRNGKey(3), 64)
        st, = alternating_batches(h, [lambda: step(keys[it[0] % 64], states[1].x)], runs)
        print(json.dumps(dict(config=f"{label}, aux-cSMC independent proposals + backward sampling, fp32, resident chains: shared / per-chain / time-varying "
                                     "transitions of the same values, then the (F, b, Q) step + commit", chains=chains, shared_ms=round(sh[0], 3),
                              shared_ms_median=round(sh[1], 3), per_chain_ms=round(pc[0], 3), per_chain_ms_median=round(pc[1], 3), time_varying_ms=round(tv[0], 3),
                              time_varying_ms_median=round(tv[1], 3), per_chain_over_shared=round(pc[0] / sh[0], 4), per_chain_over_time_varying=round(pc[0] / tv[0], 4),
                              step_commit_ms=round(st[0], 4), step_commit_ms_median=round(st[1], 4), step_over_sweep=round(st[0] / pc[0], 5),
                              flagged=int(step.flags(states[1].x).any()))), flush=True)
        del states, step


def observation_theta(runs=5):
    """loop.ObservationThetaStep (gamma + two normal fills + statistics, reduce and finish kernels) beside one keyed sweep of the same LGConcatModel once its
    observation model is per-chain (the dense general path, one concatenated record per chain), auxssm_observation_stats alone (on the dense state the step runs
    on, and on a chain-minor copy of it), auxssm_dynamics_stats on the same state, and a device-to-device copy of the bytes the statistics pass reads (the state;
    yobs is T dy reals beside it), all in one process in alternating batches (alternating_batches); best batch.  stats_GBps: the state's bytes (read once) over
    the statistics time; copy_GBps: twice the state's bytes (read + write) over the copy time -- an HBM rate only where the state exceeds the 256 MB last-level
    cache (the 256-chain row), a cache rate below that."""
    import ctypes as C
    from aux_ssm_samplers_amd.kalman import LGConcatModel
    from aux_ssm_samplers_amd.loop import ObservationThetaStep, ObsMNIWPrior
    from aux_ssm_samplers_amd.workloads import lg_model
    h = _lib.default_handle()
    bt = np.broadcast_to
    for T, d, dtype, counts in ((65536, 4, np.float64, (1, 16, 256)), (16384, 1, np.float32, (1024,))):
        m = lg_model(T, d, dtype=dtype)
        dy = d
        for chains_n in counts:
            model = LGConcatModel(m["m0"], m["P0"], bt(m["F"], (T - 1, d, d)), bt(m["Q"], (T - 1, d, d)), bt(m["b"], (T - 1, d)), bt(m["Hobs"], (T, dy, d)),
                                  bt(m["Robs"], (T, dy, dy)), bt(m["cobs"], (T, dy)), m["y"])
            init, kernel = get_kernel(model.dynamics_factory, model.observations_factory, model.log_likelihood_fn, True)
            rng = np.random.default_rng(chains_n)
            x0 = (np.asarray(m["x_true"])[None] + 0.1 * rng.standard_normal((chains_n, T, d))).astype(dtype)
            chains = DeviceChains(h, x0, dtype, chain_minor=False)   # (the per-chain sweep serves the dense layout)
            x_cm = h.to_device(np.ascontiguousarray(x0.transpose(1, 2, 0)), dtype)
            del x0
            state = init(chains)
            step = ObservationThetaStep(model, ObsMNIWPrior(np.zeros((dy, d + 1)), np.eye(d + 1), dy + 2.0, np.eye(dy)))
            keys = R.split(R.PRNGKey(3), 4096)
            it = [0]

            def nk():
                it[0] = (it[0] + 1) % 4096
                return keys[it[0]]

            step(nk(), chains)   # the model's observation parameters become per-chain here
            spare = h.empty(chains.x.shape, dtype)
            yarr = model.device(h, dtype)[2]
            ostats = h.empty((chains_n, (d + 1) * (d + 1) + dy * (d + 1)), np.float64)
            dstats = h.empty((chains_n, (d + 1) * (d + 1) + d * (d + 1) + d * d), np.float64)
            code = _lib.dtype_code(dtype)

            def sweep():
                nonlocal state
                state = kernel(nk(), state, 0.5)

            def stats_only():
                _lib.check(h.lib.auxssm_observation_stats(h.h, code, chains_n, T, d, dy, _lib.LAYOUT_DENSE, chains.x.ptr, C.byref(yarr), ostats.ptr))

            def stats_cm():
                _lib.check(h.lib.auxssm_observation_stats(h.h, code, chains_n, T, d, dy, _lib.LAYOUT_CHAIN_MINOR, x_cm.ptr, C.byref(yarr), ostats.ptr))

            def dyn_stats():
                _lib.check(h.lib.auxssm_dynamics_stats(h.h, code, chains_n, T, d, _lib.LAYOUT_DENSE, chains.x.ptr, dstats.ptr))

            st, sw, ss, sc, ds, cp = alternating_batches(h, [lambda: step(nk(), chains), sweep, stats_only, stats_cm, dyn_stats, lambda: spare.copy_from(chains.x)], runs)
            nbytes = chains.x.nbytes
            print(json.dumps(dict(config=f"observation theta step beside one keyed sweep, LGConcatModel T={T} dx={d} dy={dy} {np.dtype(dtype).name}, per-chain (H, c, R)",
                                  chains=chains_n, layout="dense", step_ms=round(st[0], 4), step_ms_median=round(st[1], 4), sweep_ms=round(sw[0], 4),
                                  sweep_ms_median=round(sw[1], 4), step_over_sweep=round(st[0] / sw[0], 4), stats_ms=round(ss[0], 4),
                                  stats_GBps=round(nbytes / ss[0] / 1e6, 1), stats_chain_minor_ms=round(sc[0], 4), stats_chain_minor_GBps=round(nbytes / sc[0] / 1e6, 1),
                                  dynamics_stats_ms=round(ds[0], 4), dynamics_stats_GBps=round(nbytes / ds[0] / 1e6, 1), copy_ms=round(cp[0], 4),
                                  copy_GBps=round(2 * nbytes / cp[0] / 1e6, 1), state_bytes=nbytes, flagged=int(step.flags(chains).any()))), flush=True)
            del chains, spare, state, step, model, x_cm


def em(runs=5):
    """One EM iteration as fit_em enqueues it (filter, smoother, statistics, M-step of all three blocks; no host synchronisation inside) beside
    auxssm_kalman_smooth_stats alone, filter + smoother alone, and a device-to-device copy of as many bytes as the statistics pass reads once (ys, Ps, sms, sPs), all in
    one process in alternating batches (alternating_batches); best batch.  stats_share: the statistics entry's part of the iteration; stats_GBps: those bytes over
    the statistics time; copy_GBps: twice those bytes (read + write) over the copy time -- an HBM rate only where they exceed the 256 MB last-level cache."""
    import ctypes as C
    from aux_ssm_samplers_amd._primitives.kalman.em import _Fit, NAMES
    from aux_ssm_samplers_amd.workloads import lg_model
    h = _lib.default_handle()
    for T, d, dtype, counts in ((65536, 4, np.float64, (1, 16)), (16384, 1, np.float32, (64,))):
        m = lg_model(T, d, dtype=dtype)
        start = dict(m0=m["m0"], P0=m["P0"], F=m["F"], b=m["b"], Q=m["Q"], H=m["Hobs"], c=m["cobs"], R=m["Robs"])
        for S in counts:
            rng = np.random.default_rng(S)
            ys = (np.asarray(m["y"])[None] + 0.05 * rng.standard_normal((S, T, d))).astype(dtype)
            fit = _Fit(h, ys, start, dtype, True, 1)
            y64 = ys.astype(np.float64).reshape(S * T, d)
            syy = np.concatenate([(y64.T @ y64).ravel(), [float(S * T)]])
            syy_c = (C.c_double * len(syy))(*[float(v) for v in syy])
            nbytes = fit.ybuf.nbytes + fit.Ps.nbytes + fit.sms.nbytes + fit.sPs.nbytes
            src, dst = h.zeros((nbytes,), np.uint8), h.empty((nbytes,), np.uint8)

            def iteration():
                fit.filter(0)
                fit.smooth()
                fit.statistics()
                fit.mstep(0, syy_c, None, 7)

            def filter_smooth():
                fit.filter(0)
                fit.smooth()

            iteration()
            it, ss, fs, cp = alternating_batches(h, [iteration, fit.statistics, filter_smooth, lambda: dst.copy_from(src)], runs)
            print(json.dumps(dict(config=f"EM iteration of a time-invariant LGSSM, T={T} dx={d} dy={d} {np.dtype(dtype).name}", sequences=S,
                                  iteration_ms=round(it[0], 4), iteration_ms_median=round(it[1], 4), stats_ms=round(ss[0], 4), stats_ms_median=round(ss[1], 4),
                                  filter_smooth_ms=round(fs[0], 4), filter_smooth_ms_median=round(fs[1], 4), stats_share=round(ss[0] / it[0], 4),
                                  iteration_over_filter_smooth=round(it[0] / fs[0], 4), stats_bytes=nbytes, stats_GBps=round(nbytes / ss[0] / 1e6, 1),
                                  copy_ms=round(cp[0], 4), copy_GBps=round(2 * nbytes / cp[0] / 1e6, 1), flags=fit.flags.to_host()[0].tolist())), flush=True)
            del fit, src, dst


if __name__ == "__main__":
    which = sys.argv[1:] or ["c3k", "c4", "c5"]
    if "spatial_kalman" in which:
        spatial_kalman()
    if "smoother" in which:
        smoother()
    if "dynamics_theta" in which:
        dynamics_theta()
    if "observation_theta" in which:
        observation_theta()
    if "csmc_theta" in which:
        csmc_theta()
    if "em" in which:
        em()
    if "poisson_kalman" in which:
        poisson_kalman()
    if "logistic_kalman" in which:
        logistic_kalman()
    if "poisson_lin_kalman" in which:
        poisson_lin_kalman()
    if "poisson_lin_trace" in which:
        poisson_lin_trace()
    if "logistic_lin_kalman" in which:
        logistic_lin_kalman()
    if "sv30" in which:
        sv30()
    if "guided" in which:
        guided()
    if "spatial" in which:
        spatial()
    if "lingauss" in which:
        lingauss()
    if "poisson" in which:
        poisson()
    if "logistic" in which:
        logistic()
    if "sv30k" in which:
        sv30_kalman()
    if "pit" in which:
        pit()
    if "pit30" in which:
        pit30()
    if "loop" in which:
        loops()
    if "c3k" in which:
        for chains, cmin in ((64, False), (64, None), (256, None), (1024, None)):
            c3_kalman(1, chains, chain_minor=cmin)
            c3_kalman(2, chains, chain_minor=cmin)
    if "c4" in which:
        c4()
    if "c5" in which:
        c5()
        c5_batched_scalar()
