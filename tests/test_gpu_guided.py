"""Guided (locally optimal) auxiliary proposals on the GPU: csmc.get_guided_kernel, AUXSSM_PROP_AUX_GUIDED, the register kernels (dx <= 4) and the wide
kernels (4 < dx <= 32, N <= 64).

No contract oracle restates this proposal, so parity is against the LITERAL NumPy sampler (tests/guided_np.py on oracle/csmc_np.py::get_generic_kernel):
fp64 with explicit noise -- identical resampling ancestors and backward indices, particles within 1e-12, log-weights within 1e-10 (the bars of
tests/test_gpu_csmc_literal.py; the literal's own rounding floor, tests/test_guided_literal.py, is 5e-15 / 1.1e-13).  Then: the table-free closed form on the
device's own log-weights, the models of the closed family, keyed == explicit noise bit for bit, resident chains, the fp32 tie rate, the Kalman smoother as
ground truth, and every refusal."""
import ctypes as C

import numpy as np
import numpy.testing as npt
import pytest

from oracle import csmc_np as L
from tests import guided_np as G
from tests import potential_gpu as GP

pytestmark = pytest.mark.gpu


def _fk(dev, gradient=False):
    from aux_ssm_samplers_amd import _lib
    from aux_ssm_samplers_amd.csmc import _device
    return _device.describe_guided(dev[0], dev[1], dev[2], dev[3], dev[2], _lib.GRAD_REFERENCE if gradient else _lib.GRAD_NONE)


def _against_literal(dev, m, x0, delta, N, gradient, backward, rng, closed_form=True):
    """one fp64 sweep on explicit noise next to the literal sampler; returns the ancestors"""
    from aux_ssm_samplers_amd.csmc import _device
    T, d = x0.shape
    nz = G.noise(T, N, d, rng)
    x, anc, hist = _device.sweep(_fk(dev, gradient), x0, N, backward, noise={k: v[None] for k, v in nz.items()}, delta=delta, want_history=True)
    xl, Bl, lh = G.get_kernel(m, N, backward, gradient)[1](L.Noise(**nz), x0, delta)
    ex, el = float(np.max(np.abs(hist["xs"] - lh["xs"]))), float(np.max(np.abs(hist["log_ws"] - lh["log_ws"])))
    print(f"d={d} N={N} T={T} gradient={gradient} backward={backward}: max |xs - literal| = {ex:.1e}, max |log_ws - literal| = {el:.1e}, "
          f"updated {int((anc != 0).sum())} of {T}")
    npt.assert_array_equal(hist["As"], lh["As"])
    npt.assert_array_equal(anc, Bl)
    npt.assert_allclose(x, xl, rtol=1e-12, atol=1e-12)
    npt.assert_allclose(hist["xs"], lh["xs"], rtol=1e-12, atol=1e-12)
    npt.assert_allclose(hist["log_ws"], lh["log_ws"], rtol=1e-10, atol=1e-10)
    assert np.all(hist["As"][:, 0] == 0) and np.array_equal(hist["xs"][:, 0], x0)  # row 0 of every step is the reference trajectory
    if closed_form and not gradient:  # the device's stored log-weights satisfy the identity that has no K_t or Lambda_t in it
        scale = np.sqrt(0.5 * np.asarray(delta, float)) * np.ones(T)
        u = x0 + scale[:, None] * nz["eps_aux"]
        for t in range(T):
            xp = hist["xs"][t - 1][hist["As"][t - 1]] if t else None
            npt.assert_allclose(hist["log_ws"][t], G.closed_form(m, t, hist["xs"][t], xp, u[t], scale[t]), rtol=1e-10, atol=1e-10)
    return anc


@pytest.mark.parametrize("backward", [False, True])
@pytest.mark.parametrize("gradient", [False, True])
def test_guided_sweep_fp64_equals_the_literal_sampler(gradient, backward):
    """the register kernels (d = 1 as sixteen full waves, d = 2, d = 4 with a partial last wave) and the wide kernels (d = 8, 30, 32; N = 25 and 64) on the cases
    of tests/test_guided_literal.py.  A single case may update nothing; over the set, every (gradient, backward) cell moves the trajectory somewhere."""
    moved = 0
    for d, N, T in G.CASES:
        rng = np.random.default_rng(1000 * d + 10 * gradient + backward)
        dev, m, xtrue, delta = G.sv_case(d, T, rng)
        x0 = xtrue + 0.3 * rng.standard_normal((T, d))
        moved += int((_against_literal(dev, m, x0, delta, N, gradient, backward, rng) != 0).sum())
    assert moved > 0


@pytest.mark.parametrize("gradient", [False, True])
@pytest.mark.parametrize("model", ["sv1", "sv3", "gauss1", "gauss3", "lorenz", "rare_event"])
def test_guided_models_of_the_closed_family(model, gradient):
    """the SV and the Gaussian-observation potential at d = 1 and 3, config C4's Lorenz-63 model (the parent's mean through the model policy, masked
    observations) and the rare-event model as an AR(1) with one observation at T - 1; backward sampling, fp64 against the literal"""
    rng = np.random.default_rng(300 + gradient)
    N = 96
    if model == "lorenz":
        T = 40
        dev, m, xtrue = G.lorenz_case(T)
        x0, delta = xtrue + 0.1 * rng.standard_normal((T, 3)), 0.05 + 0.05 * rng.random(T)
    elif model == "rare_event":
        T = 12
        dev, m, x0 = G.rare_event_case(T)
        delta = 0.2 + 0.6 * rng.random(T)
    else:
        T, d = 30, int(model[-1])
        dev, m, xtrue, delta = G.sv_case(d, T, rng, potential=model[:-1])
        x0 = xtrue + 0.3 * rng.standard_normal((T, d))
    anc = _against_literal(dev, m, x0, delta, N, gradient, True, rng)
    assert (anc != 0).any()


@pytest.mark.parametrize("batched", [False, True])
@pytest.mark.parametrize("d,N", [(2, 100), (1, 1024), (8, 25), (1, 65), (1, 512)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_keyed_noise_equals_explicit_noise(dtype, d, N, batched, monkeypatch):
    """a Threefry sweep and an explicit sweep on _device.key_noise of the same key: bitwise equal, register and wide path, several chains; batched: more chains
    than one batch, with the draws made inside the forward pass"""
    from aux_ssm_samplers_amd import _lib, random as R
    from aux_ssm_samplers_amd.csmc import _device
    rng = np.random.default_rng(11 * d)
    T, Cn = 21, (260 if d == 8 else 5)  # (wide path: more chains than CUs, the eight-wave kernel in fp32 too)
    if N in (65, 512):  # a partial last wave and eight full waves, both on the generic workgroup: two chains, three steps (the paired Threefry step has a tail)
        T, Cn = 3, 2
    dev, m, xtrue, delta = G.sv_case(d, T, rng)
    x0 = (xtrue[None] + 0.3 * rng.standard_normal((Cn, T, d))).astype(dtype)
    key = R.PRNGKey(77)
    if batched:
        monkeypatch.setenv("AUXSSM_CSMC_BATCH", "2")
        monkeypatch.setenv("AUXSSM_CSMC_NO_PREGEN", "1")
    for gradient in (False, True):
        fk = _fk(dev, gradient)
        xa, anca, _ = _device.sweep(fk, x0, N, True, key=key, delta=delta)
        xb, ancb, _ = _device.sweep(fk, x0, N, True, noise=_device.key_noise(_lib.default_handle(), key, Cn, T, N, d, dtype), delta=delta)
        npt.assert_array_equal(xa, xb)
        npt.assert_array_equal(anca, ancb)
        assert xa.dtype == dtype and len({xa[c].tobytes() for c in range(Cn)}) == Cn and (anca != 0).any()


@pytest.mark.parametrize("d,N", [(2, 100), (8, 25)])
def test_resident_chains_equal_host_sweeps_and_rebuild_their_tables(d, N):
    """three sweeps on CsmcChains equal three host-state sweeps with the same keys, bitwise; another delta gives another result (K_t and Lambda_t are rebuilt
    from the device's delta at every sweep) -- the one a host sweep with that delta gives"""
    from aux_ssm_samplers_amd import _lib, random as R
    from aux_ssm_samplers_amd.csmc import CsmcChains, CSMCState, get_guided_kernel
    rng = np.random.default_rng(5 + d)
    T, Cn = 17, 4
    dev, m, xtrue, delta = G.sv_case(d, T, rng)
    x0 = xtrue[None] + 0.3 * rng.standard_normal((Cn, T, d))
    init, kern = get_guided_kernel(dev[0], dev[1], dev[2], dev[3], N, backward=True, gradient=True)
    chains = CsmcChains(_lib.default_handle(), x0, delta=delta, dtype=np.float64)
    rs, hs = CSMCState(x=chains, updated=None), init(x0)
    for it in range(3):
        rs, hs = kern(R.PRNGKey(40 + it), rs, None), kern(R.PRNGKey(40 + it), hs, delta)
    npt.assert_array_equal(chains.to_host(), hs.x)
    npt.assert_array_equal(chains.ancestors.to_host(), hs.ancestors)
    same = kern(R.PRNGKey(50), hs, delta)
    rs = kern(R.PRNGKey(50), rs, 0.5 * delta)
    npt.assert_array_equal(chains.to_host(), kern(R.PRNGKey(50), hs, 0.5 * delta).x)
    assert not np.array_equal(chains.to_host(), same.x)


@pytest.mark.parametrize("d,N,T,Cn", [(1, 1024, 1600, 1), (30, 25, 250, 4)])
def test_fp32_ancestors_against_the_literal_order_tie_rate(d, N, T, Cn):
    """the rule of tests/test_gpu_csmc_literal.py (cumsum rounding only, whatever the proposal): rate <= 2e-4 per draw, no miss farther than one visible particle;
    register path at config C3's shape, wide path at the reference's SV protocol"""
    from aux_ssm_samplers_amd.csmc import _device
    rng = np.random.default_rng(77 + d)
    dev, m, xtrue, delta = G.sv_case(d, T, rng)
    x0 = (xtrue[None] + 0.3 * rng.standard_normal((Cn, T, d))).astype(np.float32)
    nz = dict(eps_aux=rng.standard_normal((Cn, T, d)), eps_prop=rng.standard_normal((Cn, T, N, d)), u_res=rng.random((Cn, T - 1, N)), u_bwd=rng.random((Cn, T)))
    nz = {k: v.astype(np.float32) for k, v in nz.items()}
    _, _, hist = _device.sweep(_fk(dev), x0, N, False, noise=nz, delta=0.5, want_history=True)
    assert hist["log_ws"].dtype == np.float32
    bad, tot, far = GP.tie_rate(hist, nz["u_res"])
    print(f"d={d} N={N}: {bad} of {tot} fp32 draws differ from the literal order ({bad / tot:.2e}), {far} farther than one visible particle")
    assert bad / tot <= 2e-4, (bad, tot)
    assert far == 0


@pytest.mark.parametrize("gradient", [False, True])
def test_guided_particle_gibbs_matches_the_kalman_smoother(gradient):
    """linear-Gaussian model with Gaussian observations (d = 2, T = 6): guided particle Gibbs on 1024 resident chains (Threefry keys) gives the exact posterior's
    means and second moments within 5 Monte Carlo standard errors (the construction of tests/test_gpu_user_model.py, part 3)"""
    from aux_ssm_samplers_amd import _lib, random as R
    from aux_ssm_samplers_amd.csmc import CsmcChains, CSMCState, get_guided_kernel
    rng = np.random.default_rng(9)
    T, d, sig = 6, 2, 0.7
    Cn, N, burn, iters = 1024, 32, 60, 240
    dev, m, xtrue, _ = G.sv_case(d, T, rng, potential="gauss", sig=sig)
    M0, Mt, y = dev[0], dev[2], m.y
    F, b, Q, P0, m0 = (np.asarray(a, float) for a in (Mt.F, Mt.b, Mt.Q, M0.P0, M0.m0))
    # the joint prior of (x_0, ..., x_{T-1}) and the Gaussian conditioning on y = x + sig eps, densely
    mean, cov = np.zeros((T, d)), np.zeros((T, d, T, d))
    mean[0], cov[0, :, 0, :] = m0, P0
    for t in range(1, T):
        mean[t] = F @ mean[t - 1] + b
        cov[t, :, t, :] = F @ cov[t - 1, :, t - 1, :] @ F.T + Q
        for s in range(t):
            cov[t, :, s, :] = F @ cov[t - 1, :, s, :]
            cov[s, :, t, :] = cov[t, :, s, :].T
    S = cov.reshape(T * d, T * d)
    Kg = S @ np.linalg.inv(S + sig * sig * np.eye(T * d))
    mean_true = (mean.reshape(-1) + Kg @ (y.reshape(-1) - mean.reshape(-1))).reshape(T, d)
    var_true = np.diag(S - Kg @ S).reshape(T, d)
    _, kern = get_guided_kernel(dev[0], dev[1], dev[2], dev[3], N, backward=True, gradient=gradient)
    chains = CsmcChains(_lib.default_handle(), np.zeros((Cn, T, d)), delta=0.8, dtype=np.float64)
    state = CSMCState(x=chains, updated=None)
    s1, s2 = np.zeros((Cn, T, d)), np.zeros((Cn, T, d))
    for it in range(burn + iters):
        state = kern(R.PRNGKey(2000 + it), state, None)
        if it >= burn:
            xh = chains.to_host()
            s1 += xh
            s2 += xh * xh
    m1, m2 = s1 / iters, s2 / iters  # per-chain time averages: independent across chains
    se1, se2 = m1.std(0, ddof=1) / np.sqrt(Cn), m2.std(0, ddof=1) / np.sqrt(Cn)
    z1 = np.abs(m1.mean(0) - mean_true) / se1
    z2 = np.abs(m2.mean(0) - (var_true + mean_true ** 2)) / se2
    print(f"gradient={gradient}: worst z of the means {z1.max():.2f}, of the second moments {z2.max():.2f}")
    assert z1.max() < 5 and z2.max() < 5


def test_generic_entry_accepts_the_guided_descriptor():
    from aux_ssm_samplers_amd.csmc import get_generic_kernel, GaussianInit, LinearGaussianDynamics, FlatPotential
    from aux_ssm_samplers_amd.csmc.guided import GuidedFactory
    T, d = 5, 1
    M0, Mt, G = GaussianInit(m0=[0.0], P0=[[1.0]]), LinearGaussianDynamics(F=[[0.9]], b=[0.0], Q=[[0.5]]), FlatPotential()
    init, kern = get_generic_kernel(GuidedFactory(M0, G, Mt, G, Mt), 8, backward=True, Pt=Mt)
    out = kern(np.array([0, 3], np.uint32), init(np.zeros((T, d))), 0.5)
    assert out.x.shape == (T, d) and np.all(np.isfinite(out.x))


def test_c_entry_points_refuse_what_the_guided_kernels_do_not_cover():
    """AUXSSM_ERR_UNSUPPORTED from the C ABI itself: guided with a user program, with time-varying transitions, on the parallel-in-time entry"""
    from aux_ssm_samplers_amd import _lib
    from aux_ssm_samplers_amd.csmc import (_device, GaussianInit, LinearGaussianDynamics, FlatPotential, SVPotential, DevicePotential, device_models as U)
    h = _lib.default_handle()
    T, N, d, dt = 6, 64, 1, np.float64
    M0, Mt = GaussianInit(m0=[0.0], P0=[[1.0]]), LinearGaussianDynamics(F=[[0.9]], b=[0.0], Q=[[0.5]])
    x, anc, shd = h.to_device(np.zeros((1, T, d)), dt), h.zeros((1, T), np.int32), h.to_device(np.full(T, 0.5), dt)
    nz = _lib.CsmcNoise()
    nz.mode, nz.key0, nz.key1 = _lib.NOISE_THREEFRY, 1, 2
    tail = (1, T, N, 1, shd.ptr, x.ptr, C.byref(nz), anc.ptr, None, None, None)

    def last():
        return h.lib.auxssm_last_error().decode()

    # a user program
    y = np.zeros((T, 1))
    fk = _device.describe_independent(M0, DevicePotential(U.BUILTIN_SV, y=y[0]), Mt, DevicePotential(U.BUILTIN_SV, params=y[1:]), Mt)
    fk.proposal = _lib.PROP_AUX_GUIDED
    ms, us = fk.struct(h, dt, T), fk.user.struct(h, dt, T)
    rc = h.lib.auxssm_csmc_sweep_program(h.h, fk.user.program(dt), _lib.dtype_code(dt), C.byref(ms), C.byref(us), *tail)
    assert rc == _lib.ERR_UNSUPPORTED and "guided" in last()
    # time-varying transitions
    Mtv = LinearGaussianDynamics(F=np.full((T - 1, 1, 1), 0.9), b=np.zeros((T - 1, 1)), Q=np.full((T - 1, 1, 1), 0.5))
    fk = _device.describe_independent(M0, FlatPotential(), Mtv, FlatPotential(), Mtv)
    fk.proposal = _lib.PROP_AUX_GUIDED
    ms = fk.struct(h, dt, T)
    rc = h.lib.auxssm_csmc_sweep(h.h, _lib.dtype_code(dt), C.byref(ms), *tail)
    assert rc == _lib.ERR_UNSUPPORTED and "time-invariant" in last()
    # the parallel-in-time entry
    fk = _device.describe_guided(M0, SVPotential(y=y[0]), Mt, SVPotential(params=y[1:]), Mt)
    ms = fk.struct(h, dt, T)
    rc = h.lib.auxssm_csmc_pit_sweep(h.h, _lib.dtype_code(dt), C.byref(ms), 1, T, N, shd.ptr, x.ptr, C.byref(nz), anc.ptr)
    assert rc == _lib.ERR_UNSUPPORTED and "guided" in last()
    # and the plain sweep of the same description runs
    assert h.lib.auxssm_csmc_sweep(h.h, _lib.dtype_code(dt), C.byref(ms), *tail) == 0
