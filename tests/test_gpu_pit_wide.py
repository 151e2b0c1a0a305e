"""The parallel-in-time cSMC sweep on WIDE states (4 < dx <= 32, N <= 64: csrc/pit_wide.hip behind auxssm_csmc_pit_sweep) ON THE GPU.

1. The contract oracle (oracle/csmc_ref.c::csmc_ref_pit_sweep), bit for bit in fp32 and fp64 on the cells of tests/pit_wide_cases.py: ancestors and trajectory.
   Of the leaf particles only the SELECTED ones are held (x_t = leaf[t][anc_t], so x and anc equal to the oracle's pin those T leaves): `pit_sweep` returns no
   leaves, as for tests/test_gpu_pit.py, whose bar this is.  A wrong unselected leaf would still move the stitch weights and with them the draws.
2. The literal tree (oracle/pit_np.py) in fp64: origins identical, trajectory within 1e-12, under the margin condition.  The bar of tests/test_gpu_pit_literal.py.
3. The two coupled potentials (multivariate Student-t, linear-Gaussian observation), which no contract oracle restates, against the literal on tests/mvt_np.py /
   tests/lingauss_np.py objects: gradient off and on, flat (all-NaN) steps at t = 0, on the top-level stitch boundary and at T - 1.
4. Launch forms at the stochastic-volatility protocol's width (d = 30, N = 25, T = 33, fp32): Threefry = explicit on the arrays of its streams, three chains in one
   launch = three launches (also with gradient proposals, fp32 and fp64), resident chains = host states, `_primitives.csmc.pit.get_kernel` on the reference's records = `get_independent_kernel(parallel=True)`.
5. Ground truth: a linear-Gaussian model (dx = 6, dy = 3, T = 6) whose exact posterior is one dense solve; `get_independent_kernel(..., N=32, parallel=True)` with
   gradient off and on, 1024 resident chains from one common start, at two step sizes with a burn-in set from the measured decay of the start's bias: every mean
   and second moment within 5 empirical standard errors (the standard deviation over chains of the per-chain time averages, over sqrt(chains)).
6. What the wide sweep does not cover is refused by the C entry point with AUXSSM_ERR_UNSUPPORTED and a message naming the limits."""
import ctypes as C

import numpy as np
import numpy.testing as npt
import pytest

from tests import pit_cases as PC
from tests import pit_wide_cases as W

pytestmark = pytest.mark.gpu


def _sweep(c, dtype, **kw):
    from aux_ssm_samplers_amd.csmc import _device
    return _device.pit_sweep(c.device_model(), c.x0.astype(dtype), c.N, noise={k: v[None] for k, v in c.noise.items()}, delta=c.delta, **kw)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("cell", W.WIDE_CELLS, ids=PC.cell_id)
def test_wide_pit_sweep_bit_exact_vs_contract_oracle(cell, dtype):
    c = PC.case(cell)
    x, anc = _sweep(c, dtype)
    ref = c.oracle_sweep(dtype)
    assert x.dtype == dtype
    npt.assert_array_equal(anc, ref["ancestors"])
    npt.assert_array_equal(x, ref["x"])


def _check_literal(c, literal, x, anc, what):
    xl, origins, hist = literal
    threshold = PC.margin_threshold(c.N)
    err = float(np.max(np.abs(x - xl)))
    print(f"{what}: smallest draw margin {hist['min_margin']:.2e} (threshold {threshold:.2e}); device: {int((anc != origins).sum())} of {c.T} origins differ, "
          f"max |x - literal| = {err:.1e}, {int((origins != 0).sum())} steps updated")
    assert hist["min_margin"] >= threshold
    npt.assert_array_equal(anc, origins)
    npt.assert_allclose(x, xl, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("cell", W.WIDE_CELLS, ids=PC.cell_id)
def test_wide_pit_sweep_fp64_equals_the_literal_tree(cell):
    c = PC.case(cell)
    x, anc = _sweep(c, np.float64)
    _check_literal(c, PC.literal(cell), x, anc, PC.cell_id(cell))


@pytest.mark.parametrize("cell", W.COUPLED_CELLS, ids=W.coupled_cell_id)
def test_wide_pit_sweep_coupled_potentials_fp64_equal_the_literal_tree(cell):
    c = W.coupled_case(cell)
    fk = c.device_model()
    assert fk.potential == (4 if c.kind == "mvt" else 5) and fk.user is None and fk.dx == c.d
    x, anc = _sweep(c, np.float64)
    _check_literal(c, W.coupled_literal(cell), x, anc, W.coupled_cell_id(cell))
    assert (anc != 0).any()


# ---- launch forms at d = 30, N = 25, T = 33, fp32 -------------------------------------------------------------------------------------------------------
SV30 = (30, 25, 33, W.SV, 0, 0, 0)


def test_threefry_sweep_equals_explicit_sweep_on_the_arrays_of_its_streams():
    from aux_ssm_samplers_amd import _lib, random as R
    from aux_ssm_samplers_amd.csmc import _device
    c = PC.case(SV30)
    h, key = _lib.default_handle(), R.PRNGKey(5)
    x0 = c.chains(2, 0)[0].astype(np.float32)
    noise = PC.keyed_noise(lambda s, shp: h.rng_normal(key, s, shp, np.float32).to_host(), lambda s, shp: h.rng_uniform(key, s, shp, np.float32).to_host(),
                           2, c.T, c.N, c.d)
    xa, anca = _device.pit_sweep(c.device_model(), x0, c.N, key=key, delta=c.delta)
    xb, ancb = _device.pit_sweep(c.device_model(), x0, c.N, noise=noise, delta=c.delta)
    npt.assert_array_equal(anca, ancb)
    npt.assert_array_equal(xa, xb)
    assert anca.any()


def test_three_chains_in_one_launch_equal_three_launches():
    from aux_ssm_samplers_amd.csmc import _device
    c = PC.case(SV30)
    x0, noise = c.chains(3, 1)
    x0 = x0.astype(np.float32)
    fk = c.device_model()
    x, anc = _device.pit_sweep(fk, x0, c.N, noise=noise, delta=c.delta)
    assert x.shape == x0.shape and anc.shape == x0.shape[:2]
    for k in range(3):
        xk, anck = _device.pit_sweep(fk, x0[k], c.N, noise={n: v[k:k + 1] for n, v in noise.items()}, delta=c.delta)
        npt.assert_array_equal(anck, anc[k])
        npt.assert_array_equal(xk, x[k])
    assert not np.array_equal(anc[0], anc[1]) and not np.array_equal(anc[1], anc[2])


def test_three_chains_with_gradient_proposals_in_one_launch_equal_three_launches():
    """the chain strides of u, the gradient and the per-step leaf weights (fp32 and fp64; time-varying transitions in the second cell)"""
    from aux_ssm_samplers_amd.csmc import _device
    for cell, dtype in (((30, 25, 9, W.SV, 1, 0, 0), np.float32), ((8, 32, 9, W.SV, 1, 1, 0), np.float64)):
        c = PC.case(cell)
        x0, noise = c.chains(3, 4)
        x0 = x0.astype(dtype)
        fk = c.device_model()
        assert fk.gradient != 0
        x, anc = _device.pit_sweep(fk, x0, c.N, noise=noise, delta=c.delta)
        for k in range(3):
            xk, anck = _device.pit_sweep(fk, x0[k], c.N, noise={n: v[k:k + 1] for n, v in noise.items()}, delta=c.delta)
            npt.assert_array_equal(anck, anc[k])
            npt.assert_array_equal(xk, x[k])
        assert anc.any() and not np.array_equal(anc[0], anc[1])


def test_sweep_on_resident_chains_equals_the_host_state_sweep():
    from aux_ssm_samplers_amd import _lib, random as R
    from aux_ssm_samplers_amd.csmc import _device, CsmcChains
    c = PC.case(SV30)
    h, key = _lib.default_handle(), R.PRNGKey(9)
    x0 = c.chains(3, 2)[0].astype(np.float32)
    fk = c.device_model()
    chains = CsmcChains(h, x0, delta=c.delta)
    assert chains.dtype == np.float32
    _device.pit_sweep_resident(fk, chains, c.N, key)
    x, anc = _device.pit_sweep(fk, x0, c.N, key=key, delta=c.delta)
    npt.assert_array_equal(chains.ancestors.to_host(), anc)
    npt.assert_array_equal(chains.to_host(), x)
    assert anc.any()


def test_reference_record_types_through_pit_get_kernel_equal_the_independent_kernel():
    """the records independent.py:78-118 builds by hand, through `_primitives.csmc.pit.get_kernel`, against `get_independent_kernel(..., parallel=True)` on the
    same auxiliary variables and draws; x, the step scale and the auxiliary noise are dyadic so that the eps_aux the wrapper recovers from u reproduces u exactly
    (tests/test_gpu_pit.py::test_reference_call_shape_through_pit_get_kernel)"""
    from aux_ssm_samplers_amd import _lib, random as R
    from aux_ssm_samplers_amd._primitives.csmc import pit
    from aux_ssm_samplers_amd.csmc import get_independent_kernel
    from aux_ssm_samplers_amd.csmc.independent import AuxiliaryMtDistribution, AuxiliaryG0, AuxiliaryGt
    c = PC.case(SV30)
    M0, G0, Mt, Gt = c.device_objects()
    T, d, N = c.T, c.d, c.N
    rng = np.random.default_rng(3)
    x = (np.round(rng.standard_normal((T, d)) * 64) / 64).astype(np.float32)
    scale = 0.5
    eps_aux = np.round(rng.standard_normal((T, d)) * 64) / 64
    u = x + scale * eps_aux
    mt = AuxiliaryMtDistribution(params=(u, scale * np.ones(T), None))
    init, kernel = pit.get_kernel(mt, AuxiliaryG0(M0=M0, G0=G0), AuxiliaryGt(Mt=Mt, Gt=Gt), N)
    key = R.PRNGKey(11)
    out = kernel(key, init(x))
    h = _lib.default_handle()
    k_prop, k_res = R.split(key, 2)
    noise = dict(eps_aux=eps_aux[None], eps_prop=h.rng_normal(k_prop, 2, (1, T, N, d), np.float32).to_host(),
                 u_res=h.rng_uniform(k_res, 3, (1, T, N), np.float32).to_host())
    init2, kernel2 = get_independent_kernel(M0, G0, Mt, Gt, N, parallel=True)
    ref = kernel2(key, init2(x), 2 * scale ** 2, noise=noise)
    assert out.x.dtype == np.float32
    npt.assert_array_equal(out.ancestors, ref.ancestors)
    npt.assert_array_equal(out.x, ref.x)
    npt.assert_array_equal(out.updated, ref.updated)
    assert ref.ancestors.any()


# ---- ground truth ---------------------------------------------------------------------------------------------------------------------------------------
# Every chain starts from the same state, the simulated trajectory (the recipe of tests/test_gpu_posterior_quadrature.py), which lies up to 2.1 posterior standard
# deviations from the posterior mean.  The largest bias of the across-chain mean, in posterior standard deviations, measured sweep by sweep on 1024 chains:
#   delta = 0.2, gradient off / on (0.74 / 0.79 of the steps updated per sweep):  1.9 at the start, 1.0 after 10 sweeps, 0.48 after 25, 0.19 after 50 and at the
#                noise floor of 1024 chains (0.06) from sweep 100 on: one e-folding per about 20 sweeps;
#   delta = 0.5, gradient on (the step delta / 2 times the gradient overshoots, 0.22 of the steps updated):  0.98 after 25 sweeps, 0.60 after 50, 0.35 after 100,
#                0.18 after 200, 0.09 after 300, at the floor from 400 on: one e-folding per about 100 sweeps.  Time averages over sweeps 100 .. 400 of this
#                configuration are 6 standard errors off (burn-in bias), over 300 .. 600 within 3.4.
# BURN is set from those decay rates -- ten e-foldings at delta = 0.2, four at delta = 0.5 (2 sd e^-4 = 0.04 sd, below the floor) -- not from the test's outcome.
@pytest.mark.parametrize("delta,burn", [(0.2, 200), (0.5, 400)], ids=["delta0.2", "delta0.5"])
@pytest.mark.parametrize("gradient", [False, True], ids=["plain", "gradient"])
def test_parallel_kernel_reproduces_the_exact_gaussian_posterior(gradient, delta, burn):
    from tests import lingauss_np as LG
    from aux_ssm_samplers_amd import _lib, random as R
    from aux_ssm_samplers_amd.csmc import get_independent_kernel, CsmcChains, CSMCState
    d, dy, T, N, Cn, M = 6, 3, 6, 32, 1024, 300
    dev, m, xtrue, _ = LG.case(d, dy, T, np.random.default_rng(17))
    mean, cov = LG.exact_posterior(m)
    mean = mean.reshape(T, d)
    second = np.stack([cov[t * d:(t + 1) * d, t * d:(t + 1) * d] + np.outer(mean[t], mean[t]) for t in range(T)])
    init, kernel = get_independent_kernel(*dev, N, gradient=gradient, parallel=True)
    chains = CsmcChains(_lib.default_handle(), np.repeat(xtrue[None], Cn, 0).astype(np.float64), delta=delta)
    state = CSMCState(x=chains, updated=None)
    s1, s2, moved = np.zeros((Cn, T, d)), np.zeros((Cn, T, d, d)), 0.0
    for i, k in enumerate(R.split(R.PRNGKey(23), burn + M)):
        state = kernel(k, state, None)
        if i >= burn:
            xs = chains.to_host()
            s1 += xs
            s2 += xs[..., :, None] * xs[..., None, :]
            moved += (chains.ancestors.to_host() != 0).mean()
    s1, s2 = s1 / M, s2 / M  # per-chain time averages
    z1 = (s1.mean(0) - mean) / (s1.std(0, ddof=1) / np.sqrt(Cn))
    z2 = (s2.mean(0) - second) / (s2.std(0, ddof=1) / np.sqrt(Cn))
    print(f"gradient={gradient} delta={delta}: {moved / M:.2f} of the steps updated per sweep; largest |z| of the means {np.abs(z1).max():.2f}, "
          f"of the second moments {np.abs(z2).max():.2f}")
    assert moved / M > 0.1  # (the chains move at all; the bar is the next line)
    assert np.abs(z1).max() < 5 and np.abs(z2).max() < 5


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------------
def test_what_the_wide_sweep_does_not_cover_is_refused_with_the_limits_in_the_message():
    from aux_ssm_samplers_amd import _lib
    from aux_ssm_samplers_amd.csmc import _device, GaussianInit, LinearGaussianDynamics, SVPotential
    h = _lib.default_handle()
    T, d, dt = 6, 8, np.float32
    y = np.zeros((T, d))
    M0, Mt = GaussianInit(m0=np.zeros(d), P0=np.eye(d)), LinearGaussianDynamics(F=0.9 * np.eye(d), b=np.zeros(d), Q=0.5 * np.eye(d))
    G0, Gt = SVPotential(y=y[0]), SVPotential(params=y[1:])
    x, anc, shd = h.to_device(np.zeros((1, T, d)), dt), h.zeros((1, T), np.int32), h.to_device(np.full(T, 0.5), dt)
    nz = _lib.CsmcNoise()
    nz.mode, nz.key0, nz.key1 = _lib.NOISE_THREEFRY, 1, 2

    def call(fk, N):
        ms = fk.struct(h, dt, T)
        rc = h.lib.auxssm_csmc_pit_sweep(h.h, _lib.dtype_code(dt), C.byref(ms), 1, T, N, shd.ptr, x.ptr, C.byref(nz), anc.ptr)
        return rc, h.lib.auxssm_last_error().decode()

    fk = _device.describe_independent(M0, G0, Mt, Gt, None, parallel=True)
    rc, msg = call(fk, 65)
    assert rc == _lib.ERR_UNSUPPORTED and "N <= 64" in msg and "dx <= 32" in msg and "N=65" in msg
    with pytest.raises(ValueError, match="N <= 64"):
        _device.pit_sweep(fk, np.zeros((T, d), dt), 65, key=0, delta=0.5)
    rc, msg = call(_device.describe_guided(M0, G0, Mt, Gt, Mt), 32)
    assert rc == _lib.ERR_UNSUPPORTED and "guided" in msg and "N <= 64" in msg and "dx <= 32" in msg
    rc, msg = call(fk, 64)  # and the largest N of the same description runs
    assert rc == 0, msg
