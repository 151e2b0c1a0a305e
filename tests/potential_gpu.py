"""The GPU side of the tests of the built-in observation potentials of the cSMC family, once: how a model is described and its noise drawn, and the assertion
blocks that tests/test_gpu_mvt.py, tests/test_gpu_lingauss.py, tests/test_gpu_poisson.py and tests/test_gpu_logistic.py run with their kind record
(tests/potential_np.py::Kind) -- program equality, parity with the literal sampler and the literal tree, keyed against explicit noise, resident chains, one launch
against sixteen-wave launches, the fp32 tie rate, particle Gibbs against a known posterior.  Test infrastructure only; not collected."""
import ctypes as C
import functools
import subprocess
import sys

import numpy as np
import numpy.testing as npt

from oracle import csmc_np as L
from tests import pit_cases as PC
from tests import potential_np as P

FIELDS = ("xs", "log_ws", "As", "ancestors", "x")
PROGRAM_STYLES = (("bootstrap", False), ("independent", False), ("independent", True), ("independent", "exact"))


def gmode(gradient):
    from aux_ssm_samplers_amd import _lib
    return _lib.GRAD_NONE if not gradient else (_lib.GRAD_EXACT if gradient == "exact" else _lib.GRAD_REFERENCE)


def describe(style, dev, gradient=False):
    from aux_ssm_samplers_amd.csmc import _device
    M0, G0, Mt, Gt = dev
    if style == "bootstrap":
        return _device.describe_bootstrap(M0, G0, Mt, Gt, Mt)
    if style == "guided":
        return _device.describe_guided(M0, G0, Mt, Gt, Mt, gmode(gradient))
    return _device.describe_independent(M0, G0, Mt, Gt, Mt, gmode(gradient))


def noise(Cn, T, N, d, rng, dtype=np.float64):
    nz = dict(eps_aux=rng.standard_normal((Cn, T, d)), eps_prop=rng.standard_normal((Cn, T, N, d)), u_res=rng.random((Cn, T - 1, N)), u_bwd=rng.random((Cn, T)))
    return {k: v.astype(dtype) for k, v in nz.items()}


def kernel_of(sampler, dev, N):
    """the sweep kernel of a sampler's name: independent-trace, independent-backward, exact, guided[-gradient], bootstrap, pit[-gradient]"""
    from aux_ssm_samplers_amd._primitives.csmc import get_kernel as get_bootstrap_kernel
    from aux_ssm_samplers_amd.csmc import get_guided_kernel, get_independent_kernel
    if sampler == "bootstrap":
        return get_bootstrap_kernel(*dev, N, backward=True, Pt=dev[2])[1]
    if sampler.startswith("guided"):
        return get_guided_kernel(*dev, N, backward=True, gradient=sampler.endswith("gradient"))[1]
    if sampler.startswith("pit"):
        return get_independent_kernel(*dev, N, gradient=sampler.endswith("gradient"), parallel=True)[1]
    return get_independent_kernel(*dev, N, backward=sampler != "independent-trace", Pt=dev[2], gradient="exact" if sampler == "exact" else False)[1]


# ---- the built-in against a program --------------------------------------------------------------------------------------------------------------------------
def assert_same_sweeps(fb, fu, x0, N, backward, delta, **kw):
    """the sweeps of two descriptions of one model are equal bit for bit: ancestors, trajectories, particles, log-weights and resampling indices; returns the
    first one's (ancestors, log-weights)"""
    from aux_ssm_samplers_amd.csmc import _device
    xb, ab, hb = _device.sweep(fb, x0, N, backward, delta=delta, want_history=True, **kw)
    xu, au, hu = _device.sweep(fu, x0, N, backward, delta=delta, want_history=True, **kw)
    npt.assert_array_equal(ab, au)
    npt.assert_array_equal(xb, xu)
    for name in ("xs", "log_ws", "As"):
        npt.assert_array_equal(hb[name], hu[name])
    assert xb.dtype == x0.dtype and np.all(np.isfinite(hb["log_ws"]))
    return ab, hb["log_ws"]


def assert_program_equality(kind, dev, x0, N, delta, nz, key, styles=PROGRAM_STYLES):
    """every (style, gradient) x backward mode x noise mode: the built-in sweep equals that of the same potential as a user program (kind.program), bit for bit,
    and its log-weights are finite; returns (style, gradient, backward, keyed, ancestors, log-weights) of every sweep"""
    seen = []
    for style, gradient in styles:
        fb, fu = describe(style, dev, gradient), describe(style, kind.program(dev, bool(gradient)), gradient)
        assert fb.potential == kind.code and fb.user is None and fu.user is not None
        for backward in (False, True):
            for keyed in (False, True):
                seen.append((style, gradient, backward, keyed) + assert_same_sweeps(fb, fu, x0, N, backward, delta, **(dict(key=key) if keyed else dict(noise=nz))))
    return seen


# ---- against the literal -------------------------------------------------------------------------------------------------------------------------------------
def against_literal(kind, style, gradient, backward, key):
    """one fp64 sweep on explicit noise next to the literal sampler (tests/potential_np.py::literal_sweep): resampling ancestors and backward indices identical,
    particles within 1e-12, log-weights within 1e-10; returns the ancestors"""
    from aux_ssm_samplers_amd.csmc import _device
    (xl, Bl, lh), (d, N, T, dev, m, x0, delta, nz), gap, bump = P.literal_sweep(kind, style, gradient, backward, key)
    assert gap is None or gap >= P.GAP_BAR
    nz = {k: v[None] for k, v in nz.items() if not (style == "bootstrap" and k == "eps_aux")}
    fk = describe(style, dev, gradient)
    assert fk.potential == kind.code and fk.user is None
    x, anc, hist = _device.sweep(fk, x0, N, backward, noise=nz, delta=None if style == "bootstrap" else delta, want_history=True)
    ex, el = float(np.max(np.abs(hist["xs"] - lh["xs"]))), float(np.max(np.abs(hist["log_ws"] - lh["log_ws"])))
    print(f"{style} gradient={gradient} backward={backward} {kind.label(key)}: max |xs - literal| = {ex:.1e}, max |log_ws - literal| = {el:.1e}, "
          f"updated {int((anc != 0).sum())} of {T}" + ("" if gap is None else f", smallest draw gap {gap:.1e}"))
    npt.assert_array_equal(hist["As"], lh["As"])
    npt.assert_array_equal(anc, Bl)
    npt.assert_allclose(x, xl, rtol=1e-12, atol=1e-12)
    npt.assert_allclose(hist["xs"], lh["xs"], rtol=1e-12, atol=1e-12)
    lw_lit = lh["log_ws"]
    if style == "independent" and gradient is True:
        # the reference's weighting: GradientAuxiliaryGt adds its correction summed over ALL particles (csmc/independent.py:265-266), one constant per step that
        # cancels in every normalisation and that the device does not add (include/auxssm.h, AUXSSM_GRAD_REFERENCE): compared up to that constant, read off particle 0
        lw_lit = lw_lit - (lw_lit[:, :1] - hist["log_ws"][:, :1])
        print(f"    up to the reference's per-step constant: max |log_ws - literal| = {float(np.max(np.abs(hist['log_ws'] - lw_lit))):.1e}")
    npt.assert_allclose(hist["log_ws"], lw_lit, rtol=1e-10, atol=1e-10)
    assert np.all(hist["As"][:, 0] == 0) and np.array_equal(hist["xs"][:, 0], x0)  # row 0 of every step is the reference trajectory
    if style == "independent" and not gradient:
        # the direct identity: the stored log-weights are log g_t + log initial / log transition themselves (the kernels store them before any shift)
        for t in range(T):
            g = kind.log_g(hist["xs"][t], *m.args(t))
            if t == 0:
                dens = L._mvn_chol_logpdf(hist["xs"][0], m.m0, m.LP0)
            else:
                F, b, _, LQ = m.trans(t)
                dens = L._mvn_chol_logpdf(hist["xs"][t], hist["xs"][t - 1][hist["As"][t - 1]] @ F.T + b, LQ)
            npt.assert_allclose(hist["log_ws"][t], g + dens, rtol=1e-10, atol=1e-10)
    return anc


def literal_cell_moves(kind, style, gradient, backward):
    """against_literal on every case of a (style, gradient, backward) cell: a single case may update nothing, over the set the cell moves the trajectory somewhere"""
    moved = 0
    for key in kind.cells(style, gradient, backward):
        moved += int((against_literal(kind, style, gradient, backward, key) != 0).sum())
    assert moved > 0


def pit_equals_literal_tree(kind, cell, gradient):
    """the fp64 parallel-in-time sweep against the literal tree of oracle/pit_np.py: origins identical, trajectory within 1e-12, after the margin condition of
    tests/pit_cases.margin_threshold on the literal"""
    from aux_ssm_samplers_amd.csmc import _device
    c, (xl, origins, hist) = P.pit_literal(kind, cell, gradient)
    threshold = PC.margin_threshold(c.N)
    print(f"{kind.name} tree cell {cell} gradient={gradient}: smallest draw margin {hist['min_margin']:.2e} (threshold {threshold:.2e})")
    assert hist["min_margin"] >= threshold
    fk = c.device_model()
    assert fk.potential == kind.code and fk.user is None
    x, anc = _device.pit_sweep(fk, c.x0, c.N, noise={k: v[None] for k, v in c.noise.items()}, delta=c.delta)
    print(f"    {int((anc != origins).sum())} of {c.T} origins differ, max |x - literal| = {float(np.max(np.abs(x - xl))):.1e}, {int((origins != 0).sum())} steps updated")
    assert x.dtype == np.float64
    npt.assert_array_equal(anc[0] if anc.ndim == 2 else anc, origins)
    npt.assert_allclose(x[0] if x.ndim == 3 else x, xl, rtol=1e-12, atol=1e-12)
    assert (origins != 0).any()


def pit_keyed_equals_explicit(kind, cell, gradient, delta=None):
    """three fp32 chains of a tree cell: the Threefry-keyed sweep equals the sweep on the explicit arrays of the same key (delta: the case's own, or the one given);
    returns the origins"""
    from aux_ssm_samplers_amd import _lib, random as R
    from aux_ssm_samplers_amd.csmc import _device
    dtype, Cn = np.float32, 3
    c = P.pit_literal(kind, cell, gradient)[0]
    delta = c.delta if delta is None else delta
    fk = c.device_model()
    x0 = c.chains(Cn, 1)[0].astype(dtype)
    h, key = _lib.default_handle(), R.PRNGKey(5 + c.d)
    nz = PC.keyed_noise(lambda s, shape: h.rng_normal(key, s, shape, dtype).to_host(), lambda s, shape: h.rng_uniform(key, s, shape, dtype).to_host(), Cn, c.T, c.N, c.d)
    x, anc = _device.pit_sweep(fk, x0, c.N, noise=nz, delta=delta)
    xk, anck = _device.pit_sweep(fk, x0, c.N, key=key, delta=delta)
    npt.assert_array_equal(x, xk)
    npt.assert_array_equal(anc, anck)
    assert x.dtype == dtype and np.isfinite(x).all() and anc.min() >= 0 and anc.max() < c.N
    npt.assert_array_equal(x[anc == 0], x0[anc == 0])
    return anc


# ---- resident chains, chain counts ---------------------------------------------------------------------------------------------------------------------------
def resident_equals_host(dev, x0, delta, N, style):
    """three sweeps on CsmcChains equal three host-state sweeps with the same keys, bit for bit: independent proposals with the exact gradient weighting
    ("independent"), guided proposals with gradient ("guided"), parallel in time ("pit")"""
    from aux_ssm_samplers_amd import _lib, random as R
    from aux_ssm_samplers_amd.csmc import CsmcChains, CSMCState, get_guided_kernel, get_independent_kernel
    if style == "guided":
        init, kern = get_guided_kernel(*dev, N, backward=True, gradient=True)
    else:
        init, kern = get_independent_kernel(*dev, N, backward=True, gradient="exact", parallel=style == "pit")
    chains = CsmcChains(_lib.default_handle(), x0, delta=delta, dtype=x0.dtype)
    rs, hs = CSMCState(x=chains, updated=None), init(x0)
    for it in range(3):
        rs, hs = kern(R.PRNGKey(40 + it), rs, None), kern(R.PRNGKey(40 + it), hs, delta)
    assert hs.x.dtype == x0.dtype and (hs.ancestors != 0).any()
    npt.assert_array_equal(chains.to_host(), hs.x)
    npt.assert_array_equal(chains.ancestors.to_host(), hs.ancestors)


@functools.lru_cache(maxsize=None)
def cu_count():
    """the CU count of the default handle's device: hipDeviceProp_t::multiProcessorCount, what the library's kernel selection compares the chain count with, read
    as torch.cuda.get_device_properties(device).multi_processor_count -- once, in a child process: torch ships a HIP runtime of its own, and loaded into this
    process it would stand beside the one the library is linked to (tests/test_gpu_device_delta.py resolves its ctypes calls by the runtime's name)"""
    from aux_ssm_samplers_amd import _lib
    code = f"import torch; print(torch.cuda.get_device_properties({_lib.default_handle().device}).multi_processor_count)"
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    cu = int(out.stdout.split()[-1])
    assert cu > 0
    return cu


@functools.lru_cache(maxsize=None)
def chain_inputs(seed, Cn, T, N, d):
    """x0 and explicit noise of Cn chains in fp32, every chain its own; chain c's arrays depend on (seed, c) alone (shared between tests: never modified)"""
    per = []
    for c in range(Cn):
        rng = np.random.default_rng([seed, c])
        per.append(dict(x0=rng.standard_normal((T, d)), eps_aux=rng.standard_normal((T, d)), eps_prop=rng.standard_normal((T, N, d)),
                        u_res=rng.random((T - 1, N)), u_bwd=rng.random(T)))
    out = {k: np.stack([p[k] for p in per]).astype(np.float32) for k in per[0]}
    for v in out.values():
        v.setflags(write=False)
    return out


def assert_same(got, want, what):
    """bit-identical arrays with a leading chain axis; a mismatch names the first differing (chain, step[, particle[, component]])"""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.tobytes() == want.tobytes():
        return
    bad = np.argwhere(~((got == want) | ((got != got) & (want != want))))
    if len(bad) == 0:  # (only the sign of a zero differs)
        bad = np.argwhere(np.signbit(got) != np.signbit(want))
    i = tuple(int(v) for v in bad[0])
    raise AssertionError(f"{what}: {len(bad)} of {got.size} entries differ, the first at (chain, step, ...) = {i}: {got[i]!r} against {want[i]!r}")


def sweep_fields(fk, x0, N, backward, noise, delta, **kw):
    """_device.sweep with its history, as one dict of the five compared FIELDS"""
    from aux_ssm_samplers_amd.csmc import _device
    x, anc, hist = _device.sweep(fk, x0, N, backward, noise=noise, delta=delta, want_history=True, **kw)
    return dict(xs=hist["xs"], log_ws=hist["log_ws"], As=hist["As"], ancestors=anc, x=x)


def one_launch_equals_sixteen_wave(fk, style, xtrue, delta, N, backward, what=""):
    """fp32 with more chains than CUs (the eight-wave wide kernels) against the sixteen-wave instantiations: one launch of CUs + 3 chains around xtrue (T, d) is
    bit-identical to the same chains as launches of CUs and 3; returns the number of trajectory entries that moved"""
    cu = cu_count()
    Cn, (T, d) = cu + 3, xtrue.shape
    nz = dict(chain_inputs(300 + d, Cn, T, N, d))
    x0 = (xtrue[None] + np.float32(0.3) * nz.pop("x0")).astype(np.float32)
    if style == "bootstrap":
        nz.pop("eps_aux")
        delta = None
    one = sweep_fields(fk, x0, N, backward, nz, delta)
    parts = [sweep_fields(fk, x0[a:b], N, backward, {k: v[a:b] for k, v in nz.items()}, delta) for a, b in ((0, cu), (cu, Cn))]
    for name in FIELDS:
        assert_same(one[name], np.concatenate([p[name] for p in parts]), f"{what} {name}, one launch of {Cn} chains against launches of {cu} and 3")
    assert one["xs"].dtype == np.float32 and np.all(np.isfinite(one["log_ws"]))
    assert np.all(one["As"][:, :, 0] == 0) and np.array_equal(one["xs"][:, :, 0], x0)
    return int((one["ancestors"] != 0).sum())


# ---- fp32 -----------------------------------------------------------------------------------------------------------------------------------------------------
def tie_rate(hist, u_res):
    """device fp32 ancestors vs the literal fp32 resampling redone from the DEVICE's stored log-weights and the same uniforms, step by step (teacher-forced);
    -> (misses, draws, misses farther than one visible particle): the construction of tests/test_gpu_csmc_literal.py"""
    bad = far = tot = 0
    for c in range(hist["As"].shape[0]):
        T, N = hist["log_ws"][c].shape
        for t in range(1, T):
            w = L.normalize(hist["log_ws"][c, t - 1])
            assert w.dtype == np.float32
            A = L.multinomial(u_res[c, t - 1], w)
            miss = np.nonzero(A != hist["As"][c, t - 1])[0]
            bad, tot = bad + len(miss), tot + N - 1
            for i in miss:
                a, b = sorted((int(A[i]), int(hist["As"][c, t - 1][i])))
                if b - a > 1 and float(np.sum(w[a + 1:b], dtype=np.float64)) > 8 * np.finfo(np.float32).eps:
                    far += 1
    return bad, tot, far


def tie_rate_within_the_bar(fk, x0, N, nz, delta, what, against_fp64=False):
    """one fp32 sweep with ancestor tracing on explicit noise: the literal left-to-right draw on the device's own stored fp32 log-weights (tie_rate) disagrees in
    at most 2e-4 of all draws, none farther than one visible particle -- the project's standing bar.  against_fp64: printed beside it, with no bar, the distance of
    the fp32 log-weights from the fp64 sweep on the same noise, over the particles of the first step (the same particles in both sweeps up to rounding: no
    resampling has happened yet) and over all steps whose resampling indices agree so far."""
    from aux_ssm_samplers_amd.csmc import _device
    assert x0.dtype == np.float32
    _, _, hist = _device.sweep(fk, x0, N, False, noise=nz, delta=delta, want_history=True)
    assert hist["log_ws"].dtype == np.float32 and np.all(np.isfinite(hist["log_ws"]))
    if against_fp64:
        Cn, T = x0.shape[:2]
        _, _, h64 = _device.sweep(fk, x0.astype(np.float64), N, False, noise={k: v.astype(np.float64) for k, v in nz.items()}, delta=delta, want_history=True)
        same = np.cumprod(np.all(hist["As"] == h64["As"], axis=2), axis=1).astype(bool)  # (Cn, T - 1): every resampling up to and including step t agrees
        agree = np.concatenate([np.ones((Cn, 1), bool), same], axis=1)
        dlw = np.abs(hist["log_ws"].astype(np.float64) - h64["log_ws"])
        scale = float(np.max(np.abs(h64["log_ws"][agree])))
        print(f"{what}: fp32 log-weights against the fp64 sweep on the same noise: max |diff| {float(dlw[:, 0].max()):.2e} at t = 0, "
              f"{float(dlw[agree].max()):.2e} over the {int(agree.sum())} of {Cn * T} steps whose ancestry still agrees (largest |log w| there {scale:.1f})")
    bad, tot, far = tie_rate(hist, nz["u_res"])
    print(f"{what}: {bad} of {tot} fp32 draws differ from the literal order ({bad / tot:.2e}), {far} farther than one visible particle")
    assert bad / tot <= 2e-4, (bad, tot)
    assert far == 0


# ---- particle Gibbs against a known posterior ---------------------------------------------------------------------------------------------------------------
def gibbs_moments(kernel, T, d, delta, seed, Cn=1024, burn=60, iters=240, with_delta=True):
    """per-chain time averages of x and of the products x_i x_j over `iters` sweeps of 1024 resident chains: (means, second moments) with their empirical
    standard errors across the chains, which are independent"""
    from aux_ssm_samplers_amd import _lib, random as R
    from aux_ssm_samplers_amd.csmc import CsmcChains, CSMCState
    chains = CsmcChains(_lib.default_handle(), np.zeros((Cn, T, d)), delta=delta if with_delta else None, dtype=np.float64)
    state = CSMCState(x=chains, updated=None)
    s1, s2 = np.zeros((Cn, T, d)), np.zeros((Cn, T, d, d))
    for it in range(burn + iters):
        state = kernel(R.PRNGKey(seed + it), state, None) if with_delta else kernel(R.PRNGKey(seed + it), state)
        if it >= burn:
            xh = chains.to_host()
            s1 += xh
            s2 += xh[..., :, None] * xh[..., None, :]
    m1, m2 = s1 / iters, s2 / iters
    return m1.mean(0), m1.std(0, ddof=1) / np.sqrt(Cn), m2.mean(0), m2.std(0, ddof=1) / np.sqrt(Cn)


def moments_match(estimate, truth, other, what, other_what):
    """estimate = gibbs_moments(...): every posterior mean and second moment (cross moments of a step included) within 5 empirical standard errors of truth =
    (means, second moments) -- the standard error is the standard deviation of the per-chain time averages over sqrt(chains), the rule of
    tests/test_gpu_posterior_quadrature.py.  Power: `other`, the moments of a posterior that is not the model's, lies more than 10 of the same standard errors
    away in at least one compared moment."""
    (m1, se1, m2, se2), (t1, t2), (w1, w2) = estimate, truth, other
    z1, z2 = np.abs(m1 - t1) / se1, np.abs(m2 - t2) / se2
    p1, p2 = np.abs(w1 - t1) / se1, np.abs(w2 - t2) / se2
    print(f"{what}: worst z of the means {z1.max():.2f}, of the second moments {z2.max():.2f}; {other_what} lies {max(p1.max(), p2.max()):.0f} standard errors away")
    assert max(p1.max(), p2.max()) > 10
    assert z1.max() < 5 and z2.max() < 5


# ---- the C entry points --------------------------------------------------------------------------------------------------------------------------------------
class EntryPoints:
    """auxssm_csmc_sweep and auxssm_csmc_pit_sweep called directly on one fp64 chain with Threefry noise, for a model description whose struct a test tampers
    with: struct() is a fresh FkModel of dev, sweep(ms) / pit_sweep(ms) the status of the call, error() the library's last message"""

    def __init__(self, dev, T, N, d, x, sqrt_half_delta):
        from aux_ssm_samplers_amd import _lib
        from aux_ssm_samplers_amd.csmc import _device
        self.lib, self.T, self.N, self.dt = _lib, T, N, np.float64
        self.h = h = _lib.default_handle()
        self.fk = _device.describe_independent(dev[0], dev[1], dev[2], dev[3], dev[2])
        self.x, self.anc = h.to_device(np.full((1, T, d), x), self.dt), h.zeros((1, T), np.int32)
        self.shd = h.to_device(np.full(T, sqrt_half_delta), self.dt)
        self.nz = _lib.CsmcNoise()
        self.nz.mode, self.nz.key0, self.nz.key1 = _lib.NOISE_THREEFRY, 1, 2
        self.ERR_ARG = _lib.ERR_ARG

    def struct(self, T=None):
        return self.fk.struct(self.h, self.dt, self.T if T is None else T)

    def sweep(self, ms):
        return self.h.lib.auxssm_csmc_sweep(self.h.h, self.lib.dtype_code(self.dt), C.byref(ms), 1, self.T, self.N, 1, self.shd.ptr, self.x.ptr, C.byref(self.nz),
                                            self.anc.ptr, None, None, None)

    def pit_sweep(self, ms):
        return self.h.lib.auxssm_csmc_pit_sweep(self.h.h, self.lib.dtype_code(self.dt), C.byref(ms), 1, self.T, self.N, self.shd.ptr, self.x.ptr, C.byref(self.nz),
                                                self.anc.ptr)

    def error(self):
        return self.h.lib.auxssm_last_error().decode()

    def both_refuse(self, ms, msg):
        assert self.sweep(ms) == self.ERR_ARG
        assert msg in self.error()
        assert self.pit_sweep(ms) == self.ERR_ARG
        assert msg in self.error()
