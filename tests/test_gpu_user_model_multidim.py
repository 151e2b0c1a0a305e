"""User-defined Feynman-Kac models beyond scalar states and default launches (the program path: csrc/fk_program.hip, csrc/fk_user.h, csmc.hip::run_csmc_program).

The models, their literal NumPy restatements and the list of sweeps are tests/user_models.py; tests/test_user_model_literals.py checks on the CPU that the exact
comparisons below are well posed for every entry of that list.

1. fp64 parity with the literal (oracle/csmc_np.py) on explicit noise: observations of p != dx columns read through theta (RANGE), nonlinear user means at
   dx = 2..4 under a full Q, a user potential on the built-in Lorenz transition and a user mean under the built-in masked potential, a potential of
   (x_t, x_{t-1}) on a user Jacobian, N in {2, 3, 65, 512, 1000, 1024}, T in {1, 2}, the four kinds of potential bound on inputs whose shifted weights underflow.
2. Launch-path identities, bit for bit: chain batching, Threefry = explicit noise, independence of the chains, inference of p.
3. fp32 against fp64 truth: teacher-forced log-weights within 4 times NumPy's own fp32 error, and the resampling tie rate; the four bounds in fp32 as well.

What goes red.  Two mutants were run, each on a throw-away copy of the tree; both change arithmetic only:
  - k_csmc_grad's user branch not adding gxprev: the five increments cases of test_multidim_gradient_program_fp64_equals_the_literal (xs at t < T - 1).  The
    increments cases of tests/test_gpu_user_gradient.py see it as well: this line was covered before, the new part is the same term next to a user Jacobian.
  - one sign of the Lorenz Jacobian in user_models.LORENZ_MEAN's mean_vjp (the test's own source, not the library): 16 gradient cases of the "user" and "mean"
    descriptions, the four gradient cases of test_all_user_lorenz_equals_the_builtin_lorenz_sweep, and on the CPU the host evaluation of the source in
    tests/test_user_model_literals.py (error 0.24).
So no mutant that was RUN shows a library defect which only this file catches; for the gaps below that is argued from the code:
  - the gradient flag dropped from fk_program.hip's names[FK_FWDG0 + 1] (not run; it would be as safe as the two above: the GRAD = false instantiation takes the
    same arguments, LDS size and block as the GRAD = true one, and only the proposal mean and the correction in csmc_sweep.h differ): N = 512 launches
    fn[FK_FWDG0 + 1]; a GRAD = false kernel proposes around u_t instead of u_t + delta_t / 2 grad_t, and the N512 gradexact cases compare xs with the literal's
    shifted proposals to 1e-7.  No other program test uses N = 512.
The remaining ones touch indices or launch geometry and must not be run (a wrong launch can read out of bounds or hang):
  - u.p replaced by D in fk_user.h: row t of the observations is read at y + t D; every RANGE case has p != dx, and log_ws is compared at every t >= 1.
  - a for ab in run_csmc_program's pass launches (or ab for a in the gradient launch): the batches after the first would redo the chains of the first (or read
    the gradient of other chains); test_chain_batched_program_sweep_equals_one_launch compares x and ancestors of all 7 chains, plain and gradient program.
  - swapped entries of the function table: the N in {65, 512, 1024} cases select sel = 0, 1, 2 of the plain, the gradient and the backward kernels, each
    compared with the literal.
The potential bound (exact, loose, +inf, absent) has NO failing mutant: a log_g_bound that returns another step's (finite) bound is not seen in fp64, by design --
the bound only rescales the weights of a step, and the sweep falls back to the exact maximum when they all underflow.  The bound tests show that the four kinds
give the literal's sweep; the bit-for-bit tests of tests/test_gpu_user_model.py are the ones that pin the built-in bounds' values."""
import dataclasses

import numpy as np
import numpy.testing as npt
import pytest

from oracle import csmc_np as L
from aux_ssm_samplers_amd import _lib
from tests import user_models as M

pytestmark = pytest.mark.gpu


def _ids(cases):
    return [c.id for c in cases]


def _describe(case, dev=None):
    from aux_ssm_samplers_amd.csmc import _device
    m = dev or M.device(case.spec)
    if case.proposal == "bootstrap":
        return _device.describe_bootstrap(m[0], m[1], m[2], m[3], m[2])
    g = {None: _lib.GRAD_NONE, True: _lib.GRAD_REFERENCE, "exact": _lib.GRAD_EXACT}[case.gradient]
    return _device.describe_independent(m[0], m[1], m[2], m[3], m[2], g)


def _sweep(case, dev=None, dtype=np.float64):
    """the device sweep of a case on its explicit noise (one chain, history on)"""
    from aux_ssm_samplers_amd.csmc import _device
    x0, delta, nz = M.inputs(case)
    return _device.sweep(_describe(case, dev), x0.astype(dtype), case.N, case.backward, noise={k: v[None].astype(dtype) for k, v in nz.items()}, delta=delta,
                         want_history=True)


def _first_difference(case, hist, lh):
    """where a sweep leaves the literal: the first time step at which xs / log_ws / As differ beyond the plain tolerances (for the failure message)"""
    for t in range(case.spec.T):
        for k, tol in (("xs", 1e-7 if case.gradient else 1e-12), ("log_ws", 1e-6 if case.gradient else 1e-10)):
            a, b = (M.compare_log_ws(case, h[k])[t] for h in (hist, lh)) if k == "log_ws" else (hist[k][t], lh[k][t])
            if not np.allclose(a, b, rtol=tol, atol=tol):
                return f"first difference: {k} at t = {t}, max |diff| = {np.max(np.abs(a - b)):.3e}"
        if t < case.spec.T - 1 and not np.array_equal(hist["As"][t], lh["As"][t]):
            return f"first difference: As at t = {t} ({int(np.sum(hist['As'][t] != lh['As'][t]))} of {case.N})"
    return "histories agree; the backward pass differs"


def _assert_equals_literal(case, out, log_ws_tol=1e-10):
    x, anc, hist = out
    xl, Bl, lh = M.literal_sweep(case)
    tol = 1e-7 if case.gradient else 1e-12   # (the literal differentiates numerically)
    where = f"{case.id}: {_first_difference(case, hist, lh)}"
    npt.assert_array_equal(hist["As"], lh["As"], err_msg=where)
    npt.assert_array_equal(anc, Bl, err_msg=where)
    npt.assert_allclose(x, xl, rtol=tol, atol=tol, err_msg=where)
    npt.assert_allclose(hist["xs"], lh["xs"], rtol=tol, atol=tol, err_msg=where)
    npt.assert_allclose(M.compare_log_ws(case, hist["log_ws"]), M.compare_log_ws(case, lh["log_ws"]), rtol=log_ws_tol, atol=log_ws_tol, err_msg=where)


# ---- 1. fp64 parity with the literal ------------------------------------------------------------------------------------------------------------------------
_PLAIN = [c for c in M.CASES if c.gradient is None and c.group != "bound"]
_GRAD = [c for c in M.CASES if c.gradient is not None]
_BOUND = M.cases("bound")


@pytest.mark.parametrize("case", _PLAIN, ids=_ids(_PLAIN))
def test_multidim_program_sweep_fp64_equals_the_literal(case):
    """every model x {independent, bootstrap} x {backward sampling, ancestor tracing}; N in {2, 3, 65, 512, 1000, 1024} (the 0-, 8- and 16-wave kernels, a ragged
    last wave, and at dx = 4, N = 1024 the launch beyond 64 KB of LDS); T in {1, 2}.  The Lorenz model in its three device descriptions against the one
    literal.  Ancestors equal; x, xs to 1e-12; log_ws to 1e-10."""
    fk = _describe(case)
    assert fk.user is not None
    if fk.user.flags & _lib.FK_USER_POTENTIAL:
        assert fk.user.p == case.spec.p and fk.user.y.shape == (case.spec.T, case.spec.p)
    _assert_equals_literal(case, _sweep(case))


@pytest.mark.parametrize("case", _GRAD, ids=_ids(_GRAD))
def test_multidim_gradient_program_fp64_equals_the_literal(case):
    """every model x gradient in {reference, exact} x both backward modes, the particle counts and T in {1, 2} of the plain test with gradient="exact": ancestors
    equal, x and xs to 1e-7 (the literal differentiates numerically), and the log-weights -- into which the proposal's correction enters -- to 4 times the
    literal's own numerical uncertainty: the largest change of its log_ws when grad_fd's step goes from 1e-5 to 5e-6 (never below the plain sweep's 1e-10).
    Measured uncertainty, the largest per model over the cases: range 4.3e-9, lorenz 1.5e-9, increments 5.1e-9, growth_nd 2.7e-9 (the smallest of a single case:
    6.3e-11, increments at T = 1); the device's largest deviation from the literal: range 2.7e-9, lorenz 3.5e-10, increments 3.1e-9, growth_nd 3.6e-9, at most
    1.4 times the case's own uncertainty.  With gradient=True the literal adds a constant per step that the device omits (user_models.compare_log_ws)."""
    assert _describe(case).user.flags & _lib.FK_USER_GRADIENT
    unc = M.literal_log_ws_uncertainty(case)
    out = _sweep(case)
    dev = float(np.max(np.abs(M.compare_log_ws(case, out[2]["log_ws"]) - M.compare_log_ws(case, M.literal_sweep(case)[2]["log_ws"]))))
    print(f"{case.id}: literal log_ws uncertainty {unc:.2e}, device - literal {dev:.2e}")
    _assert_equals_literal(case, out, log_ws_tol=max(4 * unc, 1e-10))


@pytest.mark.parametrize("case", _BOUND, ids=_ids(_BOUND))
def test_program_bound_and_its_fallbacks_fp64_equal_the_literal(case):
    """log_g_bound = the exact supremum, the supremum + 50, +inf, and no log_g_bound at all: the same sweep as the literal's, on ordinary inputs and on the tightened
    ones at which every weight shifted by the bound underflows (the forward pass then falls back to the exact maximum)"""
    from aux_ssm_samplers_amd.csmc import _device
    fk = _describe(case)
    assert _device.program_info(fk.user.program(np.float64))["has_bound"] == (case.spec.bound != "none")
    _assert_equals_literal(case, _sweep(case))


_LORENZ_USER = [c for c in M.CASES if c.spec.model == "lorenz" and c.spec.parts == "user" and c.group in ("grid", "gradient")]


@pytest.mark.parametrize("case", _LORENZ_USER, ids=_ids(_LORENZ_USER))
def test_all_user_lorenz_equals_the_builtin_lorenz_sweep(case):
    """the user mean + user masked potential against TRANS_LORENZ + POT_GAUSS_OBS_MASKED of the closed family, device against device: the same ancestors, x and xs
    to 1e-12, log_ws to 1e-10 (not bit for bit: the operation order of the user source is its own)"""
    builtin = dataclasses.replace(case, spec=dataclasses.replace(case.spec, parts="builtin"))
    assert _describe(builtin).user is None
    (xu, au, hu), (xb, ab, hb) = _sweep(case), _sweep(builtin)
    npt.assert_array_equal(hu["As"], hb["As"])
    npt.assert_array_equal(au, ab)
    npt.assert_allclose(xu, xb, rtol=1e-12, atol=1e-12)
    npt.assert_allclose(hu["xs"], hb["xs"], rtol=1e-12, atol=1e-12)
    npt.assert_allclose(hu["log_ws"], hb["log_ws"], rtol=1e-10, atol=1e-10)
    assert (au != 0).any()


# ---- 2. launch-path identities (exact) --------------------------------------------------------------------------------------------------------------------
_LAUNCH_SPECS = [M.Spec("range", 4, 6, "user"), M.Spec("lorenz", 3, 3, "user")]


def _chains_inputs(spec, N, C, gradient, dtype, seed=30):
    case = M.Case(spec, "independent", True, gradient, N, seed, "launch")
    x0, delta, nz = M.inputs(case, C=C)
    return case, x0.astype(dtype), delta, {k: v.astype(dtype) for k, v in nz.items()}


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("gradient", [None, "exact"])
@pytest.mark.parametrize("spec", _LAUNCH_SPECS, ids=[s.name for s in _LAUNCH_SPECS])
def test_chain_batched_program_sweep_equals_one_launch(spec, gradient, dtype, monkeypatch):
    """run_csmc_program's batch loop (the gradient kernel once on all chains, the passes batch by batch): 7 chains in batches of 3 and of 1 give the single launch's
    trajectories and ancestors bit for bit; Threefry and explicit noise, backward sampling and ancestor tracing.  (A sweep is only batched while its particle
    systems live in the workspace, so a batched sweep returns no history; the single launch with history returns the same x and ancestors, which are functions
    of xs, log_ws and As.)"""
    from aux_ssm_samplers_amd import random as R
    from aux_ssm_samplers_amd.csmc import _device
    C, N = 7, 192
    case, x0, delta, nz = _chains_inputs(spec, N, C, gradient, dtype)
    fk = _describe(case)
    key = R.PRNGKey(4242)
    for backward in (True, False):
        for kw in (dict(key=key), dict(noise=nz)):
            monkeypatch.delenv("AUXSSM_CSMC_BATCH", raising=False)
            xa, anca, _ = _device.sweep(fk, x0, N, backward, delta=delta, **kw)
            xh, anch, _ = _device.sweep(fk, x0, N, backward, delta=delta, want_history=True, **kw)
            npt.assert_array_equal(xa, xh)
            npt.assert_array_equal(anca, anch)
            for cb in ("3", "1"):
                monkeypatch.setenv("AUXSSM_CSMC_BATCH", cb)
                xb, ancb, _ = _device.sweep(fk, x0, N, backward, delta=delta, **kw)
                npt.assert_array_equal(xa, xb)
                npt.assert_array_equal(anca, ancb)
            assert len({xa[c].tobytes() for c in range(C)}) == C and (anca != 0).any()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("gradient", [False, "exact"])
@pytest.mark.parametrize("spec", _LAUNCH_SPECS, ids=[s.name for s in _LAUNCH_SPECS])
def test_chain_batched_resident_program_chains(spec, gradient, dtype, monkeypatch):
    """resident CsmcChains over three successive kernel calls, in one launch and in batches of 3 chains and of 1: the same states and ancestors"""
    from aux_ssm_samplers_amd import random as R
    from aux_ssm_samplers_amd.csmc import CsmcChains, CSMCState, get_independent_kernel
    C, N = 7, 192
    case, x0, delta, _ = _chains_inputs(spec, N, C, None, dtype)
    m = M.device(spec)
    kern = get_independent_kernel(*m, N, True, m[2], gradient=gradient)[1]
    h = _lib.default_handle()
    res = []
    for cb in (None, "3", "1"):
        if cb is None:
            monkeypatch.delenv("AUXSSM_CSMC_BATCH", raising=False)
        else:
            monkeypatch.setenv("AUXSSM_CSMC_BATCH", cb)
        chains = CsmcChains(h, x0, delta=delta, dtype=dtype)
        state = CSMCState(x=chains, updated=None)
        for it in range(3):
            state = kern(R.PRNGKey(300 + it), state, None)
        res.append((chains.to_host(), chains.ancestors.to_host()))
    for xb, ab in res[1:]:
        npt.assert_array_equal(res[0][0], xb)
        npt.assert_array_equal(res[0][1], ab)
    assert (res[0][1] != 0).mean() > 0.1


_P_NE_DX = [M.Spec("range", 2, 1, "builtin"), M.Spec("range", 2, 3, "user"), M.Spec("range", 4, 3, "builtin"), M.Spec("range", 4, 6, "user")]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("spec", _P_NE_DX, ids=[s.name for s in _P_NE_DX])
def test_threefry_equals_explicit_noise_with_p_columns(spec, dtype):
    """key= equals noise=key_noise(key) for programs whose observations have p != dx columns: everything bit for bit, plain and gradient program"""
    from aux_ssm_samplers_amd import random as R
    from aux_ssm_samplers_amd.csmc import _device
    C, N = 3, 100
    for gradient in (None, "exact"):
        case, x0, delta, _ = _chains_inputs(spec, N, C, gradient, dtype)
        fk = _describe(case)
        key = R.PRNGKey(77)
        nz = _device.key_noise(_lib.default_handle(), key, C, spec.T, N, spec.dx, dtype)
        for backward in (True, False):
            xa, aa, ha = _device.sweep(fk, x0, N, backward, key=key, delta=delta, want_history=True)
            xb, ab, hb = _device.sweep(fk, x0, N, backward, noise=nz, delta=delta, want_history=True)
            npt.assert_array_equal(xa, xb)
            npt.assert_array_equal(aa, ab)
            for k in ("xs", "log_ws", "As"):
                npt.assert_array_equal(ha[k], hb[k])
            assert (aa != 0).any()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("gradient", [None, True])
@pytest.mark.parametrize("spec", _LAUNCH_SPECS, ids=[s.name for s in _LAUNCH_SPECS])
def test_program_chains_are_independent(spec, gradient, dtype):
    """chain c of a 5-chain program sweep is the one-chain sweep of its own inputs, bit for bit"""
    from aux_ssm_samplers_amd.csmc import _device
    C, N = 5, 128
    case, x0, delta, nz = _chains_inputs(spec, N, C, gradient, dtype)
    fk = _describe(case)
    xa, aa, ha = _device.sweep(fk, x0, N, True, noise=nz, delta=delta, want_history=True)
    for c in range(C):
        x1, a1, h1 = _device.sweep(fk, x0[c], N, True, noise={k: v[c:c + 1] for k, v in nz.items()}, delta=delta, want_history=True)
        npt.assert_array_equal(xa[c], x1)
        npt.assert_array_equal(aa[c], a1)
        for k in ("xs", "log_ws", "As"):
            npt.assert_array_equal(ha[k][c], h1[k])
    assert len({xa[c].tobytes() for c in range(C)}) == C


@pytest.mark.parametrize("T", [1, 2, 24])
@pytest.mark.parametrize("spec", [_P_NE_DX[0], _P_NE_DX[3]], ids=[_P_NE_DX[0].name, _P_NE_DX[3].name])
def test_p_is_inferred_from_the_observations(spec, T):
    """DevicePotential(p=None) with y of shape (p,) or (1, p) and params (T - 1, p) -- (0, p) at T = 1 -- describes the model of an explicit p: the same
    UserModel.p and the same sweep"""
    spec = dataclasses.replace(spec, T=T)
    case = M.Case(spec, "independent", True, None, 128, 40, "p")
    explicit = M.device(spec)
    assert explicit[1].p == spec.p and explicit[3].params.shape == (T - 1, spec.p)
    ref = _sweep(case, explicit)
    inferred = M.device(spec, infer_p=True)
    row = (inferred[0], dataclasses.replace(inferred[1], y=np.reshape(inferred[1].y, (1, spec.p))), inferred[2], inferred[3])
    for dev in (inferred, row):
        assert dev[1].p is None and dev[3].p is None
        assert _describe(case, dev).user.p == spec.p == _describe(case, explicit).user.p
        out = _sweep(case, dev)
        npt.assert_array_equal(out[0], ref[0])
        npt.assert_array_equal(out[1], ref[1])
        for k in ("xs", "log_ws", "As"):
            npt.assert_array_equal(out[2][k], ref[2][k])


# ---- 3. fp32 against fp64 truth -------------------------------------------------------------------------------------------------------------------------
_fp32_runs = {}


def _fp32_sweep(chains):
    """the fp32 sweep of several one-chain cases of one spec as the chains of one launch (explicit noise, backward sampling, history on): (noise, history)"""
    from aux_ssm_samplers_amd.csmc import _device
    key = tuple(c.id for c in chains)
    if key not in _fp32_runs:
        ins = [M.inputs(c) for c in chains]
        x0 = np.stack([i[0] for i in ins]).astype(np.float32)
        nz = {k: np.stack([i[2][k] for i in ins]).astype(np.float32) for k in ins[0][2]}
        _, _, hist = _device.sweep(_describe(chains[0]), x0, chains[0].N, True, noise=nz, delta=ins[0][1], want_history=True)
        _fp32_runs[key] = (nz, hist)
    return _fp32_runs[key]


def _teacher_forced_errors(spec, hist):
    """(e_ref, e_dev): the largest deviation from the fp64 literal's log-weights at the device's own stored fp32 particles and ancestors of (the same literal
    evaluated in np.float32, the device's stored log-weights)"""
    e_ref = e_dev = 0.0
    for c in range(hist["xs"].shape[0]):
        lw64 = M.teacher_forced_log_ws(spec, hist["xs"][c], hist["As"][c], np.float64)
        lw32 = M.teacher_forced_log_ws(spec, hist["xs"][c], hist["As"][c], np.float32)
        assert np.all(np.isfinite(lw64)) and np.all(np.isfinite(hist["log_ws"][c]))
        e_ref = max(e_ref, float(np.max(np.abs(lw32 - lw64))))
        e_dev = max(e_dev, float(np.max(np.abs(hist["log_ws"][c] - lw64))))
    return e_ref, e_dev


def _tie_rate(nz, hist):
    """(misses, draws) of the device's resampling ancestors against the literal fp32 order (normalise -> cumsum -> searchsorted) redone from the device's own
    stored log-weights and the same uniforms; a miss sits at a boundary: a neighbouring particle, or only zero-weight particles in between"""
    miss = total = 0
    Cn, T, N = hist["log_ws"].shape
    for c in range(Cn):
        for t in range(1, T):
            w = L.normalize(hist["log_ws"][c, t - 1])
            ref = L.multinomial(nz["u_res"][c, t - 1], w)
            got = hist["As"][c, t - 1]
            bad = np.nonzero(ref != got)[0]
            total += N - 1
            miss += bad.size
            for i in bad:
                lo, hi = sorted((int(ref[i]), int(got[i])))
                assert np.all(w[lo + 1:hi] == 0) or hi - lo == 1
    return miss, total


@pytest.mark.parametrize("spec", M.FP32_SPECS, ids=[s.name for s in M.FP32_SPECS])
def test_multidim_program_fp32_log_weights_against_fp64_truth(spec):
    """fp32, N = 1024, 4 chains, T = 60: the fp64 literal's log-weight expression at the device's own stored fp32 particles against the device's log_ws.  The
    allowance is measured against the reference: the same NumPy literal evaluated in np.float32 on the same inputs deviates from its own fp64 value by at most
    e_ref; the device may deviate by 4 e_ref (another valid fp32 operation order differs by a small multiple, a wrong or missing term by O(1)).
    Measured (e_ref, device): range 1.593e-5, 1.593e-5; lorenz 6.298e-5, 6.346e-5."""
    nz, hist = _fp32_sweep(M.fp32_chains(spec))
    e_ref, e_dev = _teacher_forced_errors(spec, hist)
    print(f"{spec.name}: e_ref = {e_ref:.3e}, device = {e_dev:.3e}")
    assert e_dev <= 4 * e_ref, (e_dev, e_ref)


@pytest.mark.parametrize("spec", M.FP32_SPECS, ids=[s.name for s in M.FP32_SPECS])
def test_multidim_program_fp32_resampling_tie_rate(spec):
    """the same sweeps: at most 2e-4 of the resampling draws land on another particle than the literal fp32 order picks, each between neighbours or across
    zero-weight particles only (tests/test_user_model_literals.py: NumPy's own fp32 arithmetic meets this cap on these inputs).  Measured: range 29, lorenz 32 of
    241 428 draws (1.2e-4, 1.3e-4)."""
    nz, hist = _fp32_sweep(M.fp32_chains(spec))
    miss, total = _tie_rate(nz, hist)
    print(f"{spec.name}: {miss} of {total} draws differ")
    assert miss / total <= 2e-4, (miss, total)


_BOUND_FP32 = [c for c in _BOUND if c.proposal == "independent"]


@pytest.mark.parametrize("case", _BOUND_FP32, ids=_ids(_BOUND_FP32))
def test_program_bound_fallbacks_fp32(case):
    """the four kinds of bound in fp32 (4 chains), on the ordinary inputs -- where a loose but valid bound scales every weight by e^-50 and no fallback happens --
    and on the tightened ones (every shifted weight underflows at most steps): the stored log-weights within 4 e_ref of the fp64 literal at the device's own
    particles, and the resampling within the tie-rate cap.  Measured (e_ref, device), the same for the four bounds: ordinary range 5.826e-6, 5.847e-6; ordinary
    growth_nd 5.499e-5, 5.499e-5; tightened range 5.585e-3, 5.585e-3; tightened growth_nd 3.790e-2, 3.790e-2 (log-weights down to -2e3, residuals divided by
    sig = 0.02); 0 of 23 460 draws differ in all sixteen.  (The growth literal first computed its forcing term 8 cos(1.2 t) in fp64 whatever the precision of
    x; its "fp32" value was then better than any fp32 evaluation, e_ref = 9.9e-6, and the device's 5.5e-5 missed 4 e_ref.  user_models.growth_nd_mean now
    forms it in the precision of x.)"""
    chains = M.fp32_bound_chains(case)
    nz, hist = _fp32_sweep(chains)
    e_ref, e_dev = _teacher_forced_errors(case.spec, hist)
    miss, total = _tie_rate(nz, hist)
    print(f"{case.id}: e_ref = {e_ref:.3e}, device = {e_dev:.3e}; {miss} of {total} draws differ")
    assert e_dev <= 4 * e_ref, (e_dev, e_ref)
    assert miss / total <= 2e-4, (miss, total)
