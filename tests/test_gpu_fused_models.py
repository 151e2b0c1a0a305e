"""The fused chain-shared sweep (csrc/fused_shared.h, auxssm_kalman_sweep_fused) on the cases of tests/fused_cases.py: time-varying models with dy != dx (all
16 (D, PO) instantiations, packed and plain), missing rows and components under both NaN policies, a real accept / reject mix on a ping-pong pair that stays
mixed from sweep to sweep, the non-finite redo (fs_terms against fs_terms_fast), the chunk geometry of fs_chunk_len / fs_pack.

(a) against the oracle: three keyed fused sweeps per case, the lazy state read raw (never resolved, so the selector stays mixed); each checked chain's oracle
    sweep is driven from the device's own previous state and the noise of Handle.kalman_draw for the key -- oracle/kalman_np.py::kalman_sweep under the
    reference policy, fused_cases.masked_kalman_sweep under the masked one.
(b) against the keyed sweep it replaces (fused=False), same keys, from the same previous state, all chains.
(c) one chain with a NaN in its state: every other chain of its wave still meets (a) and (b) -- the redo under the per-term policy gives the numbers of the
    fast path -- and the NaN chain is rejected with its state untouched.
(d) the memoised model stage notices a new NaN pattern behind the same data pointer.  (e) host arrays take the same path through the `model=` layout hint.

fp64 bars are the project's (tests/test_gpu_fused.py): states 1e-9 / 1e-10, log terms 1e-9 relative, log alpha 1e-7.
fp32: states 2e-3; log alpha within FP32_MARGIN of the oracle; accept flags only for chains whose oracle margin |log alpha - log u| exceeds FP32_MARGIN.
FP32_MARGIN = 1.144e-4 = 4 x FP32_LOG_ALPHA_ERR = 4 x 2.86e-5, the largest |log alpha(unfused fp32 keyed sweep) - log alpha(oracle)| measured over the fp32 runs
of these cases on an MI355X (tests/fused_cases.py holds both figures; every run prints its own).  fp32 log terms other than log alpha are held to the keyed
sweep (b), not to the oracle."""
import functools

import numpy as np
import numpy.testing as npt
import pytest

from tests import fused_cases as FC

pytestmark = pytest.mark.gpu

F64 = dict(rtol=1e-9, atol=1e-10)
F32 = dict(rtol=2e-3, atol=2e-3)


def _kernel(model, policy):
    from aux_ssm_samplers_amd.kalman.generic import _get_device_kernel
    return _get_device_kernel(model, True, nan_policy=policy)[1]


def _same_bits(a, b):
    return np.array_equal(a, b, equal_nan=True)


@functools.lru_cache(maxsize=None)
def fused_run(case, dtname, policy, variant=None):
    """three fused keyed sweeps of the case on a lazy state that is never resolved; per sweep a dict of host arrays: prev / prop / new (C, T, d) -- the state
    before, the proposal (the buffer the chain did not live in) and the state after, gathered by the selector --, sel_old, sel_new, accepted, logs, the noise of
    kalman_draw for the key (ea, es, ua) and the UNFUSED keyed sweep of the same key from `prev` (unf_x, unf_acc, unf_logs).
    variant ("mid" | "first"): one NaN planted in the state of case.nan_chain."""
    from aux_ssm_samplers_amd import _lib, random as R
    from aux_ssm_samplers_amd.kalman.generic import DeviceChains, KalmanSampler
    h = _lib.default_handle()
    dtype = np.dtype(dtname).type
    model = case.model()
    kernel = _kernel(model, policy)
    x0 = case.x0.astype(dtype)
    if variant is not None:
        x0[case.nan_chain, case.nan_row(variant), case.d - 1] = np.nan
    a = DeviceChains(h, x0, chain_minor=True)
    gather = lambda xa, xb, sel: np.ascontiguousarray(np.where(sel[None, None, :] != 0, xb, xa).transpose(2, 0, 1))
    prev, sel_old, out = x0, np.zeros(case.C, np.int32), []
    for i, delta in enumerate(FC.DELTAS):
        key = case.key(i)
        kernel(key, KalmanSampler(x=a, updated=None), delta)
        assert a.fused is True
        xa, xb, sel = a._x.to_host(), a.x_alt.to_host(), a.sel.to_host()     # raw: no resolve, the selector stays as the sweep left it
        rec = dict(prev=prev, sel_old=sel_old, sel_new=sel, accepted=a.accepted.to_host(), logs=a.logs.to_host(), delta=delta,
                   prop=gather(xa, xb, 1 - sel_old), new=gather(xa, xb, sel))
        b = DeviceChains(h, prev, chain_minor=True, fused=False)
        kernel(key, KalmanSampler(x=b, updated=None), delta)
        assert b.fused is False
        rec.update(unf_x=b.to_host(), unf_acc=b.accepted.to_host(), unf_logs=b.logs.to_host())
        k_aux, k_samp, k_acc = R.split(key, 3)
        h.kalman_draw(k_aux, k_samp, k_acc, b.eps_aux, b.eps_samp, b.u_acc)
        rec.update(ea=b.stats_to_host(b.eps_aux), es=b.stats_to_host(b.eps_samp), ua=b.u_acc.to_host(), oracle={})
        out.append(rec)
        prev, sel_old = rec["new"], sel
    return out


def _oracle(case, policy, rec, c):
    """chain c's oracle sweep from the device's previous state on the device's noise (fp64 arithmetic whatever the device's dtype), once per run"""
    if c not in rec["oracle"]:
        f8 = lambda v: np.asarray(v, np.float64)
        r = case.oracle_sweep(policy, f8(rec["prev"][c]), rec["delta"], f8(rec["ea"][c]), f8(rec["es"][c]), float(rec["ua"][c]))
        r["margin"] = float(FC.margin(r["log_alpha"], rec["ua"][c]))
        rec["oracle"][c] = r
    return rec["oracle"][c]


def _check_bookkeeping(case, run, skip=()):
    """what holds for EVERY chain whatever the numbers: the selector flips exactly for accepted chains, a rejected chain's state is its previous state bit for bit"""
    for i, rec in enumerate(run):
        npt.assert_array_equal(rec["sel_new"], rec["sel_old"] ^ rec["accepted"], err_msg=f"sweep {i}")
        assert set(np.unique(rec["accepted"])) <= {0, 1}
        for c in np.flatnonzero(rec["accepted"] == 0):
            assert _same_bits(rec["new"][c], rec["prev"][c]), (i, c)


def _check_against_oracle(case, dtname, policy, run, chains):
    f64 = dtname == "float64"
    tol = F64 if f64 else F32
    worst, worst_unf, compared, total = 0.0, 0.0, 0, 0
    for i, rec in enumerate(run):
        for c in chains:
            ref = _oracle(case, policy, rec, c)
            msg = f"{case.id} {dtname} {policy} sweep {i} chain {c}"
            npt.assert_allclose(rec["prop"][c], ref["x_prop"], err_msg=msg, **tol)
            err = abs(float(rec["logs"][c, 0]) - ref["log_alpha"])
            worst, worst_unf = max(worst, err), max(worst_unf, abs(float(rec["unf_logs"][c, 0]) - ref["log_alpha"]))
            total += 1
            if f64:
                assert err < 1e-7, (msg, err)
                npt.assert_allclose(rec["logs"][c, 1:], [ref["lp_prop"], ref["lp_rev"], ref["lt_prop"], ref["lt_rev"]], rtol=1e-9, err_msg=msg)
            else:
                assert err <= FC.FP32_MARGIN, (msg, err)
                if ref["margin"] <= FC.FP32_MARGIN:
                    continue
            compared += 1
            assert bool(rec["accepted"][c]) == ref["accepted"], (msg, float(rec["logs"][c, 0]), ref["log_alpha"], float(np.log(rec["ua"][c])))
            npt.assert_allclose(rec["new"][c], ref["x"], err_msg=msg, **tol)
    print(f"{case.id} {dtname} {policy}: max |log alpha - oracle| fused {worst:.3g}, unfused keyed sweep {worst_unf:.3g}; flags compared {compared} of {total}")
    return worst_unf


def _check_against_unfused(case, dtname, policy, run, chains, flag_chains):
    """(b): chains -- the chains compared (all but a NaN chain); flag_chains -- fp32 only: those whose flags are compared (subject to the oracle margin)"""
    f64 = dtname == "float64"
    tol = F64 if f64 else F32
    chains = np.asarray(chains)
    for i, rec in enumerate(run):
        msg = f"{case.id} {dtname} {policy} sweep {i}"
        la, lb = rec["logs"][chains], rec["unf_logs"][chains]
        scale = np.abs(lb[:, 1:]).max()
        npt.assert_allclose(la[:, 1:], lb[:, 1:], rtol=0, atol=(1e-12 if f64 else 2e-6) * scale, err_msg=msg)
        if f64:
            npt.assert_array_equal(rec["accepted"][chains], rec["unf_acc"][chains], err_msg=msg)
            assert np.abs(la[:, 0] - lb[:, 0]).max() < 1e-7, msg
            same = chains
        else:
            for c in flag_chains:
                if _oracle(case, policy, rec, c)["margin"] > FC.FP32_MARGIN:
                    assert rec["accepted"][c] == rec["unf_acc"][c], (msg, c)
            same = chains[rec["accepted"][chains] == rec["unf_acc"][chains]]
            assert len(same) * 8 >= 7 * len(chains), msg
        npt.assert_allclose(rec["new"][same], rec["unf_x"][same], err_msg=msg, **tol)


# ---- (a) -----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", FC.RUNS, ids=FC.run_id)
def test_fused_sweeps_equal_the_oracle_on_a_mixed_lazy_state(run):
    """FP32_LOG_ALPHA_ERR (tests/fused_cases.py) is the largest `unfused keyed sweep` figure this test prints over the fp32 runs"""
    case, dtname, policy = run
    res = fused_run(case, dtname, policy)
    _check_bookkeeping(case, res)
    _check_against_oracle(case, dtname, policy, res, case.checked)
    if policy == "masked":   # the proposal is the exact posterior: log alpha = 0, every chain accepted
        for rec in res:
            assert np.abs(rec["logs"][:, 0]).max() < 1e-7 and rec["accepted"].all()
    else:
        assert set(np.unique(res[1]["sel_old"])) == {0, 1}     # the second sweep reads a genuinely mixed ping-pong pair
        assert 2 <= res[0]["accepted"][case.checked].sum() <= len(case.checked) - 2


# ---- (b) -----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", FC.RUNS, ids=FC.run_id)
def test_fused_sweeps_equal_the_keyed_sweep_they_replace(run):
    """same keys, fused=False, from the same previous state, all chains: the state 1e-9 / 1e-10 (fp32 2e-3), the four totals 1e-12 (fp32 2e-6) of their scale,
    fp64 flags identical.  fp32 flags: only for chains whose oracle margin |log alpha - log u| exceeds 1.144e-4 = 4 x 2.86e-5, the largest
    |log alpha(unfused fp32 keyed sweep) - log alpha(oracle)| measured over the fp32 runs of these cases and of the NaN-chain variants on an MI355X (the fused
    sweep's own figure there: 3.23e-5); the seeds keep every checked chain's margin above 1e-3 (tests/test_fused_cases.py), so none drops out."""
    case, dtname, policy = run
    _check_against_unfused(case, dtname, policy, fused_run(case, dtname, policy), np.arange(case.C), case.checked)


# ---- (c) -----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["mid", "first"])
@pytest.mark.parametrize("policy", ["reference", "masked"])
@pytest.mark.parametrize("dtname", ["float64", "float32"])
@pytest.mark.parametrize("case", FC.NAN_CASES, ids=[c.id for c in FC.NAN_CASES])
def test_a_non_finite_chain_leaves_the_rest_of_its_wave_exact(case, dtname, policy, variant):
    """the wave's ballot sends every chain of the NaN chain's wave through fs_terms at the steps the NaN touches, in pass AC (the current state) and -- because
    the chain's proposal is not finite either -- in pass E; their numbers must be those of fs_terms_fast: the bars of (a) and (b) for every other chain of the wave"""
    res = fused_run(case, dtname, policy, variant)
    nc = case.nan_chain
    others = [c for c in case.nan_wave if c != nc]
    _check_bookkeeping(case, res)
    _check_against_oracle(case, dtname, policy, res, others)
    _check_against_unfused(case, dtname, policy, res, [c for c in range(case.C) if c != nc], others)
    for i, rec in enumerate(res):
        assert np.isnan(rec["logs"][nc, 0]) and rec["accepted"][nc] == 0 and rec["sel_new"][nc] == 0, i
        assert _same_bits(rec["new"][nc], res[0]["prev"][nc]) and np.isnan(rec["new"][nc]).sum() == 1, i
        # what the NaN chain still reports does not involve the marginal likelihood: the two targets and lp_rev - lp_prop (the difference of the two joint
        # densities, each summed under the per-term policy) are those of the keyed sweep at the bars of (b)
        fa, un = rec["logs"][nc].astype(np.float64), rec["unf_logs"][nc].astype(np.float64)
        print(f"{case.id} {dtname} {policy} {variant} sweep {i}: NaN chain logs fused {fa} keyed {un}")
        scale = np.abs(rec["unf_logs"][others][:, 1:]).max()
        npt.assert_allclose([fa[3], fa[4], fa[2] - fa[1]], [un[3], un[4], un[2] - un[1]], rtol=0, atol=(1e-12 if dtname == "float64" else 2e-6) * scale, equal_nan=True)
        assert np.isfinite(fa[3:]).all()


# ---- (d) -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_model_stage_memo_notices_a_new_nan_pattern_behind_the_same_pointer():
    """tests/test_gpu_device_delta.py::test_model_stage_memo_is_exact on missing data: eight sweeps at a fixed step size (from the fourth on the memoised model stage
    is skipped), the data rewritten in place before the sixth with the SAME values where both are observed and a different NaN pattern: bit for bit the run with
    the stage on the one stream, which has nothing to memoise"""
    from aux_ssm_samplers_amd import _lib
    from aux_ssm_samplers_amd.kalman.generic import DeviceChains, KalmanSampler
    h = _lib.default_handle()
    case = FC.GROUP_A[9]   # (3, 2)
    y2 = FC.missing(case.m["y"], {3: "whole", case.E: "whole", case.T - 2: "partial"}, np.random.default_rng(77))
    assert not np.array_equal(np.isnan(y2), np.isnan(case.y))

    def run(overlap):
        h.set_option(_lib.OPT_OVERLAP_MODEL_STAGE, overlap)
        model = case.model()
        kernel = _kernel(model, "reference")
        ch = DeviceChains(h, case.x0, chain_minor=True)
        ybuf = model.device(h, np.float64)[1]
        out = []
        for i in range(8):
            if i == 5:
                ybuf.copy_from_host(np.ascontiguousarray(y2).reshape(ybuf.shape))
            kernel(case.key(i), KalmanSampler(x=ch, updated=None), 0.4)
            assert ch.fused is True
            out.append((ch.to_host(), ch.accepted.to_host(), ch.logs.to_host()))
        return out

    try:
        a = run(1)
        b = run(0)
    finally:
        h.set_option(_lib.OPT_OVERLAP_MODEL_STAGE, 1)
    for u, v in zip(a, b):
        for p, q in zip(u, v):
            npt.assert_array_equal(p, q)
    assert 0 < sum(int(u[1].sum()) for u in a) < 8 * case.C


# ---- (e) -----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [FC.GROUP_A[9], FC.GROUP_A[7]], ids=lambda c: c.id)
def test_host_arrays_take_the_fused_sweep_through_the_layout_hint(case):
    from aux_ssm_samplers_amd import _lib
    from aux_ssm_samplers_amd.kalman import get_kernel
    from aux_ssm_samplers_amd.kalman.generic import DeviceChains, KalmanSampler
    h = _lib.default_handle()
    model = case.model()
    init, kernel = get_kernel(model.dynamics_factory, model.observations_factory, model.log_likelihood_fn, True)
    x0 = np.array(case.x0)
    assert x0.shape == (6, 70, case.d) and DeviceChains(h, x0, model=model).chain_minor and not DeviceChains(h, x0).chain_minor
    out = kernel(case.key(0), init(x0), FC.DELTAS[0])
    ch = DeviceChains(h, x0, chain_minor=True)
    kernel(case.key(0), KalmanSampler(x=ch, updated=None), FC.DELTAS[0])
    assert ch.fused is True
    npt.assert_array_equal(out.logs, ch.logs.to_host())
    npt.assert_array_equal(out.updated, ch.accepted.to_host().astype(bool))
    npt.assert_array_equal(out.x, ch.to_host())
    assert 0 < out.updated.sum() < case.C


def test_device_noise_restates_the_draws_of_the_sweep():
    """fused_cases.device_noise (the input of the CPU conditions) against Handle.kalman_draw: uniforms bit for bit, fp64 normals to the tolerance oracle/rng_np.py states"""
    from aux_ssm_samplers_amd import _lib, random as R
    from aux_ssm_samplers_amd.kalman.generic import DeviceChains
    h = _lib.default_handle()
    case = FC.GROUP_B[4]
    b = DeviceChains(h, case.x0, chain_minor=True, fused=False)
    k_aux, k_samp, k_acc = R.split(case.key(2), 3)
    h.kalman_draw(k_aux, k_samp, k_acc, b.eps_aux, b.eps_samp, b.u_acc)
    ea, es, ua = FC.device_noise(case, 2)
    npt.assert_array_equal(b.u_acc.to_host(), ua)
    npt.assert_allclose(b.stats_to_host(b.eps_aux), ea, rtol=1e-12, atol=1e-13)
    npt.assert_allclose(b.stats_to_host(b.eps_samp), es, rtol=1e-12, atol=1e-13)
