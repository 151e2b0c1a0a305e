"""The wide-state cSMC kernels (csrc/csmc_wide.hip, 4 < dx <= 32, N <= 64) with MORE CHAINS THAN CUs.

run_cw picks the kernels from the chain count: fp32 with no more chains than CUs runs sixteen waves per chain (k_cw2_fwd<float, 16, false, V>, k_cw2_bwd<float, 16>),
more chains -- and fp64 always -- eight (k_cw2_fwd<R, 8, false, V>, k_cw2_bwd<R, 8>); guided proposals run k_cw2_fwd<R, 8, true, V> whatever the count.  Particle
i = 2 NW2 s + 2 wave + half lives in pass s of ceil(N / (2 NW2)), so the two fp32 instantiations differ in their passes (N = 25: one against two, the second ragged;
N = 64: two against four), in the LDS rows, the in-kernel Threefry indices and the backward kernel's register rows.  Every other test of this path runs 1 to 5 chains
in fp32 (sixteen waves) or is fp64; here C_hi = CUs + 3 chains in fp32, the CU count read from the device as the library reads it:

1. the eight-wave fp32 kernels against the contract oracle (oracle/csmc_ref.c), bit for bit, chain by chain: both proposals, both backward modes, the four
   separable potentials (the masked one included), gradient proposals in both weightings, time-varying transitions, and the underflow fallback of the bound;
2. (the masked potential at few chains: tests/test_gpu_csmc.py::test_wide_state_sweep_bit_exact_vs_oracle);
3. the coupled potentials (multivariate-t, linear-Gaussian) and guided proposals, which no contract oracle covers in fp32: one launch of C_hi chains (eight waves)
   against the same chains as launches of CUs and 3 chains (sixteen waves, held by the fp64 literal and the tie-rate rule at 4 chains), bit for bit -- the kernels'
   header says every ordered operation keeps its order whatever NW2;
4. in-kernel draws (keyed == explicit, and the first chains of a C_hi-chain keyed sweep == a keyed sweep of those chains alone) and chain batching with offsets
   beyond the CU count."""
import functools

import numpy as np
import pytest

from oracle import csmc as O
from tests import guided_np as G
from tests import lingauss_np as LG
from tests import mvt_np as MV
from tests import potential_gpu as GP
from tests.test_csmc_gradient_timevarying import _tv_model
from tests.test_gpu_csmc import _masked_obs, _models, _pot

pytestmark = pytest.mark.gpu

FIELDS, _cu, _inputs, _assert_same, _sweep = GP.FIELDS, GP.cu_count, GP.chain_inputs, GP.assert_same, GP.sweep_fields


# ---- 1. against the contract oracle ------------------------------------------------------------------------------------------------------------------------
B, I = O.BOOTSTRAP_LG, O.AUX_INDEPENDENT
FLAT, GAUSS, SV, MASKED = O.POT_FLAT, O.POT_GAUSS_OBS, O.POT_SV, O.POT_GAUSS_OBS_MASKED
S_RAGGED, S_SV, S_FULL4, S_ONE, S_ALONE, S_IDLE = (5, 25, 6), (30, 25, 6), (32, 64, 5), (8, 16, 5), (16, 17, 5), (16, 2, 4)
# (shape, proposal, potential, backward, variant).  The shapes: two passes with a ragged second and a narrow state; the SV protocol's d and N; four full passes with
# all 32 lanes of a half-wave; exactly one full pass; one particle alone in the second pass; one wave busy and seven idle.  Every (potential, proposal, backward)
# combination is here once, and every shape has both proposals.
ORACLE_CELLS = [
    (S_RAGGED, B, FLAT, True, None), (S_FULL4, B, FLAT, False, None), (S_ALONE, I, FLAT, True, None), (S_IDLE, I, FLAT, False, None),
    (S_SV, B, GAUSS, True, None), (S_ONE, B, GAUSS, False, None), (S_FULL4, I, GAUSS, True, None), (S_RAGGED, I, GAUSS, False, None),
    (S_ALONE, B, SV, True, None), (S_IDLE, B, SV, False, None), (S_SV, I, SV, True, None), (S_ONE, I, SV, False, None),
    (S_SV, B, MASKED, True, None), (S_ALONE, B, MASKED, False, None), (S_RAGGED, I, MASKED, True, None), (S_FULL4, I, MASKED, False, None),
    # gradient-informed independent proposals in both weightings (tests/test_csmc_gradient_timevarying.py's construction: small steps, backward sampling)
    (S_SV, I, SV, True, "grad_reference"), (S_SV, I, GAUSS, True, "grad_exact"), (S_RAGGED, I, GAUSS, True, "grad_reference"), (S_RAGGED, I, SV, True, "grad_exact"),
    # time-varying transitions F_t, b_t, chol Q_t (that file's construction: the Gaussian-observation potential)
    (S_SV, B, GAUSS, True, "tv"), (S_SV, I, GAUSS, False, "tv"), (S_RAGGED, I, GAUSS, True, "tv"), (S_RAGGED, B, GAUSS, False, "tv"),
    # an observation noise so small that on some steps every weight underflows under the bound c_obs: the `!(tot > 0)` fallback to the exact maximum
    (S_SV, B, GAUSS, True, "tight"),
]
TIGHT_SIG = 0.55  # (at d = 30: about a quarter of the interior steps lose every forward weight under the bound, a tenth every backward weight only)
_POT_NAME = {FLAT: "flat", GAUSS: "gauss", SV: "sv", MASKED: "masked"}


def _cell_id(cell):
    (d, N, T), proposal, potential, backward, variant = cell
    return f"d{d}-N{N}-T{T}-{'independent' if proposal == I else 'bootstrap'}-{_POT_NAME[potential]}-{'backward' if backward else 'trace'}" + (f"-{variant}" if variant else "")


@pytest.mark.parametrize("cell", ORACLE_CELLS, ids=_cell_id)
def test_more_chains_than_cus_fp32_bit_exact_vs_oracle(cell):
    """k_cw2_fwd<float, 8, false, SEP> and k_cw2_bwd<float, 8> at C_hi = CUs + 3 chains: particles, log-weights, resampling ancestors, backward indices and the
    trajectory of EVERY chain bit-exact against the contract oracle (the bars and the oracle of test_gpu_csmc.py::test_wide_state_sweep_bit_exact_vs_oracle); row 0
    of every step is the reference trajectory; at least one chain moves.  tight: at least one interior step of one chain has every weight below the exp underflow
    under its bound (read off the returned log-weights and c_obs, as test_gpu_csmc.py's tight_obs case does), and at least one more has weights that survive the
    bound in the forward pass but not once the backward pass has added the transition density (the backward kernel's fallback)."""
    from aux_ssm_samplers_amd import _lib
    from aux_ssm_samplers_amd.csmc import _device, GaussianInit, LinearGaussianDynamics
    (d, N, T), proposal, potential, backward, variant = cell
    Cn = _cu() + 3
    seed = ORACLE_CELLS.index(cell)
    rng = np.random.default_rng([1, seed])
    sig = TIGHT_SIG if variant == "tight" else 0.7
    if variant == "tv":
        F, b, Q = _tv_model(T, d, rng)
        M0, Mt = GaussianInit(m0=0.1 * rng.standard_normal(d), P0=2.0 * np.eye(d)), LinearGaussianDynamics(F=F, b=b, Q=Q)
        assert Mt.time_varying
        LQ = np.linalg.cholesky(Q)
        od = dict(F=F[0], b=b[0], chol_Q=LQ[0], F_t=F, b_t=b, chol_Q_t=LQ)
    else:
        M0, Mt = _models(d, rng)
        od = dict(F=Mt.F, b=Mt.b, chol_Q=Mt.chol())
    y = rng.standard_normal((T, d))
    if potential == MASKED:
        y = _masked_obs(y, rng, (0, T // 2, T - 1)[seed % 3])
        assert np.isnan(y).all(axis=1).sum() >= 1 and all(0 < np.isnan(y[t]).sum() for t in (0, T // 2, T - 1))
    G0, Gt = _pot(potential, y, sig)
    gmode = {"grad_reference": _lib.GRAD_REFERENCE, "grad_exact": _lib.GRAD_EXACT}.get(variant, _lib.GRAD_NONE)
    od.update(proposal=proposal, potential=potential, m0=M0.m0, chol_P0=M0.chol(), sig_y=sig, gradient=gmode)
    nz = dict(_inputs(100 + seed, Cn, T, N, d))
    x0 = nz.pop("x0")
    delta, okw = None, [{} for _ in range(Cn)]
    if proposal == I:
        delta = (0.05 + 0.1 * rng.random(T)) if gmode else (0.5 + rng.random(T))
        fk = _device.describe_independent(M0, G0, Mt, Gt, Mt, gmode)
        okw = [dict(sqrt_half_delta=np.sqrt(0.5 * delta), eps_aux=nz["eps_aux"][c]) for c in range(Cn)]
    else:
        nz.pop("eps_aux")
        fk = _device.describe_bootstrap(M0, G0, Mt, Gt, Mt)
    got = _sweep(fk, x0, N, backward, nz, delta)
    refs = [O.sweep(od, x0[c], N, backward, y=y if potential else None, eps_prop=nz["eps_prop"][c], u_res=nz["u_res"][c], u_bwd=nz["u_bwd"][c],
                    dtype=np.float32, **okw[c]) for c in range(Cn)]
    for name in FIELDS:
        _assert_same(got[name], np.stack([r[name] for r in refs]), f"{_cell_id(cell)} {name}, device against oracle")
    assert np.all(got["As"][:, :, 0] == 0) and np.array_equal(got["xs"][:, :, 0], x0)
    assert (got["ancestors"] != 0).any()
    if gmode:  # (the proposals really are the shifted ones)
        plain = _sweep(_device.describe_independent(M0, G0, Mt, Gt, Mt), x0[:2], N, backward, {k: v[:2] for k, v in nz.items()}, delta)
        assert np.max(np.abs(plain["xs"][:, :, 1:] - got["xs"][:2, :, 1:])) > 0
    if variant == "tight":
        lw = got["log_ws"].astype(np.float64)
        c_obs = d * (-np.log(sig) - 0.5 * np.log(2 * np.pi))  # the bound of a bootstrap step: sup_x g_t(x)
        top = (lw[:, 1:-1] - c_obs).max(axis=2)               # (chain, interior step): the largest shifted log-weight
        under = top < -104
        print(f"tight: {int(under.sum())} of {under.size} interior (chain, step) pairs have every forward weight below the exp underflow under the bound")
        assert under.any()
        # the backward weights of step t: log N(x_{t+1}; F x_t^i + b, Q) + lw_t^i, shifted by the forward pass's shift + the transition's constant; where the forward
        # weights survived their bound with room to spare (shift = c_obs) yet no sum does, the backward kernel falls back (det_exp flushes below -87.3)
        LQ = np.asarray(Mt.chol(), np.float64)
        xs, xn = got["xs"].astype(np.float64), got["x"].astype(np.float64)
        r = xn[:, 2:, None, :] - (xs[:, 1:-1] @ np.asarray(Mt.F, np.float64).T + np.asarray(Mt.b, np.float64))
        z = np.linalg.solve(LQ, r.reshape(-1, d).T).T.reshape(r.shape)
        both = (top > -80) & ((lw[:, 1:-1] - c_obs - 0.5 * np.sum(z * z, axis=-1)).max(axis=2) < -95)
        print(f"tight: {int(both.sum())} pairs keep a forward weight under the bound and lose every backward weight")
        assert both.any()


# ---- 3. coupled potentials and guided proposals: one launch against split launches ---------------------------------------------------------------------
# (style, gradient, backward): the independent style in both backward modes
SPLIT_STYLES = [("bootstrap", False, False), ("independent", False, True), ("independent", False, False), ("independent", "exact", True), ("guided", True, True)]


@functools.lru_cache(maxsize=None)
def _coupled_case(kind, d, dy, T):
    rng = np.random.default_rng([3, d, T])
    if kind == "mvt":
        dev, _, xtrue, delta = MV.case(d, T, rng, nan_rows=(T // 2,))
    elif kind == "lingauss":
        dev, m, xtrue, delta = LG.case(d, dy, T, rng, nan_rows=(T // 2,))
        assert np.isnan(m.y).any(axis=1).sum() == 1
    else:
        dev, _, xtrue, delta = G.sv_case(d, T, rng)
    return dev, xtrue, delta


def _one_launch_equals_split_launches(kind, d, dy, N, T, style, gradient, backward):
    """-> the number of trajectory entries that moved"""
    dev, xtrue, delta = _coupled_case(kind, d, dy, T)
    what = f"{kind} d={d} N={N} T={T} {style} gradient={gradient} backward={backward}"
    return GP.one_launch_equals_sixteen_wave(GP.describe(style, dev, gradient), style, xtrue, delta, N, backward, what)


@pytest.mark.parametrize("style,gradient,backward", SPLIT_STYLES)
@pytest.mark.parametrize("d,N,T", [(9, 25, 8), (32, 64, 5)])
def test_multivariate_t_one_launch_equals_sixteen_wave_launches(d, N, T, style, gradient, backward):
    """k_cw2_fwd<float, 8, false, MVT> / k_cw2_bwd<float, 8> against the sixteen-wave instantiations; guided: the forward kernel has eight waves on both sides, the
    backward kernels differ"""
    assert _one_launch_equals_split_launches("mvt", d, 0, N, T, style, gradient, backward) > 0


@pytest.mark.parametrize("style,gradient,backward", SPLIT_STYLES)
@pytest.mark.parametrize("d,dy,N,T", [(9, 4, 25, 8), (24, 12, 33, 6)])
def test_linear_gaussian_one_launch_equals_sixteen_wave_launches(d, dy, N, T, style, gradient, backward):
    """k_cw2_fwd<float, 8, false, LIN> / k_cw2_bwd<float, 8> against the sixteen-wave instantiations; one observation row has a NaN (a flat step)"""
    assert _one_launch_equals_split_launches("lingauss", d, dy, N, T, style, gradient, backward) > 0


@pytest.mark.parametrize("gradient", [False, True])
def test_guided_sv_backward_kernel_eight_waves_equals_sixteen(gradient):
    """the SV protocol's d and N through guided proposals: k_cw2_fwd<float, 8, true, SEP> on both sides, so this is k_cw2_bwd<float, 8> against <float, 16>"""
    assert _one_launch_equals_split_launches("sv", 30, 0, 25, 8, "guided", gradient, True) > 0


# ---- 4. in-kernel draws and batching -------------------------------------------------------------------------------------------------------------------------
def _sv_protocol_cell():
    from aux_ssm_samplers_amd.csmc import _device
    d, N, T = S_SV
    rng = np.random.default_rng(41)
    M0, Mt = _models(d, rng)
    G0, Gt = _pot(SV, rng.standard_normal((T, d)))
    return _device.describe_independent(M0, G0, Mt, Gt, Mt), d, N, T, 0.05 + 0.1 * rng.random(T)


def test_keyed_draws_equal_explicit_draws_and_do_not_depend_on_the_chain_count():
    """independent proposals, SV potential, (d, N, T) = (30, 25, 6), C_hi chains: the keyed sweep equals the explicit sweep on key_noise(wide=True) of the same key,
    and its first three chains equal a keyed sweep of three chains (the natural flat indices do not depend on C: the eight-wave kernel's draws against the
    sixteen-wave kernel's)"""
    from aux_ssm_samplers_amd import _lib, random as R
    from aux_ssm_samplers_amd.csmc import _device
    fk, d, N, T, delta = _sv_protocol_cell()
    Cn = _cu() + 3
    x0 = _inputs(400, Cn, T, N, d)["x0"]
    key = R.PRNGKey(2024)
    keyed = _sweep(fk, x0, N, True, None, delta, key=key)
    explicit = _sweep(fk, x0, N, True, _device.key_noise(_lib.default_handle(), key, Cn, T, N, d, np.float32, wide=True), delta)
    few = _sweep(fk, x0[:3], N, True, None, delta, key=key)
    for name in FIELDS:
        _assert_same(keyed[name], explicit[name], f"{name}, keyed against explicit draws at {Cn} chains")
        _assert_same(keyed[name][:3], few[name], f"{name}, chains [0, 3) of {Cn} keyed chains against 3 keyed chains")
    assert (keyed["ancestors"] != 0).any() and len({keyed["x"][c].tobytes() for c in range(Cn)}) == Cn


@pytest.mark.parametrize("backward", [True, False])
@pytest.mark.parametrize("mode", ["keyed", "explicit"])
def test_batches_of_100_chains_equal_one_launch(mode, backward, monkeypatch):
    """the same sweep without history in batches of 100, 100 and the rest (AUXSSM_CSMC_BATCH): the kernel selection is made on the whole chain count, so every batch
    runs eight waves, with chain offsets c0 beyond the CU count"""
    from aux_ssm_samplers_amd import _lib, random as R
    from aux_ssm_samplers_amd.csmc import _device
    fk, d, N, T, delta = _sv_protocol_cell()
    Cn = _cu() + 3
    assert Cn > 200
    x0 = _inputs(400, Cn, T, N, d)["x0"]
    key = R.PRNGKey(2024)
    kw = dict(key=key) if mode == "keyed" else dict(noise=_device.key_noise(_lib.default_handle(), key, Cn, T, N, d, np.float32, wide=True))
    monkeypatch.delenv("AUXSSM_CSMC_BATCH", raising=False)
    xa, anca, _ = _device.sweep(fk, x0, N, backward, delta=delta, **kw)
    monkeypatch.setenv("AUXSSM_CSMC_BATCH", "100")
    xb, ancb, _ = _device.sweep(fk, x0, N, backward, delta=delta, **kw)
    _assert_same(xb, xa, "x, batches of 100 against one launch")
    _assert_same(ancb, anca, "ancestors, batches of 100 against one launch")
    assert (anca != 0).any()
