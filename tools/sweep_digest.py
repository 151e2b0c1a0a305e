#!/usr/bin/env python3
"""One SHA-256 per case over the bytes of (x, accepted, logs) after consecutive keyed sweeps of a fixed list of small problems: every branch a driver of
the auxiliary Kalman sweep can take (csrc/api.hip: sweep_lg_concat, sweep_lg_concat_fused, sweep_lorenz, sweep_mvt and sweep_ss -- the state-space driver of the
SV, Poisson, logistic and Poisson-linear kinds), every model kind of include/auxssm.h (1-8, 11-14), in both dtypes.  For comparing two builds of the library bit for bit:
    AUXSSM_LIB=/path/to/libauxssm.so python tools/sweep_digest.py out.json        once per build, then compare the files.
A case that raises is recorded with the error's text, and the exit status is 1: two equal error strings compare equal and prove nothing.

    python tools/sweep_digest.py --host out.json        needs no GPU: one SHA-256 per built-in model class, order and dtype over everything dynamics_factory,
observations_factory and log_likelihood_fn return at a fixed (x, u, delta) on data with missing entries -- the NumPy factories the host path and the oracle run.
The two densities the models take from the device primitives (prior_logpdf, joint_logpdf) are the NumPy oracle's there.  Run it from a checkout of each of the
two trees to compare (it imports the package beside it)."""
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aux_ssm_samplers_amd import _lib, random as R  # noqa: E402
from aux_ssm_samplers_amd.kalman import (BinomialModel, DeviceChains, KalmanSampler, LGConcatModel, LorenzModel, MVTModel, NegBinomialModel,  # noqa: E402
                                         PoissonLinearModel, PoissonModel, SVModel, get_kernel)
from aux_ssm_samplers_amd.workloads import lg_model, logistic_kalman_setup, lorenz_kalman_setup, poisson_lin_setup, poisson_setup, sv_setup  # noqa: E402


def lg(T, d, tinv=False):
    """the benchmark's linear-Gaussian model; d = 6: the same recipe on 0.9 I dynamics (the wide-state path).  tinv: broadcast views, time stride 0"""
    if d <= 4:
        m = lg_model(T, d)
    else:
        rng = np.random.default_rng(d)
        m = dict(m0=np.zeros(d), P0=np.eye(d), F=0.9 * np.eye(d) + 0.02 * rng.standard_normal((d, d)), Q=0.1 * np.eye(d), b=np.zeros(d),
                 Hobs=np.eye(d), Robs=0.5 * np.eye(d), cobs=np.zeros(d), y=rng.standard_normal((T, d)))
    rep = (lambda a, n: np.broadcast_to(a, (n,) + a.shape)) if tinv else (lambda a, n: np.ascontiguousarray(np.broadcast_to(a, (n,) + a.shape)))
    return LGConcatModel(m["m0"], m["P0"], rep(m["F"], T - 1), rep(m["Q"], T - 1), rep(m["b"], T - 1), rep(m["Hobs"], T), rep(m["Robs"], T),
                         rep(m["cobs"], T), m["y"]), 0.4


def lg_missing(policy_tinv):
    """a time-varying (3, 2) model with missing rows and components (tests/fused_cases.py::tv_model, group A's shape) -- or, tinv, one step's matrices as
    broadcast views under the same kind of data: the fused sweep outside workloads.lg_model"""
    from tests import fused_cases as FC
    m = FC.tv_model(70, 3, 2, 2, tinv=policy_tinv)
    y = FC.missing(m["y"], {0: "partial", 15: "whole", 16: "partial", 69: "whole"}, np.random.default_rng(5))
    return LGConcatModel(m["m0"], m["P0"], m["Fs"], m["Qs"], m["bs"], m["Hs"], m["Rs"], m["cs"], y), 0.4


def sv(T, d, order):
    y, _, (m0, P0, F, Q, b) = sv_setup(T, d)
    return SVModel(y, m0, P0, F, Q, b, order=order), 0.05


def lorenz(T, C=None):
    """C: one theta per chain"""
    base, _ = lorenz_kalman_setup(max(T, 9), every=4, dt=1e-3)
    theta = base.theta if C is None else base.theta * (1 + 0.01 * np.arange(C))[:, None]
    return LorenzModel(base.yobs[:T], base.Hobs[:T], base.Robs[:T], base.cobs[:T], base.m0, base.P0, theta, base.sigma_x, base.dt), 1e-3


def holes(y, channel=None):
    """missing entries: one at t = 0, a whole middle row and one at T - 1 where T > 3; channel: that column everywhere"""
    y = np.array(y, np.float64)
    T = y.shape[0]
    y[0, 0] = np.nan
    if T > 3:
        y[T // 2] = np.nan
        y[T - 1, -1] = np.nan
    if channel is not None:
        y[:, channel] = np.nan
    return y


def pois(T, d, order):
    M0, Mt, _, _, _, y = poisson_setup(T, d)
    return PoissonModel(holes(y), M0.m0, M0.P0, Mt.F, Mt.Q, Mt.b, order=order), 0.05


def logit(T, d, order, family):
    """binomial (trials 1 .. 40, a binary component) or negative-binomial (r = 3) data with missing entries; the size under a missing entry is NaN"""
    base, _ = logistic_kalman_setup(T, d, family)
    y = holes(base.yobs)
    dyn = (base.m0, base.P0, base.F, base.Q, base.b)
    if family == "binomial":
        return BinomialModel(y, np.where(np.isnan(y), np.nan, base.trials), *dyn, order=order), 0.05
    return NegBinomialModel(y, base.r, *dyn, order=order), 0.05


def plin(T, dx, dy, order, delta):
    """delta: of the order of 1 / lambda_max(H' diag(e) H), which the first-order proposal needs (PoissonLinearModel's docstring)"""
    base, _, H, c = poisson_lin_setup(T, dx, dy)
    y = holes(base.yobs, channel=dy - 2) if dy > 2 else base.yobs
    return PoissonLinearModel(y, H, c, base.m0, base.P0, base.F, base.Q, base.b, order=order), delta


def mvt(T, d, order):
    """a dense precision, nu = 3, diagonal dynamics that differ by component"""
    rng = np.random.default_rng(10 * d + T)
    A = rng.standard_normal((d, d))
    prec = 1.5 * np.eye(d) + 0.8 * (A @ A.T) / d
    y = np.cumsum(0.3 * rng.standard_normal((T, d)), axis=0) + 0.5 * rng.standard_normal((T, d))
    if T > 3:
        y[T // 2, (d - 1) // 2] = np.nan
    return MVTModel(y, 0.1 * rng.standard_normal(d), 0.5 + rng.random(d), 0.9 + 0.1 * rng.random(d), 0.1 * (0.5 + rng.random(d)), 0.05 * rng.standard_normal(d),
                    3.0, prec, order=order), 0.1


# name: (model, chains, chain-minor, options {share, overlap, parallel, fused, moments, sweeps, nan_policy})
CASES = {
    "lg_dense_parallel": (lambda: lg(40, 2), 3, False, {}),
    "lg_dense_sequential": (lambda: lg(40, 2), 3, False, dict(parallel=False)),
    "lg_dense_time_invariant_obs": (lambda: lg(40, 2, tinv=True), 3, False, {}),
    "lg_cm_shared_in_pass_noise": (lambda: lg(400, 2), 64, True, {}),
    "lg_cm_shared_time_invariant_obs": (lambda: lg(400, 2, tinv=True), 64, True, {}),
    "lg_cm_shared_overlap": (lambda: lg(400, 2), 64, True, dict(overlap=1, sweeps=5)),
    "lg_cm_packed_covariances": (lambda: lg(40, 2), 64, True, dict(share=0)),
    "lg_wide_one_chain": (lambda: lg(12, 6), 1, False, {}),
    "lg_wide_carrier": (lambda: lg(12, 6), 3, False, {}),
    "lg_fused": (lambda: lg(64, 4), 66, True, dict(fused=None, overlap=1, sweeps=5)),
    "lg_fused_moments": (lambda: lg(64, 4), 66, True, dict(fused=None, overlap=1, sweeps=5, moments=True)),
    "lg_fused_tv_missing_reference": (lambda: lg_missing(False), 6, True, dict(fused=None, overlap=1, sweeps=5)),
    "lg_fused_tv_missing_masked": (lambda: lg_missing(False), 6, True, dict(fused=None, overlap=1, sweeps=5, nan_policy="masked")),
    "lg_fused_tinv_missing": (lambda: lg_missing(True), 6, True, dict(fused=None, overlap=1, sweeps=5)),
    "lorenz_dense": (lambda: lorenz(40), 3, False, {}),
    "lorenz_cm": (lambda: lorenz(40), 64, True, {}),
    "lorenz_cm_theta_per_chain": (lambda: lorenz(40, 64), 64, True, {}),
    "lorenz_one_step": (lambda: lorenz(1), 3, False, {}),
    "sv1_wide_gain_rows_reused": (lambda: sv(12, 6, 1), 3, False, {}),
    "sv1_cm_shared_overlap": (lambda: sv(40, 2, 1), 64, True, dict(overlap=1, sweeps=5)),
}
for o in (1, 2):
    CASES[f"sv{o}_dense"] = (lambda o=o: sv(40, 2, o), 3, False, {})
    CASES[f"sv{o}_cm_shared"] = (lambda o=o: sv(40, 2, o), 64, True, {})
    CASES[f"sv{o}_cm_array_free"] = (lambda o=o: sv(40, 2, o), 64, True, dict(share=0))
    CASES[f"sv{o}_wide_one_chain"] = (lambda o=o: sv(12, 6, o), 1, False, {})
    CASES[f"pois{o}_dense"] = (lambda o=o: pois(40, 2, o), 3, False, {})
    CASES[f"pois{o}_cm_shared"] = (lambda o=o: pois(40, 2, o), 64, True, {})
    CASES[f"pois{o}_cm_array_free"] = (lambda o=o: pois(40, 2, o), 64, True, dict(share=0))
    CASES[f"pois{o}_wide_one_chain"] = (lambda o=o: pois(12, 6, o), 1, False, {})
    for fam, tag in (("binomial", "binom"), ("negbinomial", "negbin")):
        CASES[f"{tag}{o}_dense"] = (lambda o=o, fam=fam: logit(40, 2, o, fam), 3, False, {})
        CASES[f"{tag}{o}_cm_shared"] = (lambda o=o, fam=fam: logit(40, 2, o, fam), 64, True, {})
        CASES[f"{tag}{o}_cm_array_free"] = (lambda o=o, fam=fam: logit(40, 2, o, fam), 64, True, dict(share=0))
        CASES[f"{tag}{o}_wide_one_chain"] = (lambda o=o, fam=fam: logit(12, 6, o, fam), 1, False, {})
    CASES[f"plin{o}_dense"] = (lambda o=o: plin(40, 2, 3, o, 0.05), 3, False, {})
    CASES[f"plin{o}_second_staging_block_ragged_chains"] = (lambda o=o: plin(40, 4, 70, o, 0.005), 5, False, {})
    CASES[f"plin{o}_one_step"] = (lambda o=o: plin(1, 2, 3, o, 0.05), 3, False, {})
    CASES[f"mvt{o}_d3"] = (lambda o=o: mvt(40, 3, o), 3, False, {})
    CASES[f"mvt{o}_d5"] = (lambda o=o: mvt(40, 5, o), 3, False, {})
    CASES[f"mvt{o}_one_step"] = (lambda o=o: mvt(1, 3, o), 3, False, {})
CASES["pois1_wide_gain_rows_reused"] = (lambda: pois(12, 6, 1), 3, False, {})
CASES["pois1_cm_shared_overlap"] = (lambda: pois(40, 2, 1), 64, True, dict(overlap=1, sweeps=5))
CASES["binom1_wide_gain_rows_reused"] = (lambda: logit(12, 6, 1, "binomial"), 3, False, {})
CASES["negbin1_cm_shared_overlap"] = (lambda: logit(40, 2, 1, "negbinomial"), 64, True, dict(overlap=1, sweeps=5))
CASES["binom2_dense_sequential"] = (lambda: logit(40, 2, 2, "binomial"), 3, False, dict(parallel=False))
CASES["pois2_dense_sequential"] = (lambda: pois(40, 2, 2), 3, False, dict(parallel=False))
CASES["plin2_dense_sequential"] = (lambda: plin(40, 2, 3, 2, 0.05), 3, False, dict(parallel=False))


def digest(make, Cn, chain_minor, opt, dtype):
    (model, delta), h = make(), _lib.Handle()
    try:
        h.set_option(_lib.OPT_SHARE_MODEL, opt.get("share", 1))
        h.set_option(_lib.OPT_OVERLAP_MODEL_STAGE, opt.get("overlap", 0))
        if "nan_policy" in opt:  # (get_kernel is the reference's signature: the policy is the device kernel's own argument)
            from aux_ssm_samplers_amd.kalman.generic import _get_device_kernel
            _, kernel = _get_device_kernel(model, opt.get("parallel", True), nan_policy=opt["nan_policy"])
        else:
            _, kernel = get_kernel(model.dynamics_factory, model.observations_factory, model.log_likelihood_fn, opt.get("parallel", True))
        x0 = start_state(model, Cn, dtype)
        ch = DeviceChains(h, x0, chain_minor=chain_minor, fused=opt.get("fused", False))
        stats = tuple(h.zeros(ch._x.shape, dtype) for _ in range(3)) if opt.get("moments") else ()
        if stats:
            h.stats_attach(stats, 0, ch._x)
        for i in range(opt.get("sweeps", 2)):  # (5: a slab of the model stage's ring of three comes round again, so the memoised stage runs)
            kernel(R.PRNGKey(100 + i), KalmanSampler(x=ch, updated=None), delta)
        if "fused" in opt and ch.fused is not True:
            raise RuntimeError("the fused sweep was refused")
        sha = hashlib.sha256()
        for a in (ch.to_host(), ch.accepted.to_host(), ch.logs.to_host()) + tuple(s.to_host() for s in stats):
            sha.update(np.ascontiguousarray(a).tobytes())
        return sha.hexdigest()
    finally:
        h.sync()
        h.close()


def start_state(model, Cn, dtype):
    return (0.3 * np.random.default_rng(1).standard_normal((Cn, model.T, model.dx))).astype(dtype)


# ---- host mode ----
HOST_MODELS = {
    "LGConcatModel": lambda: lg_missing(False)[0],
    "LorenzModel": lambda: lorenz(12)[0],
    "MVTModel:order1": lambda: mvt(12, 3, 1)[0], "MVTModel:order2": lambda: mvt(12, 3, 2)[0],
    "PoissonLinearModel:order1": lambda: plin(12, 2, 3, 1, 0.05)[0], "PoissonLinearModel:order2": lambda: plin(12, 2, 3, 2, 0.05)[0],
    "BinomialModel:order1": lambda: logit(12, 2, 1, "binomial")[0], "BinomialModel:order2": lambda: logit(12, 2, 2, "binomial")[0],
    "NegBinomialModel:order1": lambda: logit(12, 2, 1, "negbinomial")[0], "NegBinomialModel:order2": lambda: logit(12, 2, 2, "negbinomial")[0],
    "PoissonModel:order1": lambda: pois(12, 2, 1)[0], "PoissonModel:order2": lambda: pois(12, 2, 2)[0],
    "SVModel:order1": lambda: SVModel(holes(sv(12, 2, 1)[0].yobs), *sv_setup(12, 2)[2], order=1),
    "SVModel:order2": lambda: SVModel(holes(sv(12, 2, 2)[0].yobs), *sv_setup(12, 2)[2], order=2),
}


def host_digest(model, dtype):
    rng = np.random.default_rng(2)
    x = start_state(model, 1, dtype)[0]
    u = (x + 0.1 * rng.standard_normal(x.shape)).astype(dtype)
    if getattr(model, "batched_state", False):
        x, u = x[..., None], u[..., None]
    sha = hashlib.sha256()
    with np.errstate(all="ignore"):
        parts = tuple(model.dynamics_factory(x)) + tuple(model.observations_factory(x, u, 0.05)) + (model.log_likelihood_fn(x),)
    for a in parts:
        a = np.ascontiguousarray(a)
        sha.update(f"{a.dtype.str}{a.shape}".encode())
        sha.update(a.tobytes())
    return sha.hexdigest()


def densities_on_the_host():
    """the two densities the models' log_likelihood_fn take from the device primitives (they import them when called), as the NumPy oracle computes them"""
    from aux_ssm_samplers_amd._primitives.kalman import base
    from oracle import kalman_np as K
    base.prior_logpdf = lambda xs, lgssm, handle=None: K.prior_logpdf(np.asarray(xs), tuple(lgssm))
    base.joint_logpdf = lambda ys, xs, lgssm, *a, **k: K.log_likelihood(np.asarray(ys), np.asarray(xs), tuple(lgssm)) + K.prior_logpdf(np.asarray(xs), tuple(lgssm))


if __name__ == "__main__":
    host = sys.argv[1] == "--host"
    path = sys.argv[2 if host else 1]
    if host:
        densities_on_the_host()
    out, raised = {}, []
    for name, case, dtype in ((f"{n}:{np.dtype(dt).name}", c, dt) for n, c in sorted((HOST_MODELS if host else CASES).items()) for dt in (np.float64, np.float32)):
        try:
            out[name] = host_digest(case(), dtype) if host else digest(*case, dtype)
        except Exception as e:  # noqa: BLE001 -- recorded, and the run fails: an error's text is no digest
            out[name] = f"{type(e).__name__}: {e}"
            raised.append(name)
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(f"{len(out)} cases -> {path}" + (f"; RAISED: {', '.join(raised)}" if raised else ""))
    sys.exit(1 if raised else 0)
