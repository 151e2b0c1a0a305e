#!/usr/bin/env python3
"""One SHA-256 per case over the bytes of (x, accepted, logs) after consecutive keyed sweeps of a fixed list of small problems: every branch a driver of
the auxiliary Kalman sweep can take (csrc/api.hip: sweep_lg_concat, sweep_lg_concat_fused, sweep_sv, sweep_lorenz), in both dtypes.  For comparing two builds
of the library bit for bit:   AUXSSM_LIB=/path/to/libauxssm.so python tools/sweep_digest.py out.json   once per build, then compare the files.
A case that raises is recorded with the error's text."""
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aux_ssm_samplers_amd import _lib, random as R  # noqa: E402
from aux_ssm_samplers_amd.kalman import DeviceChains, KalmanSampler, LGConcatModel, LorenzModel, SVModel, get_kernel  # noqa: E402
from aux_ssm_samplers_amd.workloads import lg_model, lorenz_kalman_setup, sv_setup  # noqa: E402


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
        x0 = (0.3 * np.random.default_rng(1).standard_normal((Cn, model.T, model.dx))).astype(dtype)
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


if __name__ == "__main__":
    out = {}
    for name, (make, Cn, cm, opt) in sorted(CASES.items()):
        for dtype in (np.float64, np.float32):
            try:
                out[f"{name}:{np.dtype(dtype).name}"] = digest(make, Cn, cm, opt, dtype)
            except Exception as e:  # noqa: BLE001 -- part of the record: both builds must fail alike
                out[f"{name}:{np.dtype(dtype).name}"] = f"{type(e).__name__}: {e}"
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(f"{len(out)} cases -> {sys.argv[1]}")
