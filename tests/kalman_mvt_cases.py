"""The cells the tests of kalman.MVTModel share (tests/test_kalman_mvt_model.py, tests/test_gpu_kalman_mvt.py), and their oracle results.  Test infrastructure only.

A cell is (d, T, C, order, nu, prec kind, delta, NaN pattern, parallel).  Not the full product: two dozen cells in which every value of every axis occurs, chosen for
where the kernels can go wrong -- d = 1 (one lane), 4 / 9 / 25 (ragged waves: a wave holds several chains' components), 33 (across the half-wave), 64 (a full wave);
T = 2 and 3 (the pathwise sampler's first and only interior step) and 70 (a time loop longer than a wave); C * d from 1 lane to 4480 (seventy workgroups of the scalar
passes, never a multiple of 64 with C = 3 or 70 unless d = 64); missing data at t = 0, mid-way and T - 1, as a whole row and as a single component.

The acceptance uniforms are not drawn: they are placed at log u = log alpha -+ 0.5 (0.05 where log alpha + 0.5 would pass 0) around the ORACLE's log alpha (oracle.kalman_np.kalman_sweep driven by the model's
own factories), alternating along the chains, so that every chain's margin |log alpha - log u| is at least 0.05 >= 1e-2 and every cell has accepted and rejected chains.  A cell of
one chain is swept twice on the same noise, once with each uniform.  (The second-order factory leaves the gradient's NaN in place, so a missing row costs the move
d Var / delta in log alpha: those cells keep one missing row, a small d and delta = 0.5; and delta = 0.5 goes with the smaller T * d throughout, so that every
log alpha stays above -80 and its uniforms are representable in fp32.)"""
import functools
import math

import numpy as np

from oracle import kalman_np as K

#        d   T   C  order nu  prec     delta  nan          parallel
CELLS = [
    (1, 2, 1, 1, 1.0, "grid", 0.5, None, False),
    (1, 70, 3, 2, 3.0, "grid", 0.05, None, True),
    (4, 3, 1, 2, 1.0, "grid", 0.5, None, True),
    (4, 70, 3, 1, 3.0, "grid", 0.05, "t0_comp", False),
    (9, 2, 3, 1, 1.0, "grid", 0.05, None, True),
    (9, 70, 70, 2, 3.0, "grid", 0.5, None, False),
    (25, 3, 3, 1, 3.0, "grid", 0.5, "mid_row", True),
    (25, 70, 1, 2, 1.0, "grid", 0.05, None, False),
    (33, 3, 70, 1, 1.0, "dense", 0.5, None, True),
    (33, 70, 3, 2, 3.0, "dense", 0.05, None, False),
    (33, 2, 1, 1, 3.0, "dense", 0.05, "last_comp", True),
    (64, 3, 70, 2, 1.0, "grid", 0.5, None, True),
    (64, 70, 3, 1, 1.0, "grid", 0.05, "all", False),
    (64, 70, 1, 1, 3.0, "grid", 0.5, None, True),
    (64, 2, 3, 2, 3.0, "dense", 0.05, None, False),
    (9, 70, 3, 2, 1.0, "grid", 0.5, "mid_comp", True),
    (4, 3, 3, 2, 3.0, "grid", 0.5, "t0_row", False),
    (4, 70, 3, 2, 3.0, "dense", 0.5, "last_row", True),
    (1, 3, 70, 1, 3.0, "grid", 0.5, "mid_comp", False),
    (33, 70, 1, 1, 1.0, "dense", 0.05, "t0_row", False),
    (64, 70, 3, 2, 3.0, "grid", 0.05, None, True),
    (9, 3, 1, 1, 3.0, "dense", 0.5, None, False),
    (4, 70, 70, 1, 1.0, "grid", 0.5, None, True),
    (25, 2, 3, 1, 1.0, "grid", 0.05, None, False),
]
MARGIN, MARGIN_MIN = 0.5, 0.05   # |log alpha - log u_accept| of every chain is one of these, by construction
LOG_ALPHA_MIN = -80.0             # every chain's log alpha stays above it: exp(log alpha -+ margin) is then a normal number in fp32 too
IDS = [f"d{c[0]}-T{c[1]}-C{c[2]}-o{c[3]}-nu{c[4]:g}-{c[5]}-delta{c[6]:g}-{c[7] or 'full'}-{'par' if c[8] else 'seq'}" for c in CELLS]


def precision(kind, d, rng):
    from aux_ssm_samplers_amd.workloads import spatial_precision
    if kind == "grid":
        return spatial_precision(math.isqrt(d))
    A = rng.standard_normal((d, d))
    P = 1.5 * np.eye(d) + 0.8 * (A @ A.T) / d
    return 0.5 * (P + P.T)


def punch(y, nan):
    """the missing-data pattern `nan` into y (T, d)"""
    T, d = y.shape
    mid = T // 2
    for what in (("t0_row", "mid_comp", "last_row") if nan == "all" else (nan,) if nan else ()):
        t = {"t0": 0, "mid": mid, "last": T - 1}[what.split("_")[0]]
        if what.endswith("row"):
            y[t] = np.nan
        else:
            y[t, (d - 1) // 2] = np.nan
    return y


def build(i):
    """cell i -> dict(cell fields, model, x (C, T, d), eps_aux, eps_samp (C, T, d)): seeded by i and by the first attempt whose oracle log alpha leaves room for a
    rejection at the margin (a cell of one or three chains in which every move is all but certain would have no rejected chain)"""
    return reference(i)["cell"]


@functools.lru_cache(maxsize=None)
def _build(i, attempt):
    from aux_ssm_samplers_amd.kalman import MVTModel
    d, T, C, order, nu, kind, delta, nan, parallel = CELLS[i]
    rng = np.random.default_rng(1000 + i + 100 * attempt)
    prec = precision(kind, d, rng)
    sigma = 0.7
    truth = np.cumsum(sigma * rng.standard_normal((T, d)), axis=0)
    Lc = np.linalg.cholesky(np.linalg.inv(prec))
    y = punch(truth + (rng.standard_normal((T, d)) @ Lc.T) / np.sqrt(rng.chisquare(nu, T) / nu)[:, None], nan)
    m0, b = 0.1 * rng.standard_normal(d), 0.05 * rng.standard_normal((d, 1))
    P0, F, Q = 0.5 + rng.random((d, 1, 1)), 0.9 + 0.1 * rng.random(d), sigma ** 2 * (0.5 + rng.random((d, 1, 1)))
    model = MVTModel(y, m0, P0, F, Q, b, nu, prec, order=order)
    x = truth[None] + 0.3 * rng.standard_normal((C, T, d))
    return dict(d=d, T=T, C=C, order=order, nu=nu, delta=delta, nan=nan, parallel=parallel, model=model, x=x,
                eps_aux=rng.standard_normal((C, T, d)), eps_samp=rng.standard_normal((C, T, d)))


def oracle_sweep(model, x, delta, parallel, eps_aux, eps_samp, u_accept):
    """oracle.kalman_np.kalman_sweep on the model's own factories, one chain (T, d), in the reference's shapes"""
    e = lambda a: np.asarray(a)[..., None]
    return K.kalman_sweep(e(x), delta, model.dynamics_factory, model.observations_factory, model.log_likelihood_fn, parallel, e(eps_aux), e(eps_samp), u_accept)


@functools.lru_cache(maxsize=None)
def reference(i):
    """the oracle on cell i, computed once: dict(x_prop (C, T, d), logs (C, 5) = log alpha, lp_prop, lp_rev, lt_prop, lt_rev, us = the acceptance uniforms -- a list of
    (C,) arrays, one sweep of the cell each --, accepted = the oracle's flags under each)"""
    for attempt in range(20):
        c = _build(i, attempt)
        ref = _reference(c)
        flags = np.concatenate(ref["accepted"])
        if flags.any() and not flags.all() and np.all(ref["logs"][:, 0] > LOG_ALPHA_MIN):
            return dict(ref, cell=c)
    raise AssertionError(f"cell {IDS[i]}: no attempt with an accepted and a rejected chain")


def _reference(c):
    out = [oracle_sweep(c["model"], c["x"][k], c["delta"], c["parallel"], c["eps_aux"][k], c["eps_samp"][k], 0.5) for k in range(c["C"])]
    logs = np.array([[o["log_alpha"], o["lp_prop"], o["lp_rev"], o["lt_prop"], o["lt_rev"]] for o in out])
    la = logs[:, 0]

    # a rejecting uniform sits at log alpha + MARGIN where that is below 1, else at log alpha + MARGIN_MIN; a chain with log alpha > -MARGIN_MIN cannot be rejected
    # at a margin and accepts.  An accepting uniform sits at min(log alpha, 0) - MARGIN.
    gap = np.where(la + MARGIN < 0, MARGIN, MARGIN_MIN)
    can = la + gap < 0

    def place(reject):
        return np.where(reject & can, np.exp(np.where(can, la + gap, -1.0)), np.exp(np.minimum(la, 0.0) - MARGIN))

    C = c["C"]
    if C > 1:   # every other chain that can be rejected is
        turn = np.cumsum(can) % 2 == 1
        us = [place(turn)]
    else:
        us = [place(np.array([False])), place(np.array([True]))]
    alpha = np.exp(np.minimum(la, 0.0))
    return dict(x_prop=np.stack([o["x_prop"][..., 0] for o in out]), logs=logs, us=us, accepted=[u < alpha for u in us])
