"""The cells the tests of kalman.BinomialModel and kalman.NegBinomialModel share (tests/test_kalman_logistic_model.py, tests/test_gpu_kalman_logistic.py) and
their oracle results, computed once per process.  Test infrastructure only; modelled on tests/kalman_poisson_cases.py (same shapes, same margin rule).

A cell is a logit-link model at (d, T): log-odds with poisson_setup's banded F (0.9 on the diagonal, 0.05 / -0.05 beside it), P0 = 0.2 I, a slightly
non-diagonal Q and a stationary mean of 0 but for the last component (X_BIG).  Where T > 3 every cell holds a missing entry (NaN) at t = 0 (one component), a whole missing middle row and one at T - 1, and

    binomial      trials mixed 1 .. 40 with component 0 binary (trials = 1; at d = 1 the special entries below sit in that component and keep their own trials);
                  one y = 0; one y = trials; one trials = 1500 (y = 10, the start path at log-odds -5 there); the start state of every third chain (chain 0 of
                  a one-chain cell) reaches x = +30 at one point (y = trials there: sigma saturates at 1)
    negbinomial   r = 3, component 0 r = 0.5; one y = 0; one count of 1200 (m = y + r >= 1000, the start path at log(1200 / 3) there); every third chain's start
                  state reaches x = -30 at one point (y = 0 there: sigma saturates at 0).  "y = trials" has no counterpart: m = y + r > y always.

The saturated point sits in every third chain only: the first-order log alpha of a chain that starts from it is positive at every usable step size (the move
away from it is always accepted), so a cell whose chains all held it could hold no rejected chain.

The size of a missing entry is NaN too for the negative binomial (m = y + r), and set to NaN for the binomial's missing middle row: the device must not look at it.
The two- and three-step cells hold the zero and the large size only.

Step sizes by shape (delta_for): chosen on the CPU so that every multi-chain cell's oracle holds an accepted and a rejected chain under the margin rule below, at
the first few seeds (the Poisson cells' 0.05 / 0.02 / 0.3 leave the second-order log alpha within +-0.3, where few chains can be rejected at a margin).

The acceptance uniforms are not drawn: they are placed at log u = log alpha -+ 0.5 (0.05 where log alpha + 0.5 would pass 0) around the ORACLE's log alpha,
alternating along the chains, so every chain's margin is at least 0.05 and an accept flag that differs is a defect.  A chain with log alpha >= -0.05 can only
accept.  A multi-chain cell must hold both outcomes: its seed is the first attempt for which the oracle says so."""
import functools

import numpy as np

from oracle import kalman_np as K

MARGIN, MARGIN_MIN = 0.5, 0.05
LOG_ALPHA_MIN = -80.0   # exp(log alpha -+ margin) must be a normal number in fp32 too

FAMILIES = ("binomial", "negbinomial")
DENSE_SHAPES = [(1, 2), (4, 3), (1, 400), (2, 257), (3, 70), (4, 150), (6, 60), (30, 24)]
CM_SHAPES = [(1, 300, 40), (2, 129, 33), (4, 70, 64)]
WIDE_SHAPES = [(6, 40, 3), (30, 24, 3)]
X_SAT = 30.0
# the stationary mean of the last component's log-odds, where the large size sits: binomial 1500 sigma(-3) = 71 successes expected and lam = 68 (at log-odds 0 lam =
# 375 and a first-order step needs delta << 1 / 375); negative binomial r e^x = 1200 at r = 3, so that component's counts are all near 1200 and lam is near r
X_BIG = {"binomial": -3.0, "negbinomial": float(np.log(400.0))}


def delta_for(d, T):
    return 0.3 if T <= 3 else (0.005 if d >= 30 else 0.01)


def oracle_target(model):
    """log_likelihood_fn on the oracle's own prior density (the model's goes through the package's primitives)"""
    def f(z):
        lg = (model.m0, model.P0, model.Fs, model.Qs, model.bs, None, None, None)
        return K.prior_logpdf(z, lg) + model.log_potential(z)
    return f


def make_data(family, d, T, seed):
    """(y, size parameter (trials or r) (T, d), path, sat = (t, k, offset) of the saturated point of every third chain's start state or None, (m0, P0, F, Q, b))"""
    rng = np.random.Generator(np.random.PCG64(seed))
    F = 0.9 * np.eye(d) + 0.05 * np.eye(d, k=1) - 0.05 * np.eye(d, k=-1)
    kb = d - 1
    m0 = np.zeros(d)
    m0[kb] = X_BIG[family]
    b = m0 - F @ m0
    Q, P0 = 0.04 * np.eye(d), 0.2 * np.eye(d)
    x = np.zeros((T, d))
    x[0] = m0 + np.sqrt(0.2) * rng.standard_normal(d)
    for t in range(1, T):
        x[t] = F @ x[t - 1] + b + 0.2 * rng.standard_normal(d)
    if d > 1:
        Q = Q + 0.004 * (np.eye(d, k=1) + np.eye(d, k=-1))
    long_ = T > 3
    tz, tb = (2, T // 3) if long_ else (0, 1)   # where the zero and the large size go
    tf, ts = 3, (2 * T) // 3                     # y = trials; the saturated point (long cells only)
    p = 1.0 / (1.0 + np.exp(-x))
    if family == "binomial":
        par = rng.integers(1, 41, size=(T, d)).astype(np.float64)
        par[:, 0] = 1.0
        par[tb, kb] = 1500.0
        y = rng.binomial(par.astype(np.int64), p).astype(np.float64)
        y[tz, 0] = 0.0
        if long_:
            par[tf, kb] = 7.0
            y[tf, kb] = 7.0
            par[ts, kb] = 5.0
            y[ts, kb] = 5.0
    else:
        par = np.full((T, d), 3.0)
        par[:, 0] = 0.5
        y = rng.poisson(rng.gamma(par, np.exp(x))).astype(np.float64)
        y[tb, kb] = 1200.0
        y[tz, 0] = 0.0
        if long_:
            y[ts, kb] = 0.0
    if long_:
        y[0, (d - 1) // 2] = np.nan
        y[T // 2] = np.nan
        y[T - 1, kb] = np.nan
        if family == "binomial":
            par[T // 2] = np.nan
    sat = (ts, kb, X_SAT if family == "binomial" else -X_SAT) if long_ else None
    return y, par, x, sat, (m0, P0, F, Q, b)


def make_model(family, y, par, m0, P0, F, Q, b, order):
    from aux_ssm_samplers_amd.kalman import BinomialModel, NegBinomialModel
    return (BinomialModel if family == "binomial" else NegBinomialModel)(y, par, m0, P0, F, Q, b, order=order)


@functools.lru_cache(maxsize=None)
def _build(family, d, T, C, order, attempt, f32=False):
    """f32: every input (model, state, noise) rounded to float32 and held as float64 -- what a float32 sweep is given, for the float64 oracle"""
    r = (lambda a: np.asarray(a, np.float32).astype(np.float64)) if f32 else (lambda a: a)
    seed = 100 * attempt + 7 * d + T
    y, par, path, sat, (m0, P0, F, Q, b) = make_data(family, d, T, seed)
    model = make_model(family, y, r(par), r(m0), r(P0), r(F), r(Q), r(b), order)
    rng = np.random.default_rng(5000 + seed)
    x = path[None] + 0.1 * rng.standard_normal((C, T, d))
    if sat is not None:
        x[::3, sat[0], sat[1]] += sat[2]
    x = r(x)
    return dict(family=family, d=d, T=T, C=C, order=order, delta=delta_for(d, T), model=model, x=x, eps_aux=r(rng.standard_normal((C, T, d))),
                eps_samp=r(rng.standard_normal((C, T, d))))


def place_uniforms(la):
    """-> (us, accepted): lists of (C,) arrays, one sweep of the cell each.  Several chains: every other chain that can be rejected at a margin is; one chain:
    two sweeps, one with each uniform."""
    la = np.asarray(la, np.float64)
    gap = np.where(la + MARGIN < 0, MARGIN, MARGIN_MIN)
    can = la + gap < 0

    def place(reject):
        return np.where(reject & can, np.exp(np.where(can, la + gap, -1.0)), np.exp(np.minimum(la, 0.0) - MARGIN))

    us = [place(np.cumsum(can) % 2 == 1)] if la.size > 1 else [place(np.array([False])), place(np.array([True]))]
    alpha = np.exp(np.minimum(la, 0.0))
    return us, [u < alpha for u in us]


def oracle_chain(cell, c, parallel, u_accept=0.5):
    return K.kalman_sweep(cell["x"][c], cell["delta"], cell["model"].dynamics_factory, cell["model"].observations_factory, oracle_target(cell["model"]), parallel,
                          cell["eps_aux"][c], cell["eps_samp"][c], u_accept)


@functools.lru_cache(maxsize=None)
def reference(family, d, T, C, order, parallel=True, every=1, f32=False):
    """dict(cell, chains = the chain indices the oracle ran (every `every`-th), x_prop (n, T, d), logs (n, 5) = log alpha, lp_prop, lp_rev, lt_prop, lt_rev,
    us / accepted over ALL C chains when every == 1, else over the oracle's chains only (the others get u = 0.5))"""
    for attempt in range(20):
        cell = _build(family, d, T, C, order, attempt, f32)
        idx = np.arange(0, C, every)
        out = [oracle_chain(cell, c, parallel) for c in idx]
        logs = np.array([[o["log_alpha"], o["lp_prop"], o["lp_rev"], o["lt_prop"], o["lt_rev"]] for o in out])
        us_i, acc_i = place_uniforms(logs[:, 0])
        flags = np.concatenate(acc_i)
        if np.all(np.isfinite(logs)) and np.all(logs[:, 0] > LOG_ALPHA_MIN) and (C == 1 or (flags.any() and not flags.all())):
            us = []
            for u in us_i:
                full = np.full(C, 0.5)
                full[idx] = u
                us.append(full)
            return dict(cell=cell, chains=idx, attempt=attempt, x_prop=np.stack([o["x_prop"] for o in out]), logs=logs, us=us, accepted=acc_i)
    raise AssertionError(f"cell {family} d={d} T={T} C={C} order={order}: no attempt with an accepted and a rejected chain")
