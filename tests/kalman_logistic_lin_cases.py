"""The cells the tests of kalman.BinomialLinearModel and kalman.NegBinomialLinearModel share (tests/test_kalman_logistic_lin_model.py,
tests/test_hostsim_plin_logistic.py, tests/test_gpu_kalman_logistic_lin.py) and their oracle results, computed once per process.  Test infrastructure only; built
as tests/kalman_poisson_lin_cases.py is (same shapes, same margin rule, same placed uniforms).

A cell is workloads.logistic_lin_setup's latent path, loading matrix and offsets at (dx, dy, T) with a slightly non-diagonal Q (+ 0.004 beside the diagonal for
dx > 1), the sizes and the data drawn here so that every cell with dy >= 3 holds, whatever its seed:

    binomial      trials per channel mixed 1 .. 40, channel 0 binary (trials = 1), the last channel trials = 1500 at an offset of -3 (about 70 successes, so
                  that its curvature is 68 and not 375); one y = 0 (in the binary channel); one y = trials; a missing channel at t = 0, a wholly missing row
                  T // 2 and (T > 3) a missing channel at T - 1; at one step SAT_T the channel of the largest loading has y = trials and the start state of
                  every third chain (chain 0 of a one-chain cell) is moved along that loading until eta = +30 there: sigma saturates at 1
    negbinomial   r = 3 per channel, channel 0 r = 0.5, the last channel at an offset of log 400 with one count of 1200 (m = y + r >= 1000); one y = 0; the same
                  missing entries; at SAT_T the channel of the largest loading has y = 0 and every third chain starts at eta = -30 there: sigma saturates at 0.
                  "trials = 1" and "y = trials" have no counterpart: m = y + r > y always.

The sizes are per channel, so the one-channel cell (1, 1, 2) cannot hold trials = 1 beside trials >= 1000, nor a missing entry beside y = 0 and y = trials in
its two steps: it holds the large size (binomial trials = 1500, negative binomial a count of 1200), y = 0 / the large count at t = 0 and the saturated start at
t = 1, and nothing missing.

The step size is delta = min(0.3, 4 / lambda_max(H' diag(m) H)), the largest eigenvalue over t (the model's first_order_delta(): Lam_t <= H' diag(m_t / 4) H at
every x, so delta lambda_max(Lam_t) <= 1 wherever the chain is).  The chains start at path + min(0.1, sqrt(delta)) N(0, 1).

The acceptance uniforms are not drawn: tests/kalman_poisson_cases.py::place_uniforms puts them at log u = log alpha -+ 0.5 (0.05 where log alpha + 0.5 would
pass 0) around the ORACLE's log alpha, so every chain's margin is at least 0.05 and an accept flag that differs is a defect.  A multi-chain cell must hold both
outcomes: its seed is the first attempt (of 20) for which the oracle says so."""
import functools

import numpy as np

from oracle import kalman_np as K
from tests.kalman_poisson_cases import LOG_ALPHA_MIN, oracle_target, place_uniforms  # noqa: F401  (one placement rule for all the count models)

FAMILIES = ("binomial", "negbinomial")
ONE_CHAIN_SHAPES = [(1, 1, 2), (1, 3, 3), (2, 7, 257), (3, 5, 70), (4, 65, 150), (3, 130, 40), (1, 257, 24)]
CHAIN_SHAPES = [(2, 7, 129, 33, 7), (4, 65, 70, 5, 1), (1, 3, 300, 40, 7)]   # (dx, dy, T, C, every)
ETA_SAT = 30.0
LOG_ALPHA_MAX = 80.0   # a chain that starts at the saturated point has a positive log alpha (the move away from it is always accepted); moderate all the same
BIG = {"binomial": (1500.0, -3.0), "negbinomial": (1200.0, float(np.log(400.0)))}   # the large size (trials | count) and its channel's offset


def sat_step(T):
    return 1 if T == 2 else (2 * T) // 3


def make_model(family, dx, dy, T, seed, order, r=lambda a: a):
    """(model, path, sat): logistic_lin_setup's recipe with the cell's sizes and data; r rounds the model's arrays; sat = (t, channel, target eta)"""
    from aux_ssm_samplers_amd.kalman import BinomialLinearModel, NegBinomialLinearModel
    from aux_ssm_samplers_amd.workloads import logistic_lin_setup
    base, path, H, c, _ = logistic_lin_setup(T, dx, dy, family, seed)
    rng = np.random.Generator(np.random.PCG64(900 + seed))
    Q = np.array(base.Q)
    if dx > 1:
        Q = Q + 0.004 * (np.eye(dx, k=1) + np.eye(dx, k=-1))
    kb = dy - 1
    c = np.array(c)
    c[kb] = BIG[family][1]
    eta = path @ H.T + c
    if family == "binomial":
        par = rng.integers(2, 41, size=dy).astype(np.float64)
        par[0] = 1.0
        par[kb] = BIG[family][0]
        y = rng.binomial(np.broadcast_to(par, eta.shape).astype(np.int64), 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
    else:
        par = np.full(dy, 3.0)
        par[0] = 0.5
        y = rng.poisson(rng.gamma(np.broadcast_to(par, eta.shape), np.exp(eta))).astype(np.float64)
    ts, ks = sat_step(T), int(np.argmax(np.linalg.norm(H, axis=1)))
    if dy == 1:
        y[0, 0] = 0.0 if family == "binomial" else BIG[family][0]
    else:
        tz = 0 if T <= 3 else 2
        y[tz, 0] = 0.0
        if family == "binomial":
            y[T - 1 if T <= 3 else 3, 1] = par[1]     # y = trials
        else:
            y[0 if T <= 3 else T // 3, kb] = BIG[family][0]
        y[0, (dy - 1) // 2] = np.nan
        y[T // 2] = np.nan
        if T > 3:
            y[T - 1, kb] = np.nan
    y[ts, ks] = par[ks] if family == "binomial" else 0.0
    cls = BinomialLinearModel if family == "binomial" else NegBinomialLinearModel
    sat = (ts, ks, ETA_SAT if family == "binomial" else -ETA_SAT)
    return cls(y, r(par), r(H), r(c), r(base.m0), r(base.P0), r(base.F), r(Q), r(base.b), order=order), path, sat


def seed_of(dx, dy, T, attempt):
    return 100 * attempt + 7 * dx + 3 * dy + T


@functools.lru_cache(maxsize=None)
def _build(family, dx, dy, T, C, order, attempt, f32=False):
    """f32: every input (model, state, noise) rounded to float32 and held as float64 -- what a float32 sweep is given, for the float64 oracle"""
    r = (lambda a: np.asarray(a, np.float32).astype(np.float64)) if f32 else (lambda a: a)
    seed = seed_of(dx, dy, T, attempt)
    model, path, (ts, ks, target) = make_model(family, dx, dy, T, seed, order, r)
    delta = min(0.3, model.first_order_delta())
    rng = np.random.default_rng(7000 + seed)
    x = path[None] + min(0.1, np.sqrt(delta)) * rng.standard_normal((C, T, dx))
    h = model.H[ks]
    x[::3, ts] += ((target - (x[::3, ts] @ h + model.c[ks])) / (h @ h))[:, None] * h    # every third chain: eta = -+30 in channel ks at step ts
    x = r(x)
    return dict(family=family, d=dx, dy=dy, T=T, C=C, order=order, delta=delta, model=model, x=x, sat=(ts, ks), eps_aux=r(rng.standard_normal((C, T, dx))),
                eps_samp=r(rng.standard_normal((C, T, dx))))


def oracle_chain(cell, c, parallel, u_accept=0.5):
    return K.kalman_sweep(cell["x"][c], cell["delta"], cell["model"].dynamics_factory, cell["model"].observations_factory, oracle_target(cell["model"]), parallel,
                          cell["eps_aux"][c], cell["eps_samp"][c], u_accept)


@functools.lru_cache(maxsize=None)
def reference(family, dx, dy, T, C, order, parallel=True, every=1, f32=False):
    """dict(cell, chains = the chain indices the oracle ran (every `every`-th), x_prop (n, T, dx), logs (n, 5) = log alpha, lp_prop, lp_rev, lt_prop, lt_rev,
    us / accepted: lists of (C,) / (n,) arrays, one sweep each (the chains the oracle did not run get u = 0.5), attempt)"""
    for attempt in range(20):
        cell = _build(family, dx, dy, T, C, order, attempt, f32)
        idx = np.arange(0, C, every)
        out = [oracle_chain(cell, c, parallel) for c in idx]
        logs = np.array([[o["log_alpha"], o["lp_prop"], o["lp_rev"], o["lt_prop"], o["lt_rev"]] for o in out])
        us_i, acc_i = place_uniforms(logs[:, 0])
        flags = np.concatenate(acc_i)
        if np.all(np.isfinite(logs)) and np.all(logs[:, 0] > LOG_ALPHA_MIN) and np.all(logs[:, 0] < LOG_ALPHA_MAX) and (C == 1 or (flags.any() and not flags.all())):
            us = []
            for u in us_i:
                full = np.full(C, 0.5)
                full[idx] = u
                us.append(full)
            return dict(cell=cell, chains=idx, x_prop=np.stack([o["x_prop"] for o in out]), logs=logs, us=us, accepted=acc_i, attempt=attempt)
    raise AssertionError(f"cell {family} dx={dx} dy={dy} T={T} C={C} order={order}: no attempt with an accepted and a rejected chain")


# ---- ground truth without a restatement: posterior moments by quadrature ---------------------------------------------------------------------------------
def _log_g(y, m, H, c, x):
    """sum_j y_j eta_j - m_j softplus(eta_j) over the observed channels, x (..., dx) -> (...)"""
    from aux_ssm_samplers_amd._logistic import log_g
    return log_g(x @ H.T + c, y, np.where(np.isfinite(y), m, 0.0))


def posterior_scalar_T3(y, m, H, c, m0, P0, F, Q, b, n, width=7.0):
    """dx = 1, T = 3: mean and variance of x_0, x_1, x_2 by a tensor-product grid over (x_0, x_1, x_2) centred on m0 (tests/test_gpu_kalman_poisson_lin.py's
    grid).  Independent of every sampler and of the oracle."""
    g = m0 + np.linspace(-width * np.sqrt(P0), width * np.sqrt(P0), n)
    x0, x1, x2 = np.meshgrid(g, g, g, indexing="ij", sparse=True)
    lp = -0.5 * (x0 - m0) ** 2 / P0 - 0.5 * (x1 - F * x0 - b) ** 2 / Q - 0.5 * (x2 - F * x1 - b) ** 2 / Q
    for xt, yt, mt in ((x0, y[0], m[0]), (x1, y[1], m[1]), (x2, y[2], m[2])):
        lp = lp + _log_g(yt, mt, H, c, xt[..., None])
    w = np.exp(lp - lp.max())
    w /= w.sum()
    out = []
    for ax in range(3):
        mg = w.sum(tuple(a for a in range(3) if a != ax))
        mean = float((mg * g).sum())
        out.append((mean, float((mg * (g - mean) ** 2).sum())))
    return np.array(out)


def posterior_planar_T2(y, m, H, c, m0, P0, F, Q, b, n, width=6.0):
    """dx = 2, T = 2: mean and variance of the four coordinates (x_0, x_1 in the plane) by a 4-D tensor grid, held as an (n^2, n^2) table over (x_0, x_1):
    pi ~ N(x_0; m0, P0) g_0(x_0) N(x_1; F x_0 + b, Q) g_1(x_1).  Independent of every sampler and of the oracle."""
    ax = [m0[k] + np.linspace(-width * np.sqrt(P0[k, k]), width * np.sqrt(P0[k, k]), n) for k in range(2)]
    pts = np.stack(np.meshgrid(ax[0], ax[1], indexing="ij"), axis=-1).reshape(-1, 2)   # (n^2, 2)
    iP0, iQ = np.linalg.inv(P0), np.linalg.inv(Q)
    r0 = pts - m0
    a0 = -0.5 * np.einsum("ik,kl,il->i", r0, iP0, r0) + _log_g(y[0], m[0], H, c, pts)
    a1 = _log_g(y[1], m[1], H, c, pts)
    mu = pts @ F.T + b
    # -(x1 - mu)' iQ (x1 - mu) / 2 = -x1' iQ x1 / 2 + x1' iQ mu - mu' iQ mu / 2
    lp = (a0 - 0.5 * np.einsum("ik,kl,il->i", mu, iQ, mu))[:, None] + (a1 - 0.5 * np.einsum("ik,kl,il->i", pts, iQ, pts))[None, :] + (mu @ iQ) @ pts.T
    w = np.exp(lp - lp.max())
    w /= w.sum()
    out = []
    for mg in (w.sum(1), w.sum(0)):
        for k in range(2):
            mean = float((mg * pts[:, k]).sum())
            out.append((mean, float((mg * (pts[:, k] - mean) ** 2).sum())))
    return np.array(out)


NAN = float("nan")
QUAD = {
    # one latent, three binary channels (trials = 1), T = 3, the entry of channel 1 at t = 1 missing
    "scalar": dict(family="binomial", par=1.0, y=np.array([[1.0, 0.0, 1.0], [0.0, NAN, 1.0], [1.0, 1.0, 0.0]]), H=np.array([[1.0], [-0.6], [0.4]]),
                   c=np.array([0.5, 0.2, -0.5]), m0=np.array([0.3]), P0=np.array([[0.2]]), F=np.array([[0.9]]), Q=np.array([[0.04]]), b=np.array([0.1]),
                   grid=(posterior_scalar_T3, 101, 201)),
    # two latents, three negative-binomial channels with r = 0.5, T = 2, dense H: Lam = H' diag(m s1) H and with it Omega are truly non-diagonal
    "planar": dict(family="negbinomial", par=0.5, y=np.array([[2.0, 5.0, 0.0], [4.0, 1.0, 3.0]]), H=np.array([[0.8, -0.5], [0.3, 0.9], [-0.7, 0.4]]),
                   c=np.array([0.6, 1.0, 0.2]), m0=np.array([0.2, -0.1]), P0=np.array([[0.3, 0.05], [0.05, 0.25]]), F=np.array([[0.9, 0.05], [-0.05, 0.9]]),
                   Q=np.array([[0.09, 0.01], [0.01, 0.08]]), b=np.array([0.05, 0.0]), grid=(posterior_planar_T2, 41, 61)),
}


def quad_model(name, order):
    from aux_ssm_samplers_amd.kalman import BinomialLinearModel, NegBinomialLinearModel
    q = QUAD[name]
    cls = BinomialLinearModel if q["family"] == "binomial" else NegBinomialLinearModel
    return cls(q["y"], q["par"], q["H"], q["c"], q["m0"], q["P0"], q["F"], q["Q"], q["b"], order=order)


@functools.lru_cache(maxsize=None)
def quad_exact(name):
    """(coarse, fine): the posterior (mean, variance) of every coordinate on the two grids; the tests use the fine one once the two agree to 1e-6 relative
    (tests/test_kalman_logistic_lin_model.py asserts that on the CPU)"""
    q = QUAD[name]
    fn, n_coarse, n_fine = q["grid"]
    m = quad_model(name, 1).size
    dyn = [q[k] if name == "planar" else float(np.squeeze(q[k])) for k in ("m0", "P0", "F", "Q", "b")]
    return fn(q["y"], m, q["H"], q["c"], *dyn, n=n_coarse), fn(q["y"], m, q["H"], q["c"], *dyn, n=n_fine)
