"""The cells the tests of kalman.PoissonLinearModel share (tests/test_kalman_poisson_lin_model.py, tests/test_hostsim_plin.py,
tests/test_gpu_kalman_poisson_lin.py) and their oracle results, computed once per process.  Test infrastructure only; built as tests/kalman_poisson_cases.py is.

A cell is workloads.poisson_lin_setup's model at (dx, dy, T) with a slightly non-diagonal Q (+ 0.004 beside the diagonal for dx > 1), one count of 0, and for
T > 3 counts missing (NaN) at t = 0 (one channel), in the whole row T // 2 and at T - 1 (one channel).  The step size is
delta = min(0.3 if T <= 3 else 0.05, 1 / lambda_max), lambda_max the largest eigenvalue of Lam_t = H' diag(e_t) H over the simulated path: the first-order
proposal is only usable for delta * lambda_max of order 1 (the model's docstring).  The chains start at path + min(0.1, sqrt(delta)) N(0, 1).

The acceptance uniforms are not drawn: they are placed at log u = log alpha -+ 0.5 (0.05 where log alpha + 0.5 would pass 0) around the ORACLE's log alpha by
tests/kalman_poisson_cases.py::place_uniforms, so every chain's margin is at least 0.05 and an accept flag that differs is a defect.  A multi-chain cell must hold
both outcomes: its seed is the first attempt (of 20) for which the oracle says so.  At dy = 257 the second-order log alpha is within 0.05 of 0, so no chain there
can be rejected at a margin: those shapes are one-chain cells, with one uniform on each side.

The shapes, each for something that can go wrong (the kernel's column block is 64 channels, its time tile 256 steps, a workgroup takes 4 chains):
  (1, 1, 2) the sampler's first step; (1, 3, 3) the only interior step; (2, 7, 257) crosses the 256-step tile; (3, 5, 70) dx = 3; (4, 65, 150) dy one past a
  64-column block; (3, 130, 40) a ragged third block; (1, 257, 24) dy far beyond dx.
  Several chains: (2, 7, 129, 33) and (1, 3, 300, 40) every 7th chain against its oracle (a ragged last group of chains; two time tiles), (4, 65, 70, 5) all five."""
import functools

import numpy as np

from oracle import kalman_np as K
from tests.kalman_poisson_cases import LOG_ALPHA_MIN, oracle_target, place_uniforms  # noqa: F401  (one placement rule for both models)

ONE_CHAIN_SHAPES = [(1, 1, 2), (1, 3, 3), (2, 7, 257), (3, 5, 70), (4, 65, 150), (3, 130, 40), (1, 257, 24)]
CHAIN_SHAPES = [(2, 7, 129, 33, 7), (4, 65, 70, 5, 1), (1, 3, 300, 40, 7)]   # (dx, dy, T, C, every)


def lambda_max(model, path):
    return float(np.max(np.linalg.eigvalsh(model.grad_lam(path)[1])))


def make_model(dx, dy, T, seed, order, r=lambda a: a):
    """(model, path): poisson_lin_setup's recipe with the cell's changes; r rounds the model's arrays"""
    from aux_ssm_samplers_amd.kalman import PoissonLinearModel
    from aux_ssm_samplers_amd.workloads import poisson_lin_setup
    base, path, H, c = poisson_lin_setup(T, dx, dy, seed)
    Q = np.array(base.Q)
    if dx > 1:
        Q = Q + 0.004 * (np.eye(dx, k=1) + np.eye(dx, k=-1))
    y = np.array(base.yobs, np.float64)
    y[1 if T <= 3 else 2, 0] = 0.0
    if T > 3:
        y[0, (dy - 1) // 2] = np.nan
        y[T // 2] = np.nan
        y[T - 1, dy - 1] = np.nan
    return PoissonLinearModel(y, r(H), r(c), r(base.m0), r(base.P0), r(base.F), r(Q), r(base.b), order=order), path


@functools.lru_cache(maxsize=None)
def _build(dx, dy, T, C, order, attempt, f32=False):
    """f32: every input (model, state, noise) rounded to float32 and held as float64 -- what a float32 sweep is given, for the float64 oracle"""
    r = (lambda a: np.asarray(a, np.float32).astype(np.float64)) if f32 else (lambda a: a)
    seed = 100 * attempt + 7 * dx + 3 * dy + T
    model, path = make_model(dx, dy, T, seed, order, r)
    delta = min(0.3 if T <= 3 else 0.05, 1.0 / lambda_max(model, path))
    rng = np.random.default_rng(7000 + seed)
    x = r(path[None] + min(0.1, np.sqrt(delta)) * rng.standard_normal((C, T, dx)))
    return dict(d=dx, dy=dy, T=T, C=C, order=order, delta=delta, model=model, x=x, eps_aux=r(rng.standard_normal((C, T, dx))),
                eps_samp=r(rng.standard_normal((C, T, dx))))


def oracle_chain(cell, c, parallel, u_accept=0.5):
    return K.kalman_sweep(cell["x"][c], cell["delta"], cell["model"].dynamics_factory, cell["model"].observations_factory, oracle_target(cell["model"]), parallel,
                          cell["eps_aux"][c], cell["eps_samp"][c], u_accept)


@functools.lru_cache(maxsize=None)
def reference(dx, dy, T, C, order, parallel=True, every=1, f32=False):
    """dict(cell, chains = the chain indices the oracle ran (every `every`-th), x_prop (n, T, dx), logs (n, 5) = log alpha, lp_prop, lp_rev, lt_prop, lt_rev,
    us / accepted: lists of (C,) / (n,) arrays, one sweep each (the chains the oracle did not run get u = 0.5), attempt)"""
    for attempt in range(20):
        cell = _build(dx, dy, T, C, order, attempt, f32)
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
            return dict(cell=cell, chains=idx, x_prop=np.stack([o["x_prop"] for o in out]), logs=logs, us=us, accepted=acc_i, attempt=attempt)
    raise AssertionError(f"cell dx={dx} dy={dy} T={T} C={C} order={order}: no attempt with an accepted and a rejected chain")
