"""Shared cases of the narrow Kalman filter's full (dx, dy) grid (tests/test_kalman_grid_host.py on the CPU, tests/test_gpu_kalman_grid.py on the device).
Imports no GPU code.

PAIRS is every size the per-lane filter is compiled for: dx 1..4 x dy 1..8, in fp32 and fp64 the 64 `KalmanEntry` rows of csrc/kernels.hip.h.

Models: the recipe of tests/test_gpu_wide.py::stable_model -- contracting time-varying F ~ 0.5 N / sqrt(dx), Q, R and P0 with eigenvalues bounded below (0.1, 0.1,
0.5), dense H, c != 0 -- with every input rounded to fp32 and cast back to fp64, so that the fp32 and the fp64 kernels, the fp32 oracle and the fp64 oracle all read
the same numbers.

Missing data is placed, not drawn.  The four kinds of row
    A  wholly missing                    B  only component 0 missing
    C  only component dy-1 missing (dy > 1)    D  exactly one component present (dy >= 3; which one rotates with the case)
(dy = 1 has A only; dy = 2 has A, B, C) go, rotated by the case so that over the grid every kind meets every place, to
    * both sides of the first chunk edge: `plan_scan` (csrc/api.hip) gives one sequence of n = T - 1 = 69 elements chunks of E = 4 elements (the E ~ sqrt(n / 450)
      floor of 4) on a chip of any size, and the 256 lane-sequences of T = 33 the same E = 4, so the first edge lies between elements 3 | 4 = time steps 4 | 5;
      for T = 600 the place is the tile scan's first tile edge, elements 255 | 256 = time steps 256 | 257;
    * the last step;
    * the fourth kind, for which these three places leave no room, the step before the edge (the last element but one of the first chunk / tile).
t = 0 is partly missing for odd dy (component dy // 2: kalman_bodies.h::body_filter_t0's masked update; at dy = 1 that is the whole row) and fully observed for even dy.
Every other row is fully observed.

fp32 yardstick (`fp32_reference_error`): the NumPy oracle run in fp32 arithmetic, sequential and parallel, against the fp64 sequential oracle on the same inputs;
per quantity max|fp32 - fp64| / max|fp64|, the larger of the two orders, the worst over the 32 pairs.  A kernel may be FP32_FACTOR = 4 times worse than that (the
factor tests/test_gpu_user_model_multidim.py gives a kernel over NumPy's own fp32 error: another operation order, fused multiply-adds), separately for means,
covariances and ell.  Nothing in the bar is read off the code under test.
"""
import functools

import numpy as np

from oracle import kalman_np as K

PAIRS = [(dx, dy) for dx in range(1, 5) for dy in range(1, 9)]
TOL64 = dict(rtol=1e-7, atol=1e-9)
FP32_FACTOR = 4.0
CHUNK = 4                       # plan_scan's chunk length for one sequence of T = 70 and for the 256 lane-sequences of T = 33
LANES = dict(T=33, B=64, C=4)   # B >= 32 and C * B >= 256: auxssm_kalman_filter maps lanes to (c, b) sequences


def edge_steps(T):
    """(left, right) time steps of the first chunk edge (T < 513) or of the tile scan's first tile edge: scan element i is time step i + 1"""
    return (256, 257) if T - 1 >= 512 else (CHUNK, CHUNK + 1)


def _kinds(dy):
    return "A" if dy == 1 else "ABC" if dy == 2 else "ABCD"


def _missing(kind, dy, keep):
    m = np.zeros(dy, bool)
    if kind == "A":
        m[:] = True
    elif kind == "B":
        m[0] = True
    elif kind == "C":
        m[dy - 1] = True
    else:
        m[:] = True
        m[keep % dy] = False
    return m


def place_missing(ys, rot):
    """NaNs into ys (T, dy) in place, as the module docstring says; `rot` rotates the kinds over the places.  Returns {time step: kind}."""
    T, dy = ys.shape
    left, right = edge_steps(T)
    kinds = _kinds(dy)
    places = [left, right, T - 1, left - 1][:max(3, len(kinds))]
    if dy == 1:                      # one kind, three places
        kinds = "AAA"
    where = {}
    for k, kind in enumerate(kinds):
        t = places[(k + rot) % len(places)]
        ys[t, _missing(kind, dy, rot)] = np.nan
        where[t] = kind
    if dy % 2:
        ys[0, dy // 2] = np.nan
        where[0] = "t0"
    return where


def _model(rng, T, d, p, lead=()):
    """stable_model's recipe with optional batch axes `lead` after the time axis"""
    r32 = lambda a: a.astype(np.float32).astype(np.float64)
    sw = lambda a: np.swapaxes(a, -1, -2)
    Fs = 0.5 * rng.standard_normal((T - 1,) + lead + (d, d)) / np.sqrt(d)
    A = rng.standard_normal((T - 1,) + lead + (d, 2 * d))
    Qs = A @ sw(A) / (2 * d) + 0.1 * np.eye(d)
    bs = rng.standard_normal((T - 1,) + lead + (d,))
    Hs = rng.standard_normal((T,) + lead + (p, d)) / np.sqrt(d)
    Bm = rng.standard_normal((T,) + lead + (p, 2 * p))
    Rs = Bm @ sw(Bm) / (2 * p) + 0.1 * np.eye(p)
    cs = rng.standard_normal((T,) + lead + (p,))
    m0 = rng.standard_normal(lead + (d,))
    A0 = rng.standard_normal(lead + (d, 2 * d))
    P0 = A0 @ sw(A0) / (2 * d) + 0.5 * np.eye(d)
    return tuple(r32(a) for a in (m0, P0, Fs, Qs, bs, Hs, Rs, cs))


class Case:
    def __init__(self, dx, dy, T, seed, ys, lg, where):
        self.dx, self.dy, self.T, self.seed, self.ys, self.lg, self.where = dx, dy, T, seed, ys, lg, where

    def as_dtype(self, dtype):
        """(ys, lgssm) in `dtype`: exact for fp32, the inputs are fp32-representable"""
        return self.ys.astype(dtype), tuple(np.ascontiguousarray(a, dtype) for a in self.lg)

    def observed_fraction(self):
        return float(np.mean(np.all(np.isfinite(self.ys), axis=-1)))


@functools.lru_cache(maxsize=None)
def case(dx, dy, T, seed=0):
    """One sequence: ys (T, dy) and the LGSSM tuple, fp32-representable fp64.  Read-only."""
    rng = np.random.default_rng([dx, dy, T, seed])
    lg = _model(rng, T, dx, dy)
    ys = rng.standard_normal((T, dy)).astype(np.float32).astype(np.float64)
    where = place_missing(ys, dx + dy + seed)
    for a in lg + (ys,):
        a.flags.writeable = False
    return Case(dx, dy, T, seed, ys, lg, where)


@functools.lru_cache(maxsize=None)
def lanes_case(dx, dy, seed=0):
    """The lanes form: one model per b (B = 64), shared by C = 4 chains; ys (C, T, B, dy), every (c, b) sequence with its own observations and its own rotation of
    the missing rows."""
    T, B, Cn = LANES["T"], LANES["B"], LANES["C"]
    rng = np.random.default_rng([dx, dy, T, B, seed])
    lg = _model(rng, T, dx, dy, (B,))
    ys = rng.standard_normal((Cn, T, B, dy)).astype(np.float32).astype(np.float64)
    where = {}
    for c in range(Cn):
        for b in range(B):
            col = ys[c, :, b].copy()
            where[c, b] = place_missing(col, dx + dy + seed + c + 3 * b)
            ys[c, :, b] = col
    for a in lg + (ys,):
        a.flags.writeable = False
    return Case(dx, dy, T, seed, ys, lg, where)


def _ro(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.flags.writeable = False
    return arrays


@functools.lru_cache(maxsize=None)
def reference(cs):
    """(ms, Ps, ell) of the fp64 sequential oracle on the case's (fp32-rounded) inputs.  Cached per case, read-only."""
    return _ro(*K.filtering(cs.ys, cs.lg, False))


@functools.lru_cache(maxsize=None)
def lanes_reference(cs):
    """Per chain c: (ms (T, B, dx), Ps, ell summed over b) of the fp64 sequential batched oracle"""
    return tuple(_ro(*K.filtering(cs.ys[c], cs.lg, False)) for c in range(cs.ys.shape[0]))


def rel_err(got, want):
    """max|got - want| / max|want|; inf if anything in `got` is not finite"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if not np.all(np.isfinite(got)):
        return float("inf")
    return float(np.max(np.abs(got - want)) / np.max(np.abs(want)))


def filter_errors(got, want):
    """(means, covariances, ell) errors of a filter result against a reference triple"""
    return tuple(rel_err(g, w) for g, w in zip(got, want))


def _oracle32(ys, lg, parallel):
    ys32, lg32 = ys.astype(np.float32), tuple(a.astype(np.float32) for a in lg)
    ms, Ps, ell = K.filtering(ys32, lg32, parallel)
    assert ms.dtype == np.float32 and Ps.dtype == np.float32 and np.asarray(ell).dtype == np.float32   # the oracle's arithmetic follows its inputs
    return ms, Ps, ell


@functools.lru_cache(maxsize=None)
def _group_error(T, lanes):
    worst = np.zeros(3)
    for dx, dy in PAIRS:
        if lanes:
            cs = lanes_case(dx, dy)
            pairs = [(cs.ys[c], lanes_reference(cs)[c]) for c in range(cs.ys.shape[0])]
        else:
            cs = case(dx, dy, T)
            pairs = [(cs.ys, reference(cs))]
        for ys, ref in pairs:
            for parallel in (False, True):
                worst = np.maximum(worst, filter_errors(_oracle32(ys, cs.lg, parallel), ref))
    print(f"fp32 oracle error, {'lanes ' if lanes else ''}T = {T}, worst of {len(PAIRS)} pairs and both orders: means {worst[0]:.2e}  covariances {worst[1]:.2e}  "
          f"ell {worst[2]:.2e}")
    return tuple(float(w) for w in worst)


def fp32_reference_error(T, form):
    """(means, covariances, ell): the fp32 oracle's own error on the group of cases a form runs -- the 32 one-sequence cases of length T ("seq", "chunk", "tile",
    and the host build), or the 32 lanes cases ("lanes": the oracle's batched filter per chain).  Computed once per session."""
    if form == "lanes":
        assert T == LANES["T"]
    return _group_error(T, form == "lanes")


def check_fp32(got, want, T, form, what=""):
    """The fp32 bar: each of means, covariances, ell at most FP32_FACTOR times the group's reference error.  Prints the ratios, then asserts."""
    errs, bar = filter_errors(got, want), fp32_reference_error(T, form)
    ratios = [e / b for e, b in zip(errs, bar)]
    print(f"{form} {what}: fp32 error / oracle's  means {ratios[0]:.2f}  covariances {ratios[1]:.2f}  ell {ratios[2]:.2f}")
    for name, r, e, b in zip(("means", "covariances", "ell"), ratios, errs, bar):
        assert r <= FP32_FACTOR, f"{form} {what} {name}: error {e:.3e} is {r:.1f} times the fp32 oracle's {b:.3e} (bar: {FP32_FACTOR:g})"
    return ratios


# ---- joint log-density and sampler: the same rule on scalars / paths ------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def logpdf_case(dx, dy, T=70):
    """States near the filtered means (fp32-representable) and the fp64 oracle's posterior_logpdf, prior_logpdf, log_likelihood at them"""
    cs = case(dx, dy, T)
    ms, Ps, ell = reference(cs)
    rng = np.random.default_rng([dx, dy, T, 77])
    xs = (ms + 0.3 * rng.standard_normal(ms.shape)).astype(np.float32).astype(np.float64)
    want = (K.posterior_logpdf(cs.ys, xs, ell, cs.lg), K.prior_logpdf(xs, cs.lg), K.log_likelihood(cs.ys, xs, cs.lg))
    _ro(xs)
    return xs, tuple(float(w) for w in want)


def oracle_logpdfs(ys, xs, ell, lg, dtype):
    c = lambda a: np.asarray(a, dtype)
    lg = tuple(c(a) for a in lg)
    return (K.posterior_logpdf(c(ys), c(xs), c(ell), lg), K.prior_logpdf(c(xs), lg), K.log_likelihood(c(ys), c(xs), lg))


@functools.lru_cache(maxsize=None)
def fp32_logpdf_error(T=70):
    """(posterior_logpdf, prior_logpdf, log_likelihood, joint): |oracle in fp32 - oracle in fp64| / |fp64|, the worst over the 32 pairs"""
    worst = np.zeros(4)
    for dx, dy in PAIRS:
        cs = case(dx, dy, T)
        xs, want = logpdf_case(dx, dy, T)
        got = oracle_logpdfs(cs.ys, xs, reference(cs)[2], cs.lg, np.float32)
        errs = [rel_err(g, w) for g, w in zip(got, want)]
        errs.append(rel_err(got[1] + got[2], want[1] + want[2]))
        worst = np.maximum(worst, errs)
    print(f"fp32 oracle error, log-densities at T = {T}, worst of {len(PAIRS)} pairs: posterior {worst[0]:.2e}  prior {worst[1]:.2e}  log-likelihood {worst[2]:.2e}  "
          f"joint {worst[3]:.2e}")
    return tuple(float(w) for w in worst)


SAMPLER_DY = 2


@functools.lru_cache(maxsize=None)
def sampler_case(dx, T):
    """The oracle's filtered moments of case(dx, SAMPLER_DY, T), N(0, I) draws (fp32-representable) and the fp64 oracle's path for both orders"""
    cs = case(dx, SAMPLER_DY, T)
    ms, Ps, _ = reference(cs)
    ms, Ps = ms.astype(np.float32).astype(np.float64), Ps.astype(np.float32).astype(np.float64)
    eps = np.random.default_rng([dx, T, 78]).standard_normal((T, dx)).astype(np.float32).astype(np.float64)
    want = {par: K.sampling(eps, ms, Ps, cs.lg, par) for par in (False, True)}
    _ro(ms, Ps, eps, *want.values())
    return cs, ms, Ps, eps, want


@functools.lru_cache(maxsize=None)
def fp32_sampler_error(T):
    """max|K.sampling in fp32 - in fp64| / max|fp64|: the larger of the two orders, the worst over dx = 1..4"""
    worst = 0.0
    f = lambda a: np.asarray(a, np.float32)
    for dx in range(1, 5):
        cs, ms, Ps, eps, want = sampler_case(dx, T)
        for par in (False, True):
            xs = K.sampling(f(eps), f(ms), f(Ps), tuple(f(a) for a in cs.lg), par)
            assert xs.dtype == np.float32
            worst = max(worst, rel_err(xs, want[False]))
    print(f"fp32 oracle error, sampler at T = {T}, worst of dx 1..4 and both orders: {worst:.2e}")
    return worst
