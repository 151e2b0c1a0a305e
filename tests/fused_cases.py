"""The cases that tests/test_fused_cases.py (CPU: conditions the oracle alone must meet) and tests/test_gpu_fused_models.py (the HIP kernels of
csrc/fused_shared.h) share: time-varying linear-Gaussian models with dy != dx, data with missing rows and missing components, a real accept / reject mix, and
the chunk geometry of `fs_chunk_len` / `fs_pack` outside the sizes of workloads.lg_model.  Test infrastructure only.

Models (`tv_model`): the time-varying recipe of tests/test_gpu_kalman.py::test_chain_minor_sweep_equals_dense_sweep_and_oracle generalised to po != d; the data
are simulated from the model itself.  tinv: one step's matrices as broadcast views (time stride 0), so the driver's `obs_model_time_invariant` branch is taken
while the missingness still changes from step to step.

Missingness: whole rows with probability 0.12, single components (po > 1) with probability 0.08, and in every case a missing row at t = 0, at the last row
of chunk 0 and the first of chunk 1 (E - 1, E for the case's chunk length E), and at T - 1 -- whole or partial as `Case.forced_rows` says.

Policies: "reference" is oracle/kalman_np.py as it stands (the reference's nansum drops the whole step of the concatenated observation when a component of
y_t is missing, so log alpha != 0 and chains are rejected); "masked" (AUXSSM_NAN_MASKED) scores the finite components of each step under the matching
sub-vector of the mean and sub-block of the covariance -- `masked_log_likelihood` below, used for the target and inside the posterior of the concatenated
model.  Under it the proposal is the exact posterior and log alpha == 0: the independent check that the masked oracle is right.

Noise: `device_noise` restates on the host what the device draws for a case's key (oracle/rng_np.py, stream 0 at the (T, D, C) flat index).

Seeds: per case the smallest of 0, 1, 2, ... that meets the conditions tests/test_fused_cases.py asserts (at least 2 acceptances and 2 rejections among the
checked chains in the first sweep, every margin |log alpha - log u| >= 1e-3 in all three sweeps, at least 7 of 8 margins above FP32_MARGIN)."""
import functools
import math

import numpy as np

from oracle import kalman_np as K
from oracle import rng_np as RN

DELTAS = (0.5, 0.5, 0.2)      # the step sizes of the three consecutive sweeps of a case
MIN_MARGIN = 1e-3             # every checked chain's |log alpha - log u_accept| under the reference policy (the fp64 bar on fused log alpha is 1e-7)
# fp32: the largest |log alpha(unfused fp32 keyed sweep) - log alpha(oracle)| measured over the fp32 runs of tests/test_gpu_fused_models.py on an MI355X
# (B-d4p1-T97-C30, reference policy; the fused sweep's own largest: 3.23e-5), and four times that (the fused sums are ordered differently): fp32 accept flags
# are compared only for chains whose oracle margin exceeds FP32_MARGIN, fused fp32 log alpha is held to the oracle within FP32_MARGIN.
FP32_LOG_ALPHA_ERR = 2.86e-5
FP32_MARGIN = 4 * FP32_LOG_ALPHA_ERR


def chunk_len(C):
    """csrc/fused_shared.h::fs_chunk_len at T <= 130 on a device with >= 4 compute units"""
    return 64 if C >= 1024 else 32 if C >= 96 else 16


# ---- models -------------------------------------------------------------------------------------------------------------------------------------------------
def tv_model(T, d, po, seed, tinv=False):
    """dict(m0, P0, Fs, Qs, bs, Hs, Rs, cs, y, x_true): Fs, Qs, bs (T - 1, ...) and Hs, Rs, cs (T, ...) materialised per step (tinv: broadcast views of one
    step's), y (T, po) without missing values, simulated from the model"""
    rng = np.random.default_rng([seed, T, d, po, int(tinv)])
    n, m = (1, 1) if tinv else (T - 1, T)
    S = rng.standard_normal((d, d))
    Fb = 0.85 * np.eye(d) + 0.1 * (S - S.T)
    Fs = Fb[None] * (1 + 0.1 * rng.standard_normal((n, 1, 1))) + 0.02 * rng.standard_normal((n, d, d))
    A = rng.standard_normal((n, d, 2 * d))
    Qs = 0.05 * A @ A.transpose(0, 2, 1) / d + 0.05 * np.eye(d)
    bs = 0.1 * rng.standard_normal((n, d))
    Hs = np.eye(po, d)[None] + 0.2 * rng.standard_normal((m, po, d))
    B = rng.standard_normal((m, po, 2 * po))
    Rs = 0.2 * B @ B.transpose(0, 2, 1) / po + 0.2 * np.eye(po)
    cs = 0.1 * rng.standard_normal((m, po))
    if tinv:
        Fs, Qs, bs = (np.broadcast_to(a[0], (T - 1,) + a.shape[1:]) for a in (Fs, Qs, bs))
        Hs, Rs, cs = (np.broadcast_to(a[0], (T,) + a.shape[1:]) for a in (Hs, Rs, cs))
    m0, P0 = np.zeros(d), np.eye(d)
    x = np.empty((T, d))
    x[0] = m0 + np.linalg.cholesky(P0) @ rng.standard_normal(d)
    for t in range(1, T):
        x[t] = Fs[t - 1] @ x[t - 1] + bs[t - 1] + np.linalg.cholesky(Qs[t - 1]) @ rng.standard_normal(d)
    y = np.einsum("tij,tj->ti", Hs, x) + cs + np.einsum("tij,tj->ti", np.linalg.cholesky(Rs), rng.standard_normal((T, po)))
    return dict(m0=m0, P0=P0, Fs=Fs, Qs=Qs, bs=bs, Hs=Hs, Rs=Rs, cs=cs, y=y, x_true=x)


def missing(y, forced, rng):
    """y with whole rows (p = 0.12) and single components (po > 1, p = 0.08) set to NaN, then the forced rows {t: "whole" | "partial"}"""
    T, po = y.shape
    out = y.copy()
    out[rng.random(T) < 0.12] = np.nan
    if po > 1:
        out[rng.random((T, po)) < 0.08] = np.nan
    for t, kind in forced.items():
        if kind == "whole":
            out[t] = np.nan
        else:  # exactly one component missing
            out[t] = y[t]
            out[t, t % po] = np.nan
    return out


# ---- the masked-policy oracle ------------------------------------------------------------------------------------------------------------------------------
def masked_log_likelihood(ys, xs, lgssm):
    """sum over the steps of log N(y_t[f]; (H_t x_t + c_t)[f], R_t[f, f]) with f the finite components of y_t; a step with none contributes 0"""
    Hs, Rs, cs = [np.asarray(a) for a in lgssm[5:8]]
    ys, xs = np.asarray(ys), np.asarray(xs)
    res = ys - (np.einsum("tij,tj->ti", Hs, xs) + cs)
    fin = np.isfinite(ys)
    out = 0.0
    for pat in np.unique(fin, axis=0):
        if not pat.any():
            continue
        rows = np.flatnonzero((fin == pat).all(axis=1))
        r = res[rows][:, pat]
        L = np.linalg.cholesky(np.asarray(Rs[rows])[:, pat][:, :, pat])
        z = np.linalg.solve(L, r[..., None])[..., 0]
        out += float(np.sum(-0.5 * np.sum(z * z, -1) - np.sum(np.log(np.diagonal(L, axis1=-2, axis2=-1)), -1) - 0.5 * pat.sum() * math.log(2 * math.pi)))
    return out


def masked_kalman_sweep(x, delta, dynamics_factory, observations_factory, yobs, lgo, parallel, eps_aux, eps_samp, u_accept):
    """oracle/kalman_np.py::kalman_sweep with the reference's nansum-over-steps log-likelihood replaced by `masked_log_likelihood`, in the target and in the
    posterior of the concatenated model alike (the filter and the sampler already treat a missing component as unobserved)"""
    x = np.asarray(x)
    u = x + math.sqrt(0.5 * delta) * eps_aux

    def do_one(xlin, x_prop=None):
        m0, P0, Fs, Qs, bs, *_ = dynamics_factory(xlin)
        ys, Hs, Rs, cs, *_ = observations_factory(xlin, u, delta)
        lg = (m0, P0, Fs, Qs, bs, Hs, Rs, cs)
        ms, Ps, ell = K.filtering(ys, lg, parallel)
        if x_prop is None:
            x_prop = K.sampling(eps_samp, ms, Ps, lg, parallel)
        return masked_log_likelihood(ys, x_prop, lg) - ell + K.prior_logpdf(x_prop, lg), masked_log_likelihood(yobs, x_prop, lgo) + K.prior_logpdf(x_prop, lgo), x_prop

    lp_prop, lt_prop, x_prop = do_one(x)
    lp_rev, lt_rev, _ = do_one(x_prop, x)
    alpha, log_alpha = K.get_alpha(lp_prop, lp_rev, lt_prop, lt_rev, math.sqrt(delta), u, x, x_prop)
    accepted = bool(u_accept < alpha)
    return dict(x=x_prop if accepted else x, accepted=accepted, x_prop=x_prop, log_alpha=log_alpha, u=u,
                lp_prop=lp_prop, lp_rev=lp_rev, lt_prop=lt_prop, lt_rev=lt_rev)


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, index, group, d, po, T, C, seed, tinv=False, nan_chain=None):
        self.index, self.group, self.d, self.po, self.T, self.C, self.seed, self.tinv, self.nan_chain = index, group, d, po, T, C, seed, tinv, nan_chain
        self.E = chunk_len(C)
        self.id = f"{group}-d{d}p{po}-T{T}-C{C}" + ("-tinv" if tinv else "")

    def __repr__(self):
        return self.id

    @property
    def forced_rows(self):
        """{t: kind}: t = 0 whole or partial alternating by case, the chunk boundary E - 1 | E, and T - 1 (the other kind than t = 0); po = 1 has no partial rows"""
        first = "whole" if self.index % 2 == 0 or self.po == 1 else "partial"
        last = "partial" if first == "whole" and self.po > 1 else "whole"
        return {0: first, self.E - 1: "whole", self.E: "partial" if self.po > 1 else "whole", self.T - 1: last}

    @functools.cached_property
    def m(self):
        return tv_model(self.T, self.d, self.po, self.seed, self.tinv)

    @functools.cached_property
    def y(self):
        y = missing(self.m["y"], self.forced_rows, np.random.default_rng([self.seed, self.index, 1]))
        y.setflags(write=False)
        return y

    @functools.cached_property
    def x0(self):
        rng = np.random.default_rng([self.seed, self.index, 2])
        x0 = self.m["x_true"][None] + 0.3 * rng.standard_normal((self.C, self.T, self.d))
        x0.setflags(write=False)
        return x0

    @property
    def lgo(self):
        m = self.m
        return (m["m0"], m["P0"], m["Fs"], m["Qs"], m["bs"], m["Hs"], m["Rs"], m["cs"])

    def model(self, y=None):
        """a new LGConcatModel of the case (its device buffers are cached per model object)"""
        from aux_ssm_samplers_amd.kalman import LGConcatModel
        return LGConcatModel(*self.lgo, self.y if y is None else y)

    def key(self, i):
        from aux_ssm_samplers_amd import random as R
        return R.PRNGKey(1000 * (self.index + 1) + 10 * self.seed + i)

    @property
    def checked(self):
        """the chains held to the oracle: all of them up to 30 chains; otherwise 12 or a few more -- chains 0 and C - 1, both sides of every 64-lane and
        workgroup boundary (63 | 64, 191 | 192, 255 | 256), the neighbours of the NaN chain of the non-finite redo tests, the rest spread evenly"""
        C = self.C
        if C <= 30:
            return list(range(C))
        s = {0, C - 1}
        for b in (64, 192, 256):
            if b < C:
                s |= {b - 1, b}
        if self.nan_chain is not None:
            s |= {self.nan_chain - 1, self.nan_chain + 1}
        for c in np.linspace(0, C - 1, 12).astype(int):
            if len(s) >= 12:
                break
            if c != self.nan_chain:
                s.add(int(c))
        return sorted(s)

    @property
    def nan_wave(self):
        """the chains that share a wave with the NaN chain: every chain of the packed form (C = 30: two chunks of 32 lanes per wave), the 64 lanes around it
        in the plain one"""
        if self.C <= 32:
            return list(range(self.C))
        w = self.nan_chain // 64
        return list(range(64 * w, min(self.C, 64 * w + 64)))

    def nan_row(self, variant):
        """the time step of the planted NaN: "mid" the middle of chunk 1, "first" the first row of chunk 2 (of chunk 1 where there are only two)"""
        E = self.E
        return E + E // 2 if variant == "mid" else 2 * E if 2 * E < self.T else E

    def oracle_sweep(self, policy, x, delta, eps_aux, eps_samp, u_accept, y=None):
        """one chain's sweep under `policy` on explicit noise: oracle/kalman_np.py::kalman_sweep ("reference") or `masked_kalman_sweep`"""
        model, lgo = self._host_model if y is None else self.model(y), self.lgo
        y = self.y if y is None else y
        if policy == "masked":
            return masked_kalman_sweep(x, delta, model.dynamics_factory, model.observations_factory, y, lgo, True, eps_aux, eps_samp, u_accept)
        return K.kalman_sweep(x, delta, model.dynamics_factory, model.observations_factory, lambda z: K.log_likelihood(y, z, lgo) + K.prior_logpdf(z, lgo), True,
                              eps_aux=eps_aux, eps_samp=eps_samp, u_accept=u_accept)

    @functools.cached_property
    def _host_model(self):
        return self.model()


@functools.lru_cache(maxsize=8)
def device_noise(case, i, dtype=np.float64):
    """(eps_aux (C, T, d), eps_samp (C, T, d), u_accept (C,)) of sweep i of the case: what the device draws from the three children of the sweep's key,
    stream 0 at the (T, D, C) flat index (normals to the tolerance oracle/rng_np.py states, uniforms bit for bit)"""
    from aux_ssm_samplers_amd import random as R
    k_aux, k_samp, k_acc = R.split(case.key(i), 3)
    n = case.T * case.d * case.C
    cm = lambda a: np.ascontiguousarray(a.reshape(case.T, case.d, case.C).transpose(2, 0, 1))
    return cm(RN.normal(k_aux, 0, n, dtype)), cm(RN.normal(k_samp, 0, n, dtype)), RN.uniform(k_acc, 0, case.C, dtype)


@functools.lru_cache(maxsize=None)
def oracle_chain(case, policy, c, sweeps=len(DELTAS)):
    """chain c's consecutive oracle sweeps on the host noise, the state carried from sweep to sweep: a tuple of kalman_sweep dicts plus `margin`"""
    x, out = case.x0[c], []
    for i in range(sweeps):
        ea, es, ua = device_noise(case, i)
        r = case.oracle_sweep(policy, x, DELTAS[i], ea[c], es[c], ua[c])
        r["margin"] = margin(r["log_alpha"], ua[c])
        out.append(r)
        x = r["x"]
    return tuple(out)


def margin(log_alpha, u):
    """distance of log alpha from the accept decision  u < exp(min(0, log alpha))"""
    with np.errstate(divide="ignore"):
        return np.abs(np.asarray(log_alpha, np.float64) - np.log(np.asarray(u, np.float64)))


PAIRS = [(d, po) for d in (1, 2, 3, 4) for po in (1, 2, 3, 4)]
#            (d, po)  T    C    seed
_GROUP_A = [(p, 70, 6, 0) for p in PAIRS]
_GROUP_B = [((3, 2), 64, 4, 0), ((4, 1), 97, 30, 0), ((2, 4), 130, 64, 0), ((3, 3), 97, 128, 0), ((3, 2), 70, 130, 0), ((1, 3), 70, 258, 0), ((4, 4), 130, 1024, 0)]
_GROUP_C = [((2, 3), 70, 6, 0), ((4, 4), 70, 130, 0)]
_NAN_CHAIN = {30: 13, 130: 100, 258: 200}
# the smallest seed that meets the conditions of tests/test_fused_cases.py (0 where not listed)
_SEEDS = {"A-d1p1-T70-C6": 1, "A-d2p3-T70-C6": 1, "A-d3p2-T70-C6": 2, "A-d3p3-T70-C6": 2, "A-d3p4-T70-C6": 1, "A-d4p1-T70-C6": 1, "A-d4p2-T70-C6": 2, "A-d4p3-T70-C6": 2,
          "A-d4p4-T70-C6": 3, "B-d3p2-T64-C4": 3, "B-d3p3-T97-C128": 1, "B-d4p4-T130-C1024": 3, "C-d2p3-T70-C6-tinv": 2, "C-d4p4-T70-C130-tinv": 3}

CASES = []
for _grp, _rows in (("A", _GROUP_A), ("B", _GROUP_B), ("C", _GROUP_C)):
    for (_d, _po), _T, _C, _seed in _rows:
        _c = Case(len(CASES), _grp, _d, _po, _T, _C, _seed, tinv=_grp == "C", nan_chain=_NAN_CHAIN.get(_C) if _grp == "B" else None)
        _c.seed = _SEEDS.get(_c.id, _seed)
        CASES.append(_c)
GROUP_A, GROUP_B, GROUP_C = ([c for c in CASES if c.group == g] for g in "ABC")
NAN_CASES = [c for c in GROUP_B if c.nan_chain is not None]
# (case, dtype name, policy) of the oracle comparisons: A fp64 + fp32 reference; B fp64 both policies + fp32 reference; C fp64 both policies
RUNS = ([(c, dt, "reference") for c in GROUP_A for dt in ("float64", "float32")]
        + [(c, dt, pol) for c in GROUP_B for dt, pol in (("float64", "reference"), ("float64", "masked"), ("float32", "reference"))]
        + [(c, "float64", pol) for c in GROUP_C for pol in ("reference", "masked")])


def run_id(run):
    case, dt, pol = run
    return f"{case.id}-{dt}-{pol}"
