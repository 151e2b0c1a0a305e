"""ORACLE -- TEST INFRASTRUCTURE ONLY (never imported by the product package).

LITERAL NumPy restatement of the reference's PARALLEL-IN-TIME conditional SMC (conditional dSMC), in the reference's own arithmetic order
and with the reference's own tree: every array padded to 2^K along time (NaN for floats), whole blocks of trajectories, origins, keys and
parameters gathered and concatenated at every stitch, nodes whose right child is padding passed through unchanged, N conditional draws per
stitch and ONE unconditional draw at the root.  It evaluates GENERIC Python protocol objects (`Mt[t]` per time step, `G0`, `Gt` with
`.params`, optional `Qt[t]`) and reuses `logsumexp`, `choice`, `multinomial`, `norm_logpdf` and the protocol / model objects of
`oracle/csmc_np.py`.  It stands beside `oracle/csmc_ref.c::csmc_ref_pit_sweep`, the co-designed CONTRACT oracle of csrc/pit.hip (unnormalised
`exp(v - max)`, 64 / 256 / 1024 chunks of 8 sub-chunks, a three-level search), and beside the kernels, which keep boundary leaf indices and
slot pairs only: `tests/test_oracle_pit_literal.py` and `tests/test_gpu_pit_literal.py` drive all three with the same explicit noise.

Reference map (all paths relative to the reference's aux_samplers/):
    _primitives/csmc/pit/csmc.py     get_kernel :16-65 (init :60-63 -> `ancestors == 0`, all True), _csmc :68-114
    _primitives/csmc/pit/operator.py operator :39-85, _gather_results :88-111, get_weights_batch :114-130, get_log_weights :133-149
    _primitives/csmc/pit/dc_map.py   _dc_map :73-123 (combine :91-106), _next_power_of_2 :126-135, _passthrough :138-142, _pad :145-154
    _primitives/csmc/resamplings.py  multinomial :14-37 (csmc_np.multinomial)
    csmc/independent.py              _get_parallel_kernel :78-118 (init :113-116 -> `ancestors != 0`, all False), _log_pdf :121-134,
                                     AuxiliaryG0 :163-169, AuxiliaryMtDistribution :202-224, AuxiliaryGt :238-248
Third-party semantics [ext] as in csmc_np.py; in addition
    jax.vmap over a batched dataclass (pit/csmc.py:75,84-85)  -> a Python list of T per-time-step objects, looped over
    vmap(vmap(f, [None, 0, None]), [0, None, None]) (operator.py:141-143) -> W[i, j] = f(x_a[i], x_b[j]): row i evaluated for all j at once
    jnp.take(z, idx, 1) / jnp.unravel_index(idx, (N, N))      -> z[:, idx] / (idx // N, idx % N), C order: pair p = i N + j, i the LEFT slot
    jnp.insert(x, 0, nan_row, axis=0) (pit/csmc.py:98-102)     -> the parameter row the boundary (t-1 | t) reads is row t of the padded
                                                                  tree, i.e. row t - 1 of `Gt.params` (the transition t-1 -> t, y[t])

PRNG.  "Identical PRNG inputs" = the explicit noise arrays of the C ABI (include/auxssm.h, auxssm_csmc_pit_sweep), held in a csmc_np.Noise:
    independent.py:103,106  split(key) -> auxiliary_key -> normal(x.shape)            -> eps_aux (T, d)
    pit/csmc.py:70-72       split(key) -> (sampling_key, resampling_key), each split(., T)
    pit/csmc.py:75          sampling_keys[t] -> Mt[t].sample -> normal((N, d))          -> eps_prop[t]  (T, N, d); slot 0 is overwritten (:78)
    pit/csmc.py:110         resampling_keys[t] travels with time step t through the tree  -> row u_res[t]  (T, N)
    operator.py:77,80       the stitch at the boundary (t-1 | t) draws from keys_b[0], the key of the right block's FIRST step: row u_res[t];
                            the N-draw stitch uses u_res[t, :N] (element 0 is drawn and then overwritten by the pin, resamplings.py:36);
                            the root's scalar choice(shape=()) uses ELEMENT 0 of its row, u_res[mid, 0] (the contract's choice:
                            oracle/csmc_ref.c::csmc_ref_pit_sweep reads u_res[mid * N + n] with n = 0 at the root); row 0 is never read.
"""
import math

import numpy as np

from . import csmc_np as L


# ---- a pytree of arrays with a leading time axis: tuples / lists of arrays, None for "no parameters" --------------------------------------
def _tree(fn, *trees):
    t0 = trees[0]
    if t0 is None:
        return None
    if isinstance(t0, (tuple, list)):
        return tuple(_tree(fn, *(t[i] for t in trees)) for i in range(len(t0)))
    return fn(*(np.asarray(t) for t in trees))


# ---- dc_map.py:126-135, :145-154 -------------------------------------------------------------------------------------------------------
def next_power_of_2(n):
    q, rem, k = n, 0, 0
    while q > 1:
        q, r = divmod(q, 2)
        rem += r
        k += 1
    return 2 ** (k + 1 if rem else k)


def _pad(a, pow_2, T):
    width = [(0, pow_2 - T)] + [(0, 0)] * (a.ndim - 1)
    if np.issubdtype(a.dtype, np.integer):
        return np.pad(a, width, constant_values=0)
    return np.pad(a, width, constant_values=np.nan)


class _Node:
    """one element of the tree: a block of consecutive (padded) time steps with everything the reference carries for it"""

    def __init__(self, traj, log_w, origins, keys, params, index):
        self.traj, self.log_w, self.origins, self.keys, self.params, self.index = traj, log_w, origins, keys, params, index


def _concat(a, b, traj_a, org_a, traj_b, org_b, log_w_a, log_w_b):
    return _Node(np.concatenate([traj_a, traj_b]), np.concatenate([log_w_a, log_w_b]), np.concatenate([org_a, org_b]),
                 np.concatenate([a.keys, b.keys]), _tree(lambda p, q: np.concatenate([p, q]), a.params, b.params),
                 np.concatenate([a.index, b.index]))


def _passthrough(a, b):
    """dc_map.py:138-142: both children concatenated unchanged"""
    return _concat(a, b, a.traj, a.origins, b.traj, b.origins, a.log_w, b.log_w)


# ---- operator.py:114-149 ---------------------------------------------------------------------------------------------------------------
def get_log_weights(x_t_1, log_w_t_1, x_t, log_w_t, params_t, log_weight_fn):
    N = x_t_1.shape[0]
    inc = np.empty((N, x_t.shape[0]), x_t.dtype)
    for i in range(N):  # the outer vmap: the left particle i against every right particle j
        inc[i] = log_weight_fn(np.broadcast_to(x_t_1[i], x_t.shape), x_t, params_t)
    return inc + log_w_t_1[:, None] + log_w_t[None, :]


def get_weights_batch(a, b, log_weight_fn):
    params_t = _tree(lambda p: p[0], b.params)
    log_weights = get_log_weights(a.traj[-1], a.log_w[-1], b.traj[0], b.log_w[0], params_t, log_weight_fn)
    return np.exp(log_weights - L.logsumexp(log_weights))


def margins(u, p, idx):
    """for each draw, the distance in fp64 from r = c[-1] (1 - u) to the nearer edge of the cell (c[idx - 1], c[idx]] it fell into, in units
    of c[-1] (c: the cumulative sums `choice` searched).  An index can depend on the order of summation only where this is of the order of
    the rounding of the sums."""
    c = np.cumsum(p).astype(np.float64)
    u, idx = np.atleast_1d(np.asarray(u, np.float64)), np.atleast_1d(idx)
    r = c[-1] * (1.0 - u)
    lo = np.where(idx > 0, c[np.maximum(idx - 1, 0)], 0.0)
    return np.minimum(r - lo, c[idx] - r) / c[-1]


def operator(a, b, log_weight_fn, N, last_step, record):
    """operator.py:39-85 + _gather_results :88-111"""
    weights = get_weights_batch(a, b, log_weight_fn)
    p = np.ravel(weights)
    key = b.keys[0]
    if last_step:
        idx = L.choice(key[0], p)                               # :77, one unconditional draw
        mg = margins(key[0], p, idx)
    else:
        idx = L.multinomial(key, p, N)                          # :80, index 0 pinned to pair 0
        mg = margins(key[1:N], p, idx[1:])                      # (the pinned draw has no cell)
    l_idx, r_idx = idx // N, idx % N                            # unravel_index(idx, (N, N))
    record(int(b.index[0]), l_idx, r_idx, mg)
    nln = -math.log(N)
    return _concat(a, b, np.take(a.traj, l_idx, 1), np.take(a.origins, l_idx, 1), np.take(b.traj, r_idx, 1), np.take(b.origins, r_idx, 1),
                   np.full_like(a.log_w, nln), np.full_like(b.log_w, nln))


# ---- dc_map.py:73-123 ------------------------------------------------------------------------------------------------------------------
def dc_map(leaves, T, op, last_op):
    """leaves: the 2^K one-step nodes of the padded arrays.  Level k pairs neighbouring nodes; a pair is combined where the left node's last
    index and the right node's first index are both < T (:95), otherwise passed through.  (The reference moves the combined pairs in front
    of the unchanged ones, :106; the indices increase, so the combined pairs ARE the leading ones and the order of the nodes is kept.)"""
    nodes, K = list(leaves), int(math.log2(len(leaves) + 0.1))
    for k in range(K):
        merged = []
        for a, b in zip(nodes[::2], nodes[1::2]):
            if k == K - 1:
                merged.append(last_op(a, b))                    # :118-119, no mask at the last level
            elif a.index[-1] < T and b.index[0] < T:
                merged.append(op(a, b))
            else:
                merged.append(_passthrough(a, b))
        nodes = merged
    return nodes[0]


# ---- pit/csmc.py -------------------------------------------------------------------------------------------------------------------------
def get_kernel(Mt, G0, Gt, N, Qt=None):
    """pit/csmc.py:16-65.  Mt (and Qt): a sequence of T per-time-step distributions; kernel(noise, x_star) -> (x, origins, history)"""

    def kernel(key, x_star):
        return _csmc(key, x_star, Mt, G0, Gt, N, Qt)

    def init(x_star):
        return x_star, np.ones(x_star.shape[0], bool)           # :60-63 (ancestors == 0 -> all True)

    return init, kernel


def _csmc(key, x_star, Mt, G0, Gt, N, Qt):
    T = x_star.shape[0]
    xs = np.array([Mt[t].sample(key.eps_prop[t], N) for t in range(T)])     # :75
    xs[:, 0] = x_star                                                       # :78
    if Qt is not None:                                                      # :83-87
        log_wts = np.array([Qt[t].logpdf(xs[t]) for t in range(T)])
        log_wts = log_wts - np.array([Mt[t].logpdf(xs[t]) for t in range(T)])
    else:
        log_wts = np.zeros((T, N), xs.dtype)
    log_wts[0] = log_wts[0] + G0(xs[0])                                     # :89-90
    log_wts = log_wts - np.array([L.logsumexp(log_wts[t]) for t in range(T)])[:, None]  # :91
    origins = np.tile(np.arange(N), (T, 1))                                 # :94
    params = _tree(lambda p: np.insert(p, 0, np.ones_like(p[0]) * np.nan, axis=0), Gt.params)  # :98-102

    def log_weight_fn(x_t_1, x_t, params_t):                                # :104-105
        return Gt(x_t, x_t_1, params_t)

    history = dict(xs=xs.copy(), log_ws=log_wts.copy(), stitches=[])

    def record(t, l_idx, r_idx, mg):
        history["stitches"].append(dict(t=t, left=np.array(l_idx), right=np.array(r_idx), margins=mg))

    pow_2 = next_power_of_2(T)
    padded = [_pad(a, pow_2, T) for a in (xs, log_wts, origins, np.asarray(key.u_res))]
    padded_params = _tree(lambda p: _pad(p, pow_2, T), params)
    leaves = [_Node(*(a[t:t + 1] for a in padded), _tree(lambda p: p[t:t + 1], padded_params), np.arange(t, t + 1)) for t in range(pow_2)]
    root = dc_map(leaves, T, lambda a, b: operator(a, b, log_weight_fn, N, False, record),
                  lambda a, b: operator(a, b, log_weight_fn, N, True, record))
    history["min_margin"] = min(float(s["margins"].min()) for s in history["stitches"] if s["margins"].size)
    return root.traj[:T], root.origins[:T], history                          # dc_map.py:123, pit/csmc.py:113-114


# ---- csmc/independent.py:78-118, :202-224 --------------------------------------------------------------------------------------------------
class AuxiliaryMtDistribution(L.Distribution):
    """one time step of independent.py:202-224: params = (u_t (d,), sqrt_half_delta_t, grad_t (d,) or None)"""

    def __init__(self, params):
        self.params = params

    def _mean(self):
        u_t, sqrt_half_delta, grad_t = self.params
        half_delta = sqrt_half_delta ** 2
        return u_t if grad_t is None else u_t + half_delta * grad_t

    def sample(self, key, N):
        return self._mean()[None, :] + self.params[1] * key

    def logpdf(self, x):
        return np.sum(L.norm_logpdf(x, self._mean(), self.params[1]), axis=-1)


def get_independent_parallel_kernel(M0, G0, Mt, Gt, N, gradient=False, grad=None):
    """independent.py:78-118.  grad: u (T, d) -> the gradient of `_log_pdf` at u in closed form (csmc_np has none of its own: the callers that
    hold particles to 1e-12 pass one, e.g. tests/mvt_np.py::joint_grad); default csmc_np.grad_fd of csmc_np._log_pdf, the stand-in for jax.grad"""

    def factory(u, scale):
        T = u.shape[0]
        if gradient:
            grad_pi = np.asarray(grad(u), u.dtype) if grad is not None else \
                L.grad_fd(lambda v: float(np.sum(L._log_pdf(v.astype(u.dtype), M0, G0, Mt, Gt))), u).astype(u.dtype)
            mt = [AuxiliaryMtDistribution((u[t], scale[t], grad_pi[t])) for t in range(T)]
            qt = [AuxiliaryMtDistribution((u[t], scale[t], None)) for t in range(T)]
        else:
            mt, qt = [AuxiliaryMtDistribution((u[t], scale[t], None)) for t in range(T)], None
        return mt, L.AuxiliaryG0(M0, G0), L.AuxiliaryGt(Mt, Gt), qt

    def kernel(key, x, delta):
        T = x.shape[0]
        sqrt_half_delta = np.sqrt(x.dtype.type(0.5) * np.asarray(delta, x.dtype))
        if np.ndim(sqrt_half_delta) == 0:
            sqrt_half_delta = sqrt_half_delta * np.ones((T,), x.dtype)
        u = x + sqrt_half_delta[:, None] * key.eps_aux                      # :106
        mt, g0, gt, qt = factory(u, sqrt_half_delta)
        _, auxiliary_kernel = get_kernel(mt, g0, gt, N, qt)
        return auxiliary_kernel(key, x)

    def init(x):
        return x, np.zeros(x.shape[0], bool)                                # :113-116 (ancestors != 0 -> all False)

    return init, kernel


# ---- a second, deliberately naive recursion for T = 2^K: no padding, no node records, no parameter tree --------------------------------------
def naive_power_of_two(key, x_star, Mt, G0, Gt, N, Qt=None):
    """the conditional dSMC recursion written top-down for T a power of two: smooth(lo, hi) returns the N trajectories, origins and log-weights
    of the block [lo, hi); a block of one step is the leaf, a longer one stitches its two halves.  Same draws as `_csmc`, shares with it only
    csmc_np's `choice` / `multinomial` / `logsumexp`."""
    T = x_star.shape[0]
    assert T >= 2 and T & (T - 1) == 0

    def leaf(t):
        x = np.array(Mt[t].sample(key.eps_prop[t], N))
        x[0] = x_star[t]
        lw = Qt[t].logpdf(x) - Mt[t].logpdf(x) if Qt is not None else np.zeros(N, x.dtype)
        if t == 0:
            lw = lw + G0(x)
        return x[None], np.arange(N)[None], (lw - L.logsumexp(lw))[None]

    def smooth(lo, hi, root):
        if hi - lo == 1:
            return leaf(lo)
        mid = (lo + hi) // 2
        xa, oa, wa = smooth(lo, mid, False)
        xb, ob, wb = smooth(mid, hi, False)
        par = L._tree_index(Gt.params, mid - 1)
        lw = np.array([[Gt(xb[0][j], xa[-1][i], par) for j in range(N)] for i in range(N)]).reshape(N, N) + wa[-1][:, None] + wb[0][None, :]
        p = np.exp(lw - L.logsumexp(lw)).ravel()
        idx = L.choice(key.u_res[mid][0], p) if root else L.multinomial(key.u_res[mid], p, N)
        i, j = np.divmod(idx, N)
        w = np.full((hi - lo,) + np.shape(idx), -math.log(N))
        return np.concatenate([xa[:, i], xb[:, j]]), np.concatenate([oa[:, i], ob[:, j]]), w

    x, o, _ = smooth(0, T, True)
    return x, o
