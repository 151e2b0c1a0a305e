/*
 * auxssm.h -- C ABI of libauxssm.so: MI355X (gfx950) native auxiliary-Kalman / conditional-SMC hot path.
 *
 * This is the drop-in boundary for AdrienCorenflos/aux-ssm-samplers.  The reference has no FFI of its
 * own (it is pure Python on JAX); every entry point below replaces the body of one reference function
 * and is what a ctypes binding of that function binds.  See INTEGRATION.md for the reference-side stub.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no C++/torch types.  All functions return 0 on success and a
 *     negative auxssm_status otherwise; auxssm_last_error() returns the message for the calling thread.
 *   - Data pointers of compute entry points are DEVICE pointers (hipMalloc'd, or from auxssm_malloc).
 *     The library never frees caller memory; scratch lives in the handle's workspace, grown on demand.
 *   - One handle = one HIP device + one stream.  Calls on one handle are serialised by the caller and are
 *     asynchronous w.r.t. the host unless stated; auxssm_sync() waits for the handle's stream.
 *   - Shapes.  C = independent chains, T = time steps, B = batched independent LGSSMs (reference
 *     _primitives/kalman/base.py:40-49), dx = state dim, dy = observation dim.  Every array is described by
 *     an auxssm_arr {ptr, chain stride, time stride, batch stride} in ELEMENTS; the trailing matrix/vector
 *     axes are dense row-major.  A stride of 0 broadcasts (e.g. model parameters shared by all chains, or
 *     time-invariant F).  The natural dense layout is (C, T, B, ...).
 *   - dtype: AUXSSM_F32 or AUXSSM_F64 for every real array of a call; ancestors are int32.
 */
#ifndef AUXSSM_H
#define AUXSSM_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AUXSSM_VERSION 108

typedef struct auxssm_ctx* auxssm_handle;

typedef enum { AUXSSM_F32 = 0, AUXSSM_F64 = 1 } auxssm_dtype;

typedef enum {
    AUXSSM_OK = 0,
    AUXSSM_ERR_ARG = -1,      /* bad argument / shape (Python glue raises ValueError) */
    AUXSSM_ERR_UNSUPPORTED = -2, /* (dx, dy) not instantiated in this build */
    AUXSSM_ERR_HIP = -3,      /* HIP runtime error */
    AUXSSM_ERR_NOMEM = -4
} auxssm_status;

/* nansum policy of log_likelihood (reference base.py:137-166): REFERENCE drops a whole time step whose
 * residual has any non-finite component (what jnp.nansum over per-step logpdfs does); MASKED scores the
 * finite components of a partially observed step. */
typedef enum { AUXSSM_NAN_REFERENCE = 0, AUXSSM_NAN_MASKED = 1 } auxssm_nan_policy;

typedef struct {
    const void* ptr;
    int64_t sc; /* chain stride  (elements) */
    int64_t st; /* time stride   (elements) */
    int64_t sb; /* batch stride  (elements) */
} auxssm_arr;

/* LGSSM parameter bundle == reference `LGSSM` NamedTuple (_primitives/kalman/base.py:12-69).
 * m0 (dx) P0 (dx,dx) [no time axis: st ignored]; Fs,Qs (T-1,dx,dx) bs (T-1,dx); Hs (T,dy,dx) Rs (T,dy,dy) cs (T,dy). */
typedef struct {
    auxssm_arr m0, P0, Fs, Qs, bs, Hs, Rs, cs;
} auxssm_lgssm;

typedef struct {
    int32_t C, T, B, dx, dy;
} auxssm_dims;

/* ---- lifecycle ------------------------------------------------------------------------------- */
int auxssm_version(void);
const char* auxssm_last_error(void);
int auxssm_device_count(int* count);
int auxssm_create(int device, auxssm_handle* out);
int auxssm_destroy(auxssm_handle h);
int auxssm_sync(auxssm_handle h);
/* Options of a handle.
 * AUXSSM_OPT_SHARE_MODEL (default 1): in the chain-minor sweep, when the
 *   model's parameter arrays do not depend on the chain (chain stride 0: the factories of a linear-Gaussian model ignore the
 *   linearisation point), everything that depends on the parameters only -- element matrices, gains, Cholesky factors of Q_t /
 *   R_t, the filtered covariances -- is computed once per time step and sweep instead of once per chain (what jax.vmap leaves
 *   unbatched in the reference).  0 forces the general per-chain path.  Results agree to rounding.
 * AUXSSM_OPT_OVERLAP_MODEL_STAGE (default 0 = every call ordered on the one stream; environment AUXSSM_OVERLAP_TAB=1 / 0 changes the default;
 *   the Python host layer, whose every device write goes through an auxssm_* call, switches it on): a chain-shared sweep with a host step
 *   size runs its MODEL STAGE -- the concatenated observation model, the matrix filter on one sequence, the gain / sampler / log-density
 *   tables: everything that reads the model and the step size only -- on a second stream with a double-buffered workspace, so that the stage
 *   of one sweep overlaps the chain passes of the sweep before (same results bit for bit).  The stage runs ahead of earlier SWEEPS only: when
 *   any other call went through the handle since the last such sweep, or once auxssm_stream() has handed the raw stream to the caller (who
 *   may queue work on it the library cannot see), the stage first waits for the tail of the stream.  Still outside the library's sight with
 *   the option on: model arrays written by ANOTHER stream or handle without host synchronisation -- call auxssm_sync first, or leave it 0. */
typedef enum { AUXSSM_OPT_SHARE_MODEL = 1, AUXSSM_OPT_OVERLAP_MODEL_STAGE = 2 } auxssm_option;
int auxssm_set_option(auxssm_handle h, int option, int value);
int auxssm_get_option(auxssm_handle h, int option, int* value);

/* the hipStream_t the handle launches on (as an opaque pointer) */
int auxssm_stream(auxssm_handle h, void** stream);

/* ---- device memory owned by the caller --------------------------------------------------------- */
int auxssm_malloc(auxssm_handle h, size_t bytes, void** dptr);
int auxssm_free(auxssm_handle h, void* dptr);
int auxssm_memcpy_h2d(auxssm_handle h, void* dst, const void* src, size_t bytes); /* synchronous */
int auxssm_memcpy_d2h(auxssm_handle h, void* dst, const void* src, size_t bytes); /* synchronous */
int auxssm_memcpy_d2d(auxssm_handle h, void* dst, const void* src, size_t bytes); /* async on stream */
int auxssm_memset(auxssm_handle h, void* dst, int value, size_t bytes);           /* async on stream */

/* ---- in-library kernel timing with HIP events on the handle's stream ----------------------------
 * kernel_id: one of AUXSSM_K_*.  While enabled, every launch of that kernel group is bracketed by a pair of
 * events from a pool of `max_launches`; read() synchronises and returns the count and the summed ms.
 * AUXSSM_K_ALL brackets every group; read_groups() then returns launches[id] / total_ms[id] for id < n_ids
 * (the event pairs serialise nothing: groups run back to back on one stream anyway). */
typedef enum {
    AUXSSM_K_ALL = -1,
    AUXSSM_K_NONE = 0,
    AUXSSM_K_FILTER_INIT = 1,
    AUXSSM_K_FILTER_SCAN = 2, /* the three launches of the filter's associative scan, timed as one unit */
    AUXSSM_K_FILTER_ELL = 3,  /* chain-shared wide filter: the mean / log-likelihood scan of all sequences (else unused: the scan elements carry the log-likelihood) */
    AUXSSM_K_SAMPLE_INIT = 4,
    AUXSSM_K_SAMPLE_SCAN = 5,
    AUXSSM_K_LOGPDF = 6,
    AUXSSM_K_CSMC_FWD = 7,
    AUXSSM_K_CSMC_BWD = 8,
    AUXSSM_K_PIT_STITCH = 9, /* the log2(T) stitching launches of the parallel-in-time cSMC sweep, timed as one unit */
    AUXSSM_K_RNG = 10,       /* Threefry fills (auxssm_rng_*, auxssm_kalman_draw) */
    AUXSSM_K_SELECT = 11,    /* accept / select step (+ running moments) of the Kalman sweep */
    AUXSSM_K_FACTORY = 12,   /* device factories of a sweep: concatenated / linearised model, observation tables */
    AUXSSM_K_FILTER_TAB = 13,/* chain-shared model: the one-sequence matrix filter and the gain tables derived from it */
    AUXSSM_K_COUNT = 14
} auxssm_kernel_id;
int auxssm_prof_enable(auxssm_handle h, int kernel_id, int max_launches);
int auxssm_prof_read(auxssm_handle h, int* launches, double* total_ms);
int auxssm_prof_read_groups(auxssm_handle h, int n_ids, int* launches /* [n_ids] */, double* total_ms /* [n_ids] */);
int auxssm_prof_disable(auxssm_handle h);

/* ---- Kalman primitives --------------------------------------------------------------------------
 * auxssm_kalman_filter  == filtering(ys, lgssm, parallel)        (_primitives/kalman/filtering.py:18-46)
 *   ys (C,T,B,dy) -> ms (C,T,B,dx), Ps (C,T,B,dx,dx) dense outputs, ell (C) [summed over B, :43-45].
 *   parallel != 0: associative scan over T (filtering.py:49-63); 0: the same kernels run the scan with one
 *   chunk per sequence, i.e. the sequential recursion (filtering.py:66-79).  NaN observations = missing.
 *   Wide states (dx > 4 or dy > 8), parallel != 0, C * B >= 2 sequences whose parameter arrays (P0, Fs, Qs, bs, Hs, Rs, cs) all have chain
 *   and batch stride 0, AUXSSM_OPT_SHARE_MODEL on: the covariance recursion runs ONCE (sequence 0) and every sequence keeps the affine mean /
 *   log-likelihood recursion of the gain form (csrc/wide_shared.h).  That form needs all sequences to miss the same observations; the call
 *   checks it on the device and reads the 4-byte answer back (one stream synchronisation per call), falling back to the per-sequence scan
 *   when they differ.  Same results to rounding.
 */
int auxssm_kalman_filter(auxssm_handle h, int dtype, const auxssm_dims* dims, const auxssm_lgssm* lgssm,
                         const auxssm_arr* ys, int parallel, void* ms, void* Ps, void* ell);

/* auxssm_kalman_sample  == sampling(key, ms, Ps, lgssm, parallel) (_primitives/kalman/sampling.py:11-40)
 *   with the N(0,I) draws given explicitly: eps (C,T,B,dx) dense == jax.random.normal(key, ms.shape) (:128).
 *   ms, Ps dense as produced by auxssm_kalman_filter.  -> xs (C,T,B,dx) dense. */
int auxssm_kalman_sample(auxssm_handle h, int dtype, const auxssm_dims* dims, const auxssm_lgssm* lgssm,
                         const void* ms, const void* Ps, const void* eps, int parallel, void* xs);

/* auxssm_kalman_smooth: the smoothing marginals  sms[t] = E[x_t | y_{0:T-1}],  sPs[t] = Cov[x_t | y_{0:T-1}]  (Rauch-Tung-Striebel) from the filtered moments.
 *   ms (C,T,B,dx), Ps (C,T,B,dx,dx) dense as auxssm_kalman_filter writes them -> sms, sPs of the same shapes; of the model only Fs, Qs, bs are read (any chain or
 *   batch stride, 0 included).  With S_t = sym(F_t P_t F_t^T + Q_t), G_t = P_t F_t^T S_t^-1 (an SPD solve) -- the pathwise sampler's gain (sampling.py:86-98):
 *     sms[t] = m_t + G_t (sms[t+1] - F_t m_t - b_t),   sPs[t] = G_t sPs[t+1] G_t^T + sym(P_t - G_t S_t G_t^T),   sms[T-1] = m_{T-1}, sPs[T-1] = P_{T-1},
 *   run as a backward associative scan over the elements (G, g, L) of the map (sm, sP) -> (G sm + g, G sP G^T + L).  parallel != 0: the chunked or the tile scan,
 *   chosen as for auxssm_kalman_sample; 0: one chunk per sequence, i.e. the sequential recursion.  sPs is symmetric bit for bit.  T = 1 copies.
 *   Refused before anything is enqueued: NULL arguments and sms / sPs overlapping ms / Ps or each other (AUXSSM_ERR_ARG); dx > 4 (AUXSSM_ERR_UNSUPPORTED:
 *   auxssm_kalman_sample covers wide states). */
int auxssm_kalman_smooth(auxssm_handle h, int dtype, const auxssm_dims* dims, const auxssm_lgssm* lgssm,
                         const void* ms, const void* Ps, int parallel, void* sms, void* sPs);

/* auxssm_kalman_dnc_sample == dnc_sampling.sampling(key, ms, Ps, lgssm) (_primitives/kalman/dnc_sampling.py:17-77: the divide-and-conquer pathwise sampler --
 *   leaves _init_elems :128-137, pairwise combination _combination_operator_impl :104-118 with the odd interval carried up :140-169, the two ends :46-68, the
 *   mid-points level by level :70-86) with the N(0, I) draws given explicitly: eps (C,T,dx) dense, time index t is sampled with eps[:, t].  The reference calls it a
 *   proof of concept (:38-41); same distribution as auxssm_kalman_sample.  dx <= 4, B must be 1 (:42-43: AUXSSM_ERR_ARG).  -> xs (C,T,dx) dense.
 *   One stream synchronisation per call (the tree's index plan is uploaded). */
int auxssm_kalman_dnc_sample(auxssm_handle h, int dtype, const auxssm_dims* dims, const auxssm_lgssm* lgssm, const void* ms, const void* Ps, const void* eps, void* xs);

/* auxssm_kalman_joint_logpdf == log_likelihood(ys, xs, lgssm) + prior_logpdf(xs, lgssm)
 *   (_primitives/kalman/base.py:99-166); posterior_logpdf (:72-96) is this minus ell.
 *   xs (C,T,B,dx) described by an auxssm_arr; out (C). */
int auxssm_kalman_joint_logpdf(auxssm_handle h, int dtype, const auxssm_dims* dims, const auxssm_lgssm* lgssm,
                               const auxssm_arr* ys, const auxssm_arr* xs, int nan_policy, void* out);

/* ---- one auxiliary-Kalman MH sweep, fully on device ------------------------------------------------
 * == kernel(key, state, delta) of aux_samplers.kalman.get_kernel (kalman/generic.py:53-76) for models whose
 * factories are the built-in device factory below, for C chains at once.
 *
 * Device factory AUXSSM_KMODEL_LG_CONCAT (linear-Gaussian model, auxiliary observations concatenated with
 * the real ones, the pattern of examples/lorenz/auxiliary_kalman.py:26-35):
 *   dynamics_factory(x)          -> (m0, P0, Fs, Qs, bs)  = `model` dynamics, independent of x
 *   observations_factory(x,u,d)  -> ys = [u_t ; y_t], Hs = [I ; Hobs_t], Rs = blkdiag(d/2 I, Robs_t), cs = [0 ; cobs_t]
 *   log_likelihood_fn(x)         -> prior_logpdf(x) + sum_t log N(y_t; Hobs_t x_t + cobs_t, Robs_t)
 * `model` holds the dynamics and the REAL observation model (dy = dims->dy = p_obs); yobs (T, p_obs).
 * yobs is shared by the chains (chain stride 0).  So is the observation model (Hs, Rs, cs), with one exception: AUXSSM_KMODEL_LG_CONCAT on the register path
 * (dx <= 4, dy <= 4) in AUXSSM_LAYOUT_DENSE reads a per-chain, time-invariant one (chain strides on Hs, Rs, cs, their time strides 0) -- the buffers
 * auxssm_observation_theta_update writes.  Chain strides there in any other case (the chain-minor layout, a time-varying model, the wide-state path, another
 * model kind, auxssm_kalman_sweep_fused) are AUXSSM_ERR_ARG with the reason, nothing enqueued.
 *
 * Noise is explicit (the parity contract): eps_aux, eps_samp (C,T,dx) ~ N(0,I), u_acc (C) ~ U[0,1).
 * x (C,T,dx) is updated in place; accepted (C) int32; logs (C,5) = log_alpha, lp_prop, lp_rev, lt_prop, lt_rev
 * (may be NULL).  B must be 1.
 *
 * layout: AUXSSM_LAYOUT_DENSE -- x, eps_aux, eps_samp are (C,T,dx) row-major and lanes run over time;
 *         AUXSSM_LAYOUT_CHAIN_MINOR -- they are (T,dx,C) row-major (chain index fastest).  Then lanes run over CHAINS: every
 *         per-chain buffer inside the sweep is [t][component][chain], so each wave access is one contiguous run and the
 *         chain-shared model parameters are wave-uniform loads; there is no transposition anywhere in the sweep.  This is the
 *         layout to use with >= 32 chains (bench.py); results are identical up to the combination tree of the scan.  LG_CONCAT and the
 *         SV and LORENZ63_EXT factories (dx <= 4) take it; the wide-state sizes (dx > 4) are dense only.
 * Chain-minor SV sweeps whose observation model differs per chain (second order; first order without chain-shared dynamics) materialise neither the
 * pseudo-observations nor scan elements: the passes fold every step from (x, u, y) (csrc/kalman_bodies.h::FilterOpFlySV).  Wide-state sweeps (dx > 4)
 * of C >= 2 chains on one model (chain stride 0 on every model array) keep ONE copy of the filtered covariances and build the sampler's gains / factors
 * and the log-densities' inverses once per time step, the chains as columns (csrc/wide_shared.h); no sweep synchronises with the host.
 */
typedef enum {
    AUXSSM_KMODEL_LG_CONCAT = 1,
    /* Stochastic volatility y_{t,k} ~ N(0, exp(x_{t,k})) on linear-Gaussian dynamics (`model`: m0, P0, Fs, Qs, bs; Hs/Rs/cs unused),
     * examples/stochastic_volatility/auxiliary_kalman.py:22-48: observations_factory(x, u, d) is the first-order
     * (ys = u + d/2 grad log g(x), R = d/2 I) or second-order (R = (-hess + 2/d I)^-1, ys = R (2u/d + grad - hess x)) auxiliary
     * observation set with H = I, c = 0, rebuilt at both linearisation points (x and x_prop) each sweep;
     * log_likelihood_fn(x) = prior_logpdf(x) + sum log g.  yobs (T, dx), dims->dy = dx; dense or (dx <= 4) chain-minor layout. */
    AUXSSM_KMODEL_SV_FIRST = 2,
    AUXSSM_KMODEL_SV_SECOND = 3,
    /* Stochastic Lorenz-63 (examples/lorenz/auxiliary_kalman.py:14-52, model.py:10-25): dynamics_factory(x) is the first-order
     * extended linearisation (linearisation.py:11-44, analytic Jacobian) of mean(x) = x + dt (phi_0(x) + theta * phi(x)) at every x_t,
     * rebuilt at both linearisation points each sweep; observations_factory concatenates the auxiliary and the real observations as
     * LG_CONCAT does; log_likelihood_fn(x) = log N(x_0; m0, P0) + sum log N(x_{t+1}; mean(x_t), Q) + nansum_t log N(y_t; H_t x_t + c_t, R_t).
     * `model`: m0, P0, Qs as usual; Fs.ptr -> DEVICE array [theta1, theta2, theta3, dt] of `dtype`, chain stride Fs.sc (0: one theta for all chains; 4: one row per chain) (bs unused); Hs, Rs, cs = the
     * real observation model (rows of unobserved steps may be NaN); yobs (T, dy) with NaN = missing; dx = 3, dy <= 3; dense or chain-minor layout. */
    AUXSSM_KMODEL_LORENZ63_EXT = 4,
    /* The spatial example's batched model (examples/spatial/auxiliary_kalman.py:10-66, model.py:103-124): dx independent scalar LGSSMs
     * x_{t+1,k} = F_k x_{t,k} + b_k + N(0, Q_k), x_{0,k} ~ N(m0_k, P0_k), coupled only through the multivariate Student-t potential
     * log g_t(x) = -(nu + dx) / 2 log(1 + (y_t - x)^T prec (y_t - x) / nu), NaN -> 0.  observations_factory(x, u, d) is the first-order
     * (ys = u + d/2 nan_to_num(grad), R = d/2) or second-order (h_k = -nu prec_kk / (nu - 2), Omega_k = 1 / (-h_k + 2/d),
     * ys = Omega (2u/d + grad - h x), R = Omega; needs nu != 2 and -h_k + 2/d > 0) auxiliary observation set with H = 1, c = 0 per component;
     * log_likelihood_fn(x) = sum_k prior_logpdf(x_{.,k}) + sum_t log g_t(x_t).
     * `model`: m0, P0, Fs, Qs, bs point at (dx) VECTORS of `dtype` (the diagonal model; strides ignored); Rs.ptr -> prec (dx, dx) row-major and
     * cs.ptr -> [nu], both DEVICE arrays of `dtype` (Hs unused).  yobs (T, dx) with NaN = missing (a NaN anywhere makes the step's potential flat),
     * dims->dy = dx <= 64; dense layout and nan_policy 0 only (anything else: AUXSSM_ERR_UNSUPPORTED, nothing enqueued); `parallel` is ignored
     * (csrc/kalman_mvt.hip: C * dx scalar recursions of length T). */
    AUXSSM_KMODEL_MVT_FIRST = 5,
    AUXSSM_KMODEL_MVT_SECOND = 6,
    /* Poisson counts y_{t,k} ~ Poisson(exp(x_{t,k})) on linear-Gaussian dynamics: the SV sweep above with the pointwise potential
     * log g_t(x) = sum_k y_k x_k - exp(x_k) (the constant -log y_k! left out, as AUXSSM_POT_POISSON does), grad_k = y_k - exp(x_k), -hess_kk = exp(x_k),
     * all three 0 where y_{t,k} is NaN: a missing count drops that component's term alone and leaves the component observed through u with variance d/2 in
     * both orders (no pseudo-observation is ever NaN).  Same arrays, layouts, widths and checks as SV_FIRST / SV_SECOND; counts must be >= 0 (not
     * checked here) and exp(x) is not guarded against overflow.  Second order is always well defined: -hess = exp(x) > 0. */
    AUXSSM_KMODEL_POISSON_FIRST = 7,
    AUXSSM_KMODEL_POISSON_SECOND = 8,
    /* (9 and 10 are unassigned.)
     * Poisson counts through a loading matrix (the Poisson linear dynamical system): y_{t,j} ~ Poisson(exp(h_j' x_t + c_j)), j = 1..dy, on linear-Gaussian
     * dynamics.  With eta = H x_t + c, e = exp(eta) and every term of a NaN count dropped: log g_t = sum_j y_j eta_j - e_j (the constant -log y_j! left out),
     * grad = H' (y - e), Lam = -hess = H' diag(e) H (symmetric PSD).  observations_factory(x, u, d) is the first-order (ys = u + d/2 grad, R = d/2 I) or
     * second-order (Omega = sym((Lam + 2/d I)^-1), ys = Omega (2u/d + grad + Lam x), R = Omega: dense, one per chain and step) auxiliary observation set with
     * H_obs = I, c_obs = 0; log_likelihood_fn(x) = prior_logpdf(x) + sum_t log g_t.  `model`: m0, P0, Fs, Qs, bs as usual; Hs.ptr -> H (dy, dx) row-major and
     * cs.ptr -> c (dy), both DEVICE arrays of `dtype`, time-invariant and chain-shared (strides ignored; Rs unused).  yobs (T, dy) with NaN = missing, counts
     * >= 0 (not checked here); exp is not guarded against overflow.  dims->dx <= 4, dims->dy <= 1024, dense layout only (anything else: AUXSSM_ERR_UNSUPPORTED;
     * a NULL Hs / cs / yobs: AUXSSM_ERR_ARG; nothing enqueued).  auxssm_kalman_sweep, _dd and _keyed run them (csrc/kalman_plin.hip: one lane per (chain, step),
     * the counts staged through LDS in blocks of 64 channels); auxssm_kalman_sweep_fused refuses them. */
    AUXSSM_KMODEL_POISSON_LIN_FIRST = 11,
    AUXSSM_KMODEL_POISSON_LIN_SECOND = 12,
    /* Binomial and negative-binomial counts with a logit link on linear-Gaussian dynamics: the SV sweep above with the pointwise potential
     * log g_t(x) = sum_k y_k x_k - m_k softplus(x_k), grad_k = y_k - m_k sigma(x_k), -hess_kk = m_k sigma(x_k) (1 - sigma(x_k)) >= 0, where the SIZE m_k is
     * the number of trials n (binomial: y successes of n at probability sigma(x); binary data is n = 1) or y + r (negative binomial: y ~ NB(r, p = sigma(x)),
     * mean r e^x).  The combinatorial constants are left out.  All three are 0 where y_{t,k} is NaN, whatever m is: a missing entry drops that component's
     * term alone and leaves the component observed through u with variance d/2 in both orders (no pseudo-observation is ever NaN).  `model`: m0, P0, Fs, Qs,
     * bs as usual; cs -> m (T, dx), a DEVICE array of `dtype` laid out as yobs is (the same time stride st, components contiguous), shared by the chains (chain stride 0; a
     * NULL cs.ptr, another chain stride or a time stride that is not yobs's: AUXSSM_ERR_ARG, nothing enqueued); Hs, Rs unused.  Same layouts, widths and other checks as SV_FIRST / SV_SECOND;
     * 0 <= y <= m is not checked here.  Evaluated through exp(-|x|): nothing overflows at any x.  auxssm_kalman_sweep, _dd and _keyed run them;
     * auxssm_kalman_sweep_fused refuses them. */
    AUXSSM_KMODEL_LOGISTIC_FIRST = 13,
    AUXSSM_KMODEL_LOGISTIC_SECOND = 14,
    /* Binomial and negative-binomial channels through a loading matrix: POISSON_LIN_* under the logit link of LOGISTIC_*.  With eta = H x_t + c,
     * yy = y where it is finite and 0 where it is NaN, the SIZE m_{t,j} = s_j + w_j yy_{t,j} (binomial: s = trials, w = 0; negative binomial y ~ NB(r, p = sigma(eta)):
     * s = r, w = 1 -- one kind, no branch), e = exp(-|eta|), r = 1 / (1 + e), sigma = eta >= 0 ? r : e r, and every term of a NaN y_{t,j} dropped whatever its
     * size is: log g_t = sum_j yy_j eta_j - m_j (max(eta_j, 0) + log1p(e_j)) (the combinatorial constants left out), grad = H' (yy - m sigma),
     * Lam = -hess = H' diag(m (e r) r) H (symmetric PSD, and Lam <= H' diag(m / 4) H at every x: d <= 4 / lambda_max(H' diag(m) H) is the first order's a-priori
     * step size).  The factories, log_likelihood_fn, the limits (dims->dx <= 4, dims->dy <= 1024, dense layout only: anything else AUXSSM_ERR_UNSUPPORTED), the
     * entries that run them and the fused entry's refusal are POISSON_LIN_*'s.  `model`: m0, P0, Fs, Qs, bs as usual; Hs.ptr -> H (dy, dx) row-major and
     * cs.ptr -> [c; s; w] (3, dy) row-major, both DEVICE arrays of `dtype`, time-invariant and chain-shared (strides ignored; Rs unused; a NULL Hs / cs / yobs:
     * AUXSSM_ERR_ARG, nothing enqueued).  yobs (T, dy) with NaN = missing; 0 <= y (<= trials) and s > 0 are not checked here.  Nothing overflows at any eta.
     * (csrc/kalman_plin.hip::k_plin_obs_logistic: one exponential, one reciprocal and one logarithm per chain, step and channel.) */
    AUXSSM_KMODEL_LOGISTIC_LIN_FIRST = 15,
    AUXSSM_KMODEL_LOGISTIC_LIN_SECOND = 16
} auxssm_kalman_model;
typedef enum { AUXSSM_LAYOUT_DENSE = 0, AUXSSM_LAYOUT_CHAIN_MINOR = 1 } auxssm_layout;
int auxssm_kalman_sweep(auxssm_handle h, int dtype, int model_kind, const auxssm_dims* dims,
                        const auxssm_lgssm* model, const auxssm_arr* yobs, double delta, int parallel,
                        int nan_policy, int layout, void* x, const void* eps_aux, const void* eps_samp, const void* u_acc,
                        int32_t* accepted, void* logs);
/* The same sweep with a DEVICE-RESIDENT step size: delta_dev points at one scalar of `dtype` in device memory (e.g. the array
 * auxssm_delta_adapt updates, m = 1), read by the sweep's kernels on the handle's stream -- the adaptation loop of
 * the experiment drivers under examples/ (common.py:4-32 delta_adaptation between sweeps) then runs without any host round trip.  Results are bit-identical
 * to auxssm_kalman_sweep called with the same value.  delta_dev must hold a value > 0 (not checked: that would need a read-back). */
int auxssm_kalman_sweep_dd(auxssm_handle h, int dtype, int model_kind, const auxssm_dims* dims,
                           const auxssm_lgssm* model, const auxssm_arr* yobs, const void* delta_dev, int parallel,
                           int nan_policy, int layout, void* x, const void* eps_aux, const void* eps_samp, const void* u_acc,
                           int32_t* accepted, void* logs);
/* The sweep as the reference's kernel(key, state, delta) takes it: with the KEYS of its three draws instead of the drawn arrays
 * (keys = {aux0, aux1, samp0, samp1, acc0, acc1}, the three children of the sweep's key, kalman/generic.py:58).  Equivalent to
 * auxssm_kalman_draw(keys, ...) into (eps_aux, eps_samp, u_acc) followed by auxssm_kalman_sweep[_dd] on them -- the three buffers (caller-owned
 * scratch of x's size / C entries) hold exactly those values afterwards -- but the library may generate the noise inside its first
 * consumer instead of in a separate pass (chain-minor LG_CONCAT sweeps with chain-shared parameters do).  delta_dev != NULL: device-resident
 * step size as auxssm_kalman_sweep_dd (delta ignored). */
int auxssm_kalman_sweep_keyed(auxssm_handle h, int dtype, int model_kind, const auxssm_dims* dims,
                              const auxssm_lgssm* model, const auxssm_arr* yobs, double delta, const void* delta_dev,
                              const uint32_t* keys, int parallel, int nan_policy, int layout, void* x, void* eps_aux, void* eps_samp,
                              void* u_acc, int32_t* accepted, void* logs);

/* The keyed LG_CONCAT sweep for chain-shared model parameters in TWO streaming passes over the chains (csrc/fused_shared.h; three up to round 3): the draws, the
 * filter, the pathwise sampler and every log-density of the MH ratio (kalman/generic.py:53-106) are folded into a forward pass over x that emits the auxiliary
 * variables and the sampler's chunk-local increments, and a backward pass that emits x' -- 6 instead of 15 reads / writes of a (C, T, dx) array per sweep, no
 * eps_aux / eps_samp buffers at all.  The chain-independent model stage of the sweep is memoised on the device: rebuilt only when the model arrays, the data or the
 * step size differ byte for byte from what its tables were built from (no host synchronisation).  Same keys -> same draws as auxssm_kalman_sweep_keyed; x' and the five log terms agree with it to rounding
 * (the per-chain totals are summed in a different order).
 *   x, x_alt : two (T, dx, C) chain-minor buffers.
 *   sel == NULL : x is the state (in / out), x_alt scratch for the proposals (accepted chains are copied back by the usual select pass).
 *   sel != NULL : LAZY state -- chain c's current trajectory is x_alt[:, :, c] if sel[c] != 0 else x[:, :, c]; the sweep reads it from there,
 *                 writes the proposal to the other buffer and acceptance flips sel[c]: no select pass.  auxssm_kalman_state_resolve gathers the
 *                 state into x (and zeroes sel) before anything else reads x.
 * Returns AUXSSM_ERR_UNSUPPORTED -- before enqueueing anything -- when the sweep cannot run fused (other model kinds, dense layout, per-chain
 * parameters, AUXSSM_OPT_SHARE_MODEL off, odd chain count, T < 64, parallel == 0, dx > 4 or dy outside 1..4): the caller then runs
 * auxssm_kalman_sweep_keyed.  Running moments (auxssm_stats_attach) are NOT a refusal: attached to `x` they are folded by the sweep (one extra pass over
 * the buffer pair; a rejected chain folds a zero jump and its unchanged state), attached to any other state the call returns AUXSSM_ERR_ARG. */
int auxssm_kalman_sweep_fused(auxssm_handle h, int dtype, int model_kind, const auxssm_dims* dims, const auxssm_lgssm* model,
                              const auxssm_arr* yobs, double delta, const void* delta_dev, const uint32_t* keys, int parallel, int nan_policy,
                              int layout, void* x, void* x_alt, int32_t* sel, void* u_acc, int32_t* accepted, void* logs);
int auxssm_kalman_state_resolve(auxssm_handle h, int dtype, const auxssm_dims* dims, void* x, const void* x_alt, int32_t* sel);

/* ---- conditional SMC (particle Gibbs) sweep ------------------------------------------------------------
 * == kernel(key, state) of aux_samplers._primitives.csmc.get_kernel (csmc.py:16-66: forward pass _csmc :69-107 with
 * conditional multinomial resampling resamplings.py:14-37, then _backward_scanning_pass :110-124 or
 * _backward_sampling_pass :127-149), and -- with proposal = AUX_INDEPENDENT -- kernel(key, state, delta) of
 * aux_samplers.csmc.get_independent_kernel's classical branch (csmc/generic.py:56-72 + csmc/independent.py:57-75,
 * 143-169, 192-198, 238-248), for C chains at once.
 *
 * A Python Mt/Gt object cannot run inside a kernel; the Feynman-Kac model is a closed family instead:
 *   transition  x_t | x_{t-1} ~ N(F x_{t-1} + b, Q)   (time-invariant), initial N(m0, P0)
 *   potential   FLAT: 0 | GAUSS_OBS: log N(y_t; x_t, sig_y^2 I) | SV: sum_k log N(y_{t,k}; 0, exp(x_{t,k})) | GAUSS_OBS_MASKED | MVT: multivariate Student-t
 *               with a precision matrix | LIN_GAUSS: log N(y_t; H x_t + c, R), dy <= dx | POISSON: sum_k [y_{t,k} x_{t,k} - exp(x_{t,k})]
 *               | LOGISTIC: sum_k [y_{t,k} x_{t,k} - m_{t,k} softplus(x_{t,k})], binomial / negative-binomial counts (auxssm_fk_potential below)
 *   proposal    BOOTSTRAP_LG:    M0 = initial, Mt = transition, G0/Gt = potential          (test_csmc/common.py fixtures)
 *               AUX_INDEPENDENT: u = x + sqrt(delta_t/2) eps_aux; M0/Mt = N(u_t, delta_t/2 I);
 *                                G0 = log initial + potential, Gt = log transition + potential, Pt = transition
 * m0, chol_P0 (lower), F, b, chol_Q (lower) are small HOST arrays of doubles; y (T, dx) is a DEVICE array of `dtype`
 * shared by all chains ((2, T, dx) for AUXSSM_POT_LOGISTIC: the data, then the sizes); sqrt_half_delta (T) is a DEVICE array of `dtype` (AUX_INDEPENDENT only).
 *
 * Noise: EXPLICIT device arrays (the parity contract): eps_aux (C,T,dx) [AUX only], eps_prop (C,T,N,dx) ~ N(0,1) (row t
 * feeds M0 / Mt.sample at time t), u_res (C,T-1,N) ~ U[0,1) (row t-1 resamples into time t), u_bwd (C,T) (entry t draws
 * B_t; only entry T-1 is used when backward == 0); or THREEFRY: the same quantities generated in-kernel from
 * (key0, key1) with streams 1..4 of the auxssm_rng_normal/uniform counter space: eps_aux and u_bwd over the same flat
 * indices; eps_prop and u_res with two consecutive time steps sharing one Threefry block (index map in csrc/csmc.hip,
 * k_csmc_fwd), so a THREEFRY run equals an EXPLICIT run on the correspondingly permuted fills.
 *
 * x (C,T,dx): reference trajectories in, new trajectories out.  ancestors (C,T) int32 out (updated = ancestors != 0,
 * csmc.py:59).  xs_out (C,T,N,dx), log_ws_out (C,T,N), As_out (C,T-1,N) int32: optional full particle history
 * (NULL -> kept in the handle's workspace).  N <= 1024.  Arithmetic uses the fixed reduction orders and the
 * bit-reproducible exp/log documented in csrc/csmc.hip, so ancestors are bit-exact against oracle/csmc_ref.c. */
/* AUX_GUIDED (the `csmc-guided` sampler style of the reference's examples, examples/stochastic_volatility/auxiliary_guided_csmc.py on csmc/generic.py:56-72):
 * proposals conditioned on the auxiliary variable AND the parent particle.  With s_t = sqrt(delta_t / 2), u_t = x_t + s_t eps_aux_t, pred / P = m0 / P0 at
 * t = 0 and the transition mean of the parent / Q after:
 *   K_t = P (P + s_t^2 I)^-1,  Lambda_t = P - K_t P,  x_t^i ~ N(mu_t, Lambda_t),  mu_t = pred + K_t (u~_t - pred),
 *   log w = log g_t(x) + log N(x; pred, P) + sum_k log N(x_k; u_{t,k}, s_t^2) - log N(x; mu_t, Lambda_t),  Pt = transition.
 * u~ = u, or with gradient = AUXSSM_GRAD_REFERENCE u + s_t^2 grad_x log g_t(u_t) (the POTENTIAL's gradient only, written once per chain and step; the third
 * term of the weight stays at u).  K_t and chol Lambda_t (a factor with a non-finite entry is replaced by s_t I) are built on the device from chol_P0, chol_Q
 * and sqrt_half_delta at every sweep.  The weights have no reduction-free bound: every step shifts by its exact maximum.  Noise, including eps_aux, as for
 * AUX_INDEPENDENT.  Covered: every potential, LINEAR and LORENZ63_EM transitions at dx <= 4, LINEAR at 4 < dx <= 32 (N <= 64), gradient NONE / REFERENCE.
 * AUXSSM_ERR_UNSUPPORTED: time-varying transitions, auxssm_csmc_sweep_program, auxssm_csmc_pit_sweep.  No contract oracle restates this proposal: parity is
 * against the literal NumPy restatement to rounding, not bit for bit (DESIGN). */
typedef enum { AUXSSM_PROP_BOOTSTRAP_LG = 0, AUXSSM_PROP_AUX_INDEPENDENT = 1, AUXSSM_PROP_AUX_GUIDED = 2 } auxssm_fk_proposal;
typedef enum {
    AUXSSM_POT_FLAT = 0,
    AUXSSM_POT_GAUSS_OBS = 1,        /* y_t ~ N(x_t, sig_y^2 I) */
    AUXSSM_POT_SV = 2,               /* y_{t,k} ~ N(0, exp(x_{t,k})) */
    AUXSSM_POT_GAUSS_OBS_MASKED = 3, /* y_{t,k} ~ N(x_{t,k}, sig_y^2) for the finite y_{t,k} only: missing components / steps skipped
                                        (examples/lorenz/model.py:43-56: x2, x3 observed every 80th step) */
    AUXSSM_POT_MVT = 4,              /* the unnormalised multivariate Student-t log-density with a precision matrix (examples/spatial/t_distribution.py:98-104,
                                        model.py:121-124), the one potential of the family that couples the components of a state:
                                          log g_t(x) = -(nu + dx)/2 log(1 + (x - y_t)^T prec (x - y_t) / nu),  the whole value 0 when it is NaN
                                        (any NaN component of y_t makes the step flat, as the reference's nan_to_num does).  nu > 0, prec symmetric positive definite.
                                        Arithmetic order (every kernel; explicit fma, det_log, no contraction):  r_k = x_k - y_k;  z_k = sum_j fma(prec_kj, r_j, .) with j
                                        ascending from 0;  q = sum_k fma(z_k, r_k, .) with k ascending from 0;  s = 1 + q * (1/nu);  v = -((nu + dx)/2) * det_log(s);
                                        log g = (v == v) ? v : 0.  The constants (nu + dx)/2 and 1/nu are formed once on the host in the sweep's dtype.  Gradient (prec
                                        symmetric):  d log g / dx_k = (-((nu + dx)/2 + (nu + dx)/2) * (1/nu) / s) * z_k = -(nu + dx)/(nu + q) z_k to rounding, every component 0 when s is NaN.
                                        sup_x log g = 0, which is the forward pass's reduction-free bound at dx <= 4; the wide kernels (dx > 4) shift by the exact maximum of every step, the bound being tens of nats above the weights there. */
    AUXSSM_POT_LIN_GAUSS = 5,        /* the linear-Gaussian observation y_t ~ N(H x_t + c, R), H (dy,dx) dense, R (dy,dy) symmetric positive definite, 1 <= dy <= dx:
                                          log g_t(x) = log N(y_t; H x + c, R),  the whole value 0 when it is NaN
                                        (any NaN component of y_t makes the step flat).  The CALLER whitens once, in double, with L = chol(R):
                                          Hw = L^-1 H,  yw_t = L^-1 (y_t - c),  c_lin = -sum_k log L_kk - (dy/2) log 2 pi,   log g_t(x) = c_lin - |yw_t - Hw x|^2 / 2
                                        and passes obs_H = Hw zero-padded to (dx,dx), obs_const = c_lin and y = yw zero-padded to (T,dx), a row of y with any NaN as an all-NaN
                                        row.  The residual form on purpose: information-form quantities around the origin cancel in fp32.
                                        Arithmetic order (every kernel; explicit fma, no contraction; k, j over all dx padded components):
                                          a_k = sum_j fma(H_kj, x_j, .) with j ascending from 0;  z_k = y_{t,k} - a_k;  q = sum_k fma(z_k, z_k, .) with k ascending from 0;
                                          v = fma(-1/2, q, c_lin) = c_lin - q/2 rounded once;  log g = (v == v) ? v : 0.
                                        Gradient:  d log g / dx_j = sum_k fma(H_kj, z_k, .) with k ascending from 0, every component 0 when v is NaN.
                                        sup_x log g <= c_lin (0 on a NaN row), the forward pass's reduction-free bound at dx <= 4; the wide kernels (dx > 4) shift by the exact
                                        maximum of every step, as for AUXSSM_POT_MVT. */
    AUXSSM_POT_POISSON = 6,          /* counts with a log link, y_{t,k} ~ Poisson(exp(x_{t,k})), independent over the components:
                                          log g_t(x) = sum_k [ y_{t,k} x_k - exp(x_k) ]   over the components whose y_{t,k} is finite
                                        (a NaN y_{t,k} drops component k of step t, per component as for AUXSSM_POT_SV -- not the whole-step rule of the coupled kinds).
                                        UNNORMALISED: the constant -sum_k log y_{t,k}! is left out, as the multivariate-t potential leaves out its normaliser; it does
                                        not depend on x and cancels in every normalisation of the weights.  y is not checked on the device: the caller passes finite
                                        entries >= 0 (non-integers are accepted: the formula is the same) or NaN.  An offset (log-exposure) needs no field: it is a
                                        shift of the state, through m0 and b.
                                        Arithmetic order (every kernel; explicit fma, det_exp, no contraction):  e_k = det_exp(x_k);  v_k = fma(y_k, x_k, -e_k);
                                        v_k counts only if y_k - y_k == 0;  log g = sum of the counted v_k, accumulated over k ascending from 0 (from 0).
                                        Gradient:  d log g / dx_k = y_k - det_exp(x_k), 0 for a missing component.
                                        sup_x log g = sum_k (y_k > 0 ? y_k (det_log(y_k) - 1) : 0) (attained at x_k = log y_k; missing components and y_k = 0 add 0), always
                                        finite: the forward pass's reduction-free bound at dx <= 4; the wide kernels (dx > 4) shift by the exact maximum of every step,
                                        as for AUXSSM_POT_MVT and AUXSSM_POT_LIN_GAUSS. */
    /* 7 is unassigned: "unknown potential kind 7" */
    AUXSSM_POT_LOGISTIC = 8          /* counts with a logit link and a SIZE m_{t,k} > 0 beside every observation, independent over the components:
                                          log g_t(x) = sum_k [ y_{t,k} x_k - m_{t,k} softplus(x_k) ]   over the components whose y_{t,k} is finite
                                        -- binomial y ~ Bin(m, sigma(x)) with m = the trials (binary data: m = 1); negative binomial y ~ NB(r, p = sigma(x)) with
                                        m = y + r.  A NaN y_{t,k} drops component k of step t whatever m_{t,k} is; UNNORMALISED (the combinatorial constant is left
                                        out); non-integers are accepted; nothing is checked on the device.
                                        The size adds no field: for THIS kind y is a device array of shape (2, T, dx), plane 0 the data and plane 1 the sizes (0 where
                                        the data is missing), so m_{t,k} = y[(T + t) dx + k].
                                        Arithmetic order (every kernel; explicit fma, det_exp, det_log, no contraction):  e = det_exp(-|x_k|) (<= 1: nothing overflows
                                        at any x);  l = det_log(1 + e);  sp = max(x_k, 0) + l;  v_k = fma(y_k, x_k, -(m_k sp)), counted only if y_k - y_k == 0;
                                        log g = sum of the counted v_k, accumulated over k ascending from 0 (from 0).  There is no det_log1p: det_log(1 + e) carries
                                        an absolute error of at most half an ulp of 1 in softplus, i.e. m_k ulp / 2 in a log-weight.
                                        Gradient:  r = 1 / (1 + e);  s = (x_k >= 0) ? r : e r;  d log g / dx_k = fma(-m_k, s, y_k), 0 for a missing component.
                                        sup_x log g = sum_k b_k over the finite y_k, the binomial log-likelihood at p = y / m written without cancellation,
                                          b_k = (y_k > 0 ? y_k det_log(y_k / m_k) : 0) + (m_k - y_k > 0 ? (m_k - y_k) det_log((m_k - y_k) / m_k) : 0)
                                        (<= 0, always finite; 0 at y = 0 and y = m, where it is approached, not attained): the forward pass's reduction-free bound at
                                        dx <= 4; the wide kernels (dx > 4) shift by the exact maximum of every step, as for AUXSSM_POT_POISSON. */
} auxssm_fk_potential;
/* transition x_{t+1} | x_t ~ N(mean(x_t), Q): LINEAR mean = F x + b; LORENZ63_EM mean = x + dt (phi_0(x) + theta * phi(x)), the
 * Euler-Maruyama step of examples/lorenz/model.py:10-25 (dx = 3; theta = F[0..2], dt = b[0], Q = chol_Q chol_Q^T = dt sigma_x^2 I) */
typedef enum { AUXSSM_TRANS_LINEAR = 0, AUXSSM_TRANS_LORENZ63_EM = 1 } auxssm_fk_transition;
typedef enum { AUXSSM_NOISE_EXPLICIT = 0, AUXSSM_NOISE_THREEFRY = 1 } auxssm_noise_mode;
typedef struct {
    int32_t proposal, potential, dx, transition;
    const double* m0;      /* host (dx) */
    const double* chol_P0; /* host (dx,dx) lower */
    const double* F;       /* host (dx,dx) */
    const double* b;       /* host (dx) */
    const double* chol_Q;  /* host (dx,dx) lower */
    const void* y;         /* device (T,dx), may be NULL for FLAT */
    double sig_y;
    /* Time-varying LINEAR transitions (the reference scans Mt.params over time, _primitives/csmc/csmc.py:103, csmc/base.py:56-71):
     * DEVICE arrays of `dtype`, row t = the transition x_t -> x_{t+1}: F_t (T-1,dx,dx), b_t (T-1,dx), chol_Q_t (T-1,dx,dx) lower.
     * All three NULL: the time-invariant host F / b / chol_Q above; otherwise all three non-NULL (auxssm_csmc_sweep only). */
    const void* F_t;
    const void* b_t;
    const void* chol_Q_t;
    /* Gradient-informed independent proposals (csmc/independent.py:57-75 with gradient=True, :121-134, :173-190, :252-268), AUX_INDEPENDENT
     * only: x_t^i ~ N(u_t + delta_t/2 grad_t, delta_t/2 I) with grad = the gradient at u of the model's joint log-density
     * log M0(u_0) + G0(u_0) + sum_t [log Mt(u_{t+1} | u_t) + Gt(u_{t+1})], evaluated in closed form for the model family.  The weights get the
     * importance correction  sum_k [log N(x_k; u_k, s) - log N(x_k; u_k + delta/2 grad_k, s)]:
     *   AUXSSM_GRAD_REFERENCE  at t = 0 only -- the reference's GradientAuxiliaryGt sums its correction over ALL particles (jnp.sum without
     *                          an axis, :265-266), a constant that cancels in every normalisation, so for t >= 1 it is no correction at all;
     *   AUXSSM_GRAD_EXACT      at every step (the weights the construction intends). */
    int32_t gradient;
    int32_t reserved;
    /* AUXSSM_POT_MVT only (appended: every field above keeps its offset) */
    double nu;             /* degrees of freedom, > 0 */
    const double* prec;    /* host (dx,dx) row-major, symmetric positive definite, like F */
    /* AUXSSM_POT_LIN_GAUSS only (appended likewise) */
    const double* obs_H;   /* host (dx,dx) row-major: the whitened observation matrix L^-1 H, rows beyond dy zero */
    double obs_const;      /* c_lin = -sum_k log L_kk - (dy/2) log 2 pi */
} auxssm_fk_model;
typedef enum { AUXSSM_GRAD_NONE = 0, AUXSSM_GRAD_REFERENCE = 1, AUXSSM_GRAD_EXACT = 2 } auxssm_fk_gradient;
typedef struct {
    int32_t mode;
    uint32_t key0, key1;
    int32_t reserved;
    const void* eps_aux;
    const void* eps_prop;
    const void* u_res;
    const void* u_bwd;
} auxssm_csmc_noise;
/* xs_out / log_ws_out / As_out NULL: the particle systems live in the handle's workspace, T N (dx + 1) reals (+ 4 T N bytes of traced ancestors)
 * per chain.  When those of all C chains exceed what the device has free, the forward + backward pair runs over batches of chains (whole rounds of
 * the chip: one workgroup per chain and CU) -- same results bit for bit, every array and random stream being indexed by the global chain;
 * AUXSSM_ERR_NOMEM only when a single chain does not fit. */
int auxssm_csmc_sweep(auxssm_handle h, int dtype, const auxssm_fk_model* model, int32_t C, int32_t T, int32_t N,
                      int32_t backward, const void* sqrt_half_delta, void* x, const auxssm_csmc_noise* noise,
                      int32_t* ancestors, void* xs_out, void* log_ws_out, int32_t* As_out);

/* ---- user-defined Feynman-Kac models: the sequential sweep compiled at run time ----------------------------------------------
 * == the reference's cSMC kernels on ANY model object that follows its protocol (_primitives/csmc/base.py:18-71), for the models whose
 * potential and / or transition mean can be written as device code.  auxssm_fk_program_compile compiles `source` (hipRTC, gfx950, the flags of
 * the static sweep: -O3 -std=c++17 -ffp-contract=off) together with the sweep kernels of csrc/csmc_sweep.h, every instantiation the launcher may
 * pick (full workgroups of 8 / 16 waves and the generic one, forward and backward).  It needs no handle and no device.  The source defines, at
 * global scope (R = float / double, D = dx):
 *   template <typename R, int D> __device__ R log_g(int t, const R* x, const R* xprev, const R* y, const R* theta);       [AUXSSM_FK_USER_POTENTIAL]
 *   template <typename R, int D> __device__ R log_g_bound(int t, const R* y, const R* theta);                             [optional: sup_x log G_t]
 *   template <typename R, int D> __device__ void mean(int t, const R* xprev, const R* theta, R* mu);                      [AUXSSM_FK_USER_MEAN]
 * (t = the time index of x, resp. of x_t; xprev = x_{t-1}, NULL at t = 0; y = row t of auxssm_fk_user::y or NULL; theta = theta_g / theta_m).
 * With AUXSSM_FK_USER_GRADIENT the program also holds the gradient-informed sweep (model->gradient != AUXSSM_GRAD_NONE), and the source must
 * define the derivative of each user-defined part (a built-in part keeps its closed form):
 *   template <typename R, int D> __device__ void grad_log_g(int t, const R* x, const R* xprev, const R* y, const R* theta, R* gx, R* gxprev);
 *       the partial derivatives of log_g w.r.t. x (gx, D) and xprev (gxprev, D; NULL at t = 0), both zero-filled by the caller   [user potential]
 *   template <typename R, int D> __device__ void mean_vjp(int t, const R* xprev, const R* theta, const R* v, R* out);
 *       out = J^T v, J = d mean(t, xprev) / d xprev                                                                           [user mean]
 * A missing derivative (or one of another signature) returns AUXSSM_ERR_UNSUPPORTED.  The gradient at u is then
 *   d_x log G_t(u_t, u_{t-1}) + d_xprev log G_{t+1}(u_{t+1}, u_t) - Q^-1 (u_t - mean_t(u_{t-1})) + J_{t+1}(u_t)^T Q^-1 (u_{t+1} - mean_{t+1}(u_t)).
 * What the flags leave to the built-in family comes from `model` as in auxssm_csmc_sweep.  include_dir: the directory of csmc_sweep.h.  On a
 * compile error `log` (log_len bytes) receives hipRTC's log and the call returns AUXSSM_ERR_ARG.  dx 1..4.
 * auxssm_csmc_sweep_program: auxssm_csmc_sweep (same arguments, validation, workspace and chain batching) with the program's model; the module is
 * loaded once per handle.  Not covered: time-varying transitions (F_t), and gradient proposals with a program compiled without
 * AUXSSM_FK_USER_GRADIENT (AUXSSM_ERR_UNSUPPORTED). */
typedef struct auxssm_fk_program_s* auxssm_fk_program;
typedef enum { AUXSSM_FK_USER_POTENTIAL = 1, AUXSSM_FK_USER_MEAN = 2, AUXSSM_FK_USER_GRADIENT = 4 } auxssm_fk_program_flag;
typedef struct {
    const void* y;        /* device (T, p) of dtype, shared by all chains, or NULL */
    const void* theta_g;  /* device, the potential's parameters, or NULL */
    const void* theta_m;  /* device, the transition mean's parameters, or NULL */
    int32_t p;
    int32_t reserved;
} auxssm_fk_user;
int auxssm_fk_program_compile(const char* source, const char* include_dir, int dtype, int32_t dx, int32_t flags, char* log, size_t log_len,
                              auxssm_fk_program* out);
int auxssm_fk_program_free(auxssm_fk_program prog);
/* what a compiled program holds: its dtype, dx and flags, and whether the source defines log_g_bound (has_bound 1 / 0); any pointer may be NULL */
int auxssm_fk_program_info(auxssm_fk_program prog, int32_t* dtype, int32_t* dx, int32_t* flags, int32_t* has_bound);
int auxssm_csmc_sweep_program(auxssm_handle h, auxssm_fk_program prog, int dtype, const auxssm_fk_model* model, const auxssm_fk_user* user, int32_t C,
                              int32_t T, int32_t N, int32_t backward, const void* sqrt_half_delta, void* x, const auxssm_csmc_noise* noise,
                              int32_t* ancestors, void* xs_out, void* log_ws_out, int32_t* As_out);

/* ---- particle Gibbs over (x, F, b, Q): the sequential sweep on PER-CHAIN transitions (csrc/csmc_chain.hip) -----------------------------------------
 * auxssm_csmc_sweep_chain_dynamics: auxssm_csmc_sweep -- the same validation, workspace plan, chain batching, noise and outputs, the arguments from C on
 * exactly its own -- with chain c's linear-Gaussian transition x_{t+1} | x_t ~ N(F_c x_t + b_c, chol_Q_c chol_Q_c^T) taken from row c of `dyn`, DEVICE arrays
 * of `dtype` that the caller owns: F (C,dx,dx), b (C,dx), chol_Q (C,dx,dx) lower (the strict upper triangle is not read).  c is the global chain, whatever
 * the batching.  The model's host F / b / chol_Q must still be valid (they are checked) and take no part in the transition; m0 / chol_P0 and the potential
 * are shared by the chains as before.  A chain's sweep is bit for bit the one-chain auxssm_csmc_sweep whose time-varying rows F_t / b_t / chol_Q_t repeat
 * that chain's row T - 1 times, on the chain's slices of the noise (Threefry: on the explicit arrays its streams stand for).  The kernels copy the row into
 * scalar registers once, before their time loop: the sweep costs what the chain-shared one does.
 * Covered: dx <= 4; AUXSSM_PROP_BOOTSTRAP_LG and AUXSSM_PROP_AUX_INDEPENDENT with every gradient mode; the eight potentials; ancestor tracing and backward
 * sampling; fp32 and fp64; both noise modes.  AUXSSM_ERR_UNSUPPORTED before anything is enqueued, with the limit in the message: dx > 4 (the wide-state
 * kernels), AUXSSM_PROP_AUX_GUIDED (its K_t / chol Lambda_t tables would be per chain and step), AUXSSM_TRANS_LORENZ63_EM, F_t / b_t / chol_Q_t set.  User
 * programs and the parallel-in-time sweep have no such entry point.  AUXSSM_ERR_ARG: dyn or one of its arrays NULL, and whatever auxssm_csmc_sweep refuses.
 *
 * auxssm_csmc_dynamics_commit: one launch between auxssm_dynamics_theta_update, which has written its draw of (F, b, Q) | x into STAGING buffers F_new (C,dx,dx),
 * b_new (C,dx), Q_new (C,dx,dx) (chain strides dx dx, dx, dx dx; time stride 0) and its codes into step_flags (C), and the next sweep.  For each chain, in one
 * lane (csrc/chain_dynamics.h, which a host compiler runs too): factor Q_new in double from its values AS ROUNDED TO `dtype` (auxssm_dynamics_theta_update's
 * pivot rule), round the factor to `dtype`, and write the whole quadruple into the live buffers F, b, Q, chol_Q (dyn points at F, b, chol_Q) -- only if the update
 * left the chain unflagged, the factor exists, and every entry of the quadruple is finite in `dtype` with a positive factor diagonal.  Otherwise the live
 * quadruple is untouched and flags[c] holds the update's code (1 - 4) or 5: Q is not positive definite once rounded to `dtype`.  flags[c] = 0 for a committed
 * chain; flags may be step_flags itself.  A sweep therefore never reads a non-finite factor, or an F of one draw beside a Q of another.
 * Refused before anything is enqueued: C < 1, dx < 1, a NULL argument (named), a live buffer that is its own staging buffer (AUXSSM_ERR_ARG); dx > 4
 * (AUXSSM_ERR_UNSUPPORTED). */
typedef struct {
    const void* F;      /* device (C,dx,dx) */
    const void* b;      /* device (C,dx) */
    const void* chol_Q; /* device (C,dx,dx) lower */
} auxssm_fk_chain_dynamics;
int auxssm_csmc_sweep_chain_dynamics(auxssm_handle h, int dtype, const auxssm_fk_model* model, const auxssm_fk_chain_dynamics* dyn, int32_t C, int32_t T,
                                     int32_t N, int32_t backward, const void* sqrt_half_delta, void* x, const auxssm_csmc_noise* noise,
                                     int32_t* ancestors, void* xs_out, void* log_ws_out, int32_t* As_out);
int auxssm_csmc_dynamics_commit(auxssm_handle h, int dtype, int32_t C, int32_t dx, const void* F_new, const void* b_new, const void* Q_new,
                                const int32_t* step_flags, void* F, void* b, void* Q, void* chol_Q, int32_t* flags);

/* ---- parallel-in-time conditional SMC (conditional dSMC) ------------------------------------------------------------
 * == kernel(key, state, delta) of aux_samplers.csmc.get_independent_kernel(..., parallel=True), classical branch
 * (csmc/independent.py:78-118 on _primitives/csmc/pit/csmc.py:69-114, operator.py, dc_map.py), for C chains at once: all T x N
 * proposals x_t^n ~ N(u_t, delta_t/2 I) are drawn at once (slot 0 = the reference trajectory), then a binary tree over time stitches
 * neighbouring blocks: N x N weights G_t(x_t^j, x_{t-1}^i) w_{t-1}^i w_t^j between the left block's last and the right block's first step,
 * N conditional multinomial draws of (i, j) pairs (pair 0 pinned to (0, 0)); the root draws ONE pair and the selected trajectory is
 * read off the tree.  log2(T) launches instead of T sequential steps; work (T - 1) N^2.
 * model: proposal must be AUXSSM_PROP_AUX_INDEPENDENT (the tree needs proposals that are independent across time); any transition /
 * potential of the family.  sqrt_half_delta (T) device.  Noise: EXPLICIT eps_aux (C,T,dx), eps_prop (C,T,N,dx), u_res (C,T,N) [row t
 * feeds the stitch at the boundary (t-1 | t); entry (t, 0) is used by the root only; row 0 never] or THREEFRY (streams 1, 2, 3 at the
 * same flat indices).  x (C,T,dx) in/out; ancestors (C,T) int32 = the leaf particle index selected at each step (updated =
 * ancestors != 0).  T >= 2, 2 <= N <= 1024.  Reduction orders and exp/log are fixed (csrc/pit.hip): bit-exact vs oracle/csmc_ref.c.
 * Covered: dx <= 4 (csrc/pit.hip) -- every transition and potential of the family, gradient NONE / REFERENCE / EXACT (in the tree both are the per-particle
 * correction), N <= 1024; 4 < dx <= 32 (csrc/pit_wide.hip) -- AUXSSM_TRANS_LINEAR, time-invariant or time-varying, the eight built-in potentials, the same
 * gradient modes, 2 <= N <= 64, fp32 and fp64, both noise modes, several chains per launch.  AUXSSM_ERR_UNSUPPORTED, with the limit in the message: dx > 32;
 * at dx > 4, N > 64 and AUXSSM_TRANS_LORENZ63_EM; guided proposals (AUXSSM_PROP_AUX_GUIDED) at any dx.  User programs have no parallel-in-time entry point. */
int auxssm_csmc_pit_sweep(auxssm_handle h, int dtype, const auxssm_fk_model* model, int32_t C, int32_t T, int32_t N,
                          const void* sqrt_half_delta, void* x, const auxssm_csmc_noise* noise, int32_t* ancestors);

/* auxssm_normalize_resample == normalize(log_weights) (_primitives/math/utils.py:23-39) and/or
 * multinomial(key, weights) (_primitives/csmc/resamplings.py:14-37) with the U[0,1) draws given explicitly, for `rows`
 * independent weight vectors of length N <= 1024 (row-major).  Give log_weights (-> normalised weights in weights_out, may be
 * NULL) or already normalised weights; if `indices` is non-NULL the conditional multinomial ancestors (index 0 pinned to 0)
 * are written from `uniforms` (rows, N).  Same reduction orders and exp/log as the cSMC kernels (bit-exact vs oracle). */
int auxssm_normalize_resample(auxssm_handle h, int dtype, int32_t rows, int32_t N, const void* log_weights, const void* weights,
                              const void* uniforms, void* weights_out, int32_t* indices);

/* ---- the MCMC loop around the sweeps: running statistics, step-size adaptation, Lorenz theta step --------------------
 * == the body of `loop` in examples/stochastic_volatility/experiment.py:88-128 and examples/lorenz/experiment.py:120-169
 * (stats_fn :81-83; moving averages :110-113; delta_adaptation aux_samplers/common.py:4-32), kept on the device so that a run of
 * sweeps needs no host round trip.  `iter` is the reference's loop counter i (sweeps already folded in).
 *
 * auxssm_stats_attach: from now on the accept/select step of every auxssm_kalman_sweep on this handle also folds the sweep into the
 *   running means  sq_jump <- (i sq_jump + (x' - x)^2) / (i + 1),  mean <- (i mean + x') / (i + 1),  sq_mean <- (i sq_mean + x'^2) / (i + 1)
 *   (x the state before the sweep, x' after), arrays of x's shape, layout and dtype, and advances i by one; `iter` sets i for the next
 *   sweep.  The moments are bound to ONE resident state: `x` is its device pointer (the `x` argument of the sweeps to fold), `n` = C*T*dx
 *   its element count, `dtype` its type; while attached, an auxssm_kalman_sweep on this handle over any other state (pointer, size or
 *   dtype) returns AUXSSM_ERR_ARG instead of folding.  All three moment pointers NULL detaches (dtype, n, x ignored).  The fold costs no
 *   extra pass over x.
 * auxssm_stats_update: the same fold as a standalone pass over n = C*T*dx elements (cSMC sweeps: keep a copy of x before the sweep).
 * auxssm_accept_update: flags (C, m) int32, nonzero = updated (`accepted` of a Kalman sweep, m = 1; `ancestors` of a cSMC sweep,
 *   m = T, csmc.py:59):  avg <- (i avg + f) / (i + 1),  window <- beta f + (1 - beta) window,  both (C, m) of `dtype`.
 * auxssm_delta_adapt: delta_j <- clip(delta_j exp(rate (mean_c window[c, j] - target)), min_delta, max_delta), j < m: the reference's rule
 *   on the chain-averaged windowed acceptance, because the chains of one sweep call share delta (C = 1: exactly the reference).  delta (m)
 *   and, if non-NULL, sqrt_half_delta (m) = sqrt(delta / 2) (the cSMC sweep's input) are DEVICE arrays of `dtype`.
 * auxssm_lorenz_theta_update: theta | x of the stochastic Lorenz-63 model (examples/lorenz/model.py:59-79: three independent conjugate
 *   linear regressions of dx - dt phi_0(x) on dt phi(x), prior N(0, sigma_theta^2)), then theta = mean + chol * eps
 *   (experiment.py:112-113).  x (C, T, 3) dense or (T, 3, C) chain-minor (`layout`, as the sweep's); eps (C, 3) ~ N(0, 1); par (C, 4) rows [theta1, theta2, theta3, dt]: dt is read, theta
 *   overwritten -- the array model->Fs points at for AUXSSM_KMODEL_LORENZ63_EXT (chain stride 4).  mean_chol (C, 6) out, may be NULL. */
int auxssm_stats_attach(auxssm_handle h, int dtype, int64_t n, const void* x, void* sq_jump, void* mean, void* sq_mean, int64_t iter);
int auxssm_stats_update(auxssm_handle h, int dtype, int64_t n, int64_t iter, const void* x_prev, const void* x_next, void* sq_jump,
                        void* mean, void* sq_mean);
int auxssm_accept_update(auxssm_handle h, int dtype, int32_t C, int32_t m, int64_t iter, double beta, const int32_t* flags, void* avg,
                         void* window);
int auxssm_delta_adapt(auxssm_handle h, int dtype, int32_t C, int32_t m, const void* window, double target, double rate, double min_delta,
                       double max_delta, void* delta, void* sqrt_half_delta);
int auxssm_lorenz_theta_update(auxssm_handle h, int dtype, int32_t C, int32_t T, int layout, const void* x, double sigma_theta,
                               double sigma_x, const void* eps, void* par, void* mean_chol);

/* auxssm_systematic_resample == systematic(key, weights, N) (_primitives/csmc/resamplings.py:40-86): conditional systematic resampling
 * (Chopin & Singh, Algorithm 4) of `rows` independent weight vectors of length M <= 1024 into N <= 1024 indices each, index 0 kept at
 * position 0; uvw (rows, 3) ~ U[0,1)^3 are the three uniforms of :61.  No reference kernel calls it (csmc.py uses multinomial); it
 * completes resamplings.py.  Same cumsum order as the multinomial path (bit-exact vs oracle/csmc_ref.c::csmc_ref_systematic). */
int auxssm_systematic_resample(auxssm_handle h, int dtype, int32_t rows, int32_t M, int32_t N, const void* weights, const void* uvw,
                               int32_t* indices);

/* auxssm_mvn_logpdf == mvn.logpdf(x, m, chol) (_primitives/math/mvn/base.py:15-58, with tril_log_det :108-128) for n independent triplets of
 * dimension dim <= 64: x, m (dim), chol (dim, dim) lower-triangular row-major, triplet g at x + g sx, m + g sm, chol + g sl (ELEMENT strides;
 * 0 broadcasts).  Reference semantics, IEEE-literal: non-finite entries of chol act as +inf in the forward substitution, the dimension
 * counts the finite diagonal entries only, non-finite diagonal entries drop out of the log-determinant.  out (n).
 * Inside the filter / log-density kernels the same function is csrc/kalman_math.h::gauss_logpdf; this is its standalone export
 * (aux_samplers.mvn.logpdf, reference aux_samplers/__init__.py:3). */
int auxssm_mvn_logpdf(auxssm_handle h, int dtype, int64_t n, int32_t dim, const void* x, int64_t sx, const void* m, int64_t sm, const void* chol,
                      int64_t sl, void* out);

/* auxssm_rng_jax: jax.random's own draws -- `jax.vmap(lambda k: jax.random.uniform(k, (n,), dtype, minval, maxval))(keys)` (kind 0) or `... jax.random.normal(k, (n,), dtype)`
 * (kind 1; minval / maxval ignored) for the threefry2x32 implementation in its non-partitionable layout (JAX's default up to 0.4.x; jax/_src/prng.py: threefry_2x32,
 * threefry_random_bits; jax/_src/random.py: _uniform, _normal_real).  keys: DEVICE (nkeys, 2) uint32 (jax.random.split's rows: aux_ssm_samplers_amd.random.jax_split);
 * out[c * key_stride + i * elem_stride], strides in elements.  The reference's call sites: kalman/generic.py:58-61 (split(key, 3), normal(k, x.shape)), :73 (bernoulli),
 * _primitives/kalman/sampling.py:128, csmc/generic.py:64-67, _primitives/csmc/csmc.py:71-85, :129-138 (split per time step; choice = one uniform per index).
 * Pinned by the values JAX's documentation prints for PRNGKey(0) / PRNGKey(42) (tests/test_rng.py); float64 normals agree with XLA's erfinv to rounding. */
int auxssm_rng_jax(auxssm_handle h, int dtype, int kind, int64_t nkeys, int64_t n, const uint32_t* keys, double minval, double maxval, void* out, int64_t key_stride,
                   int64_t elem_stride);

/* auxssm_mvn_optimal_covariance == mvn.get_optimal_covariance(chol_P, chol_Sig) (_primitives/math/mvn/base.py:78-105): the Cholesky factor of the dominating
 * covariance of Section 3 of the paper -- Y = chol_P^-1 chol_Sig, (w, V) = eigh(Y^T Y), w <- min(w, 1), L = chol_Sig V diag(w^-1/2), out = chol(L L^T) -- for
 * dim <= 64 (lower-triangular row-major inputs and output, dim x dim).  vector != 0: the reference's scalar / diagonal branch (:94-95), out = max(chol_P, chol_Sig)
 * elementwise over dim entries.  The symmetric eigen-decomposition is a cyclic Jacobi iteration; the result does not depend on the eigenvectors' order or signs. */
int auxssm_mvn_optimal_covariance(auxssm_handle h, int dtype, int32_t dim, int vector, const void* chol_P, const void* chol_Sig, void* out);

/* auxssm_ess == effective_sample_size(input_array, var) (examples/rare_event/ess.py:28-160: BlackJAX's estimator -- Geyer's initial positive, monotone sequence of
 * paired autocorrelations, autocovariances averaged over the chains -- with the option of dividing by the TRUE variance): a (M chains, N draws, K series) dense,
 * var (K) or NULL, out (K).  Autocovariances by direct sums in double (the reference's FFT to rounding).  N >= 4, K <= 65535. */
int auxssm_ess(auxssm_handle h, int dtype, int64_t M, int64_t N, int64_t K, const void* a, const void* var, void* out);

/* auxssm_linearise == extended / cubature / gauss_hermite(mean, cov, params, x_star, P_star[, order]) (_primitives/linearisation.py:11-44, :78-104, :47-75 on
 * _generic_sigma_points :107-127) for n linearisation points at once, for the conditional means the device knows in closed form (cov(x) = Qc):
 *   AUXSSM_FN_AFFINE    mean(x) = A x + a, A (dim_out, dim), a (dim_out)    (the reference's own test of the three methods, test_linearisation.py:13-48: 4 -> 2)
 *   AUXSSM_FN_LORENZ63  mean(x) = x + dt (phi_0(x) + theta * phi(x)), A = (theta_0, theta_1, theta_2, dt), a unused, dim = dim_out = 3 (examples/lorenz/model.py:10-25)
 * x_star (n, dim) dense; P_star (dim, dim) with point stride sP in elements (0 = one matrix for every point; unused by EXTENDED, may be NULL);
 * GAUSS_HERMITE: `nodes`, `weights` = HOST doubles, the `order`-point rule for N(0, 1) (order <= 8), tensorised on the device (order^dim points);
 * CUBATURE: the 2 dim points +- sqrt(dim) e_i.  EXTENDED uses the analytic Jacobian where the reference differentiates with jacfwd.
 * Out: F (n, dim_out, dim), Q (n, dim_out, dim_out), b (n, dim_out) -- what a dynamics_factory hands to get_kernel.  dim, dim_out <= 4; Qc (dim_out, dim_out). */
typedef enum { AUXSSM_LIN_EXTENDED = 0, AUXSSM_LIN_CUBATURE = 1, AUXSSM_LIN_GAUSS_HERMITE = 2 } auxssm_lin_method;
typedef enum { AUXSSM_FN_AFFINE = 0, AUXSSM_FN_LORENZ63 = 1 } auxssm_lin_fn;
int auxssm_linearise(auxssm_handle h, int dtype, int method, int order, int fn_kind, int64_t n, int32_t dim, int32_t dim_out, const void* A, const void* a,
                     const void* Qc, const void* nodes, const void* weights, const void* x_star, const void* P_star, int64_t sP, void* F, void* Q, void* b);

/* ---- device RNG: Threefry-2x32-20 counter stream -> N(0,1) / U[0,1) fill -----------------------------
 * out[i], i < n, is a pure function of (key0, key1, stream, i) -- number (i & 1) of Threefry block i >> 1: see
 * oracle/rng_np.py for the restatement. */
int auxssm_rng_normal(auxssm_handle h, int dtype, uint32_t key0, uint32_t key1, uint32_t stream, int64_t n, void* out);
/* the noise of one auxssm_kalman_sweep in ONE launch: keys = {aux0, aux1, samp0, samp1, acc0, acc1} (the three children of the sweep's key,
 * kalman/generic.py:58); eps_aux, eps_samp (n) <- auxssm_rng_normal(key, stream 0), u_acc (nu) <- auxssm_rng_uniform(key, stream 0): the same values. */
int auxssm_kalman_draw(auxssm_handle h, int dtype, const uint32_t* keys, int64_t n, int64_t nu, void* eps_aux, void* eps_samp, void* u_acc);
int auxssm_rng_uniform(auxssm_handle h, int dtype, uint32_t key0, uint32_t key1, uint32_t stream, int64_t n, void* out);
/* out (n, m), out[j, i] ~ Gamma(shapes[i], 1): Marsaglia & Tsang (2000), shape < 1 through the draw of shape + 1 times U^(1 / shape).  shapes: m <= 8 HOST
 * doubles, positive.  Draw g = j m + i is a pure function of (key0, key1, stream, g): attempt k < 16 takes its normal from Threefry block 2 (16 g + k) of the
 * stream (the cos branch of the fp64 Box-Muller transform, both dtypes) and its two uniforms (b + 1/2) 2^-32 from the two words of the next block; the first
 * accepted attempt is the draw, NaN if none is (probability < 1e-20).  Arithmetic in double for both dtypes, the acceptance test on csrc/det_math.h's
 * logarithm (the same decision on a host that runs csrc/dynamics_theta.h); the result is rounded to `dtype`.  n m <= 2^42. */
int auxssm_rng_gamma(auxssm_handle h, int dtype, uint32_t key0, uint32_t key1, uint32_t stream, int64_t n, int32_t m, const double* shapes, void* out);

/* ---- theta | x for linear-Gaussian dynamics x_{t+1} = F x_t + b + N(0, Q): the conjugate step on (F, b, Q) (csrc/dynamics_theta.hip) -----------------
 * With z_t = [x_t; 1] (n = dx + 1), A = [F b] (dx x n) and the T - 1 transitions of each chain (x_0's prior takes no part; stationarity is not imposed):
 *   prior       Q ~ IW(nu0, Psi0),  A | Q ~ MN(M0, Q, K0^-1)        K0 (n, n), Psi0 (dx, dx) symmetric positive definite, nu0 > dx - 1
 *   statistics  S_zz = sum z_t z_t^T,  S_xz = sum x_{t+1} z_t^T,  S_xx = sum x_{t+1} x_{t+1}^T
 *   posterior   K_n = K0 + S_zz,  M_n = (M0 K0 + S_xz) K_n^-1,  nu_n = nu0 + T - 1,  Psi_n = sym(Psi0 + S_xx + M0 K0 M0^T - M_n K_n M_n^T)
 *   draw        L = chol(Psi_n), U = chol(K_n), B lower triangular with B_ii = sqrt(chi_scale chi[c, i]), B_ij = eps_w[c, i, j] (i > j):
 *               Q = L B^-T B^-1 L^T (symmetric bit for bit),  A = M_n + chol(Q) eps_a[c] U^-1
 * x: the resident state, (C, T, dx) [AUXSSM_LAYOUT_DENSE] or (T, dx, C) [AUXSSM_LAYOUT_CHAIN_MINOR] of `dtype`; dx <= 4, T >= 2.  Products and sums are formed
 * in double whatever `dtype`; a chain's sums are added in an order that depends on T and the layout alone (segments of the time axis in ascending order, no
 * atomics), so a chain's result is the same alone and inside any batch.
 * auxssm_dynamics_stats: stats_out (C, n n + dx n + dx dx) DEVICE doubles, per chain [S_zz (n, n) | S_xz (dx, n) | S_xx (dx, dx)], each row-major.
 * auxssm_dynamics_theta_update: the noise is explicit -- chi (C, dx) with chi_scale chi[c, i] ~ chi^2(nu_n - i), eps_w (C, dx, dx) (the strict lower triangle
 *   is read) and eps_a (C, dx, n) ~ N(0, 1), DEVICE arrays of `dtype`.  F, b, Q: where chain c's (dx, dx), (dx), (dx, dx) are written, rounded to `dtype`, at
 *   ptr + c * chain stride (time stride 0: time-invariant dynamics; with C > 1 the chain strides must keep the chains apart) -- the arrays model->Fs / bs / Qs of
 *   the next sweep point at.  post_out (C, dx n + n n + 1 + dx dx) DEVICE doubles [M_n | K_n | nu_n | Psi_n], may be NULL.  flags (C) DEVICE int32: 0, or why
 *   chain c was left UNCHANGED -- 1 chol(K_n) failed, 2 chol(Psi_n) failed (or Psi_n's diagonal is rounding noise of the terms it is the difference of),
 *   3 a chi that is not positive and finite, 4 chol(Q) failed or a result is not finite in `dtype`.  A pivot below 2^-46 of its diagonal entry counts as failed.
 *   Nothing non-finite is ever written into F, b, Q.
 * Refused before anything is enqueued: dx > 4 (AUXSSM_ERR_UNSUPPORTED), T < 2, NULL arguments, a prior that is not finite, symmetric, positive definite or has
 * nu0 <= dx - 1, and what one launch cannot hold: C x ceil((T - 1) / 512) > 2^31 - 1, or, chain-minor, C > 65535 x 64 = 4194240 chains. */
typedef struct auxssm_mniw_prior {
    double M0[20];    /* (dx, dx + 1) row-major in the leading entries */
    double K0[25];    /* (dx + 1, dx + 1) row-major in the leading entries */
    double nu0;
    double Psi0[16];  /* (dx, dx) row-major in the leading entries */
    double chi_scale; /* 1: chi holds chi-square draws; 2: chi holds Gamma((nu_n - i) / 2, 1) draws as auxssm_rng_gamma writes them */
} auxssm_mniw_prior;
int auxssm_dynamics_stats(auxssm_handle h, int dtype, int32_t C, int32_t T, int32_t dx, int layout, const void* x, double* stats_out);
int auxssm_dynamics_theta_update(auxssm_handle h, int dtype, int32_t C, int32_t T, int32_t dx, int layout, const void* x, const auxssm_mniw_prior* prior,
                                 const void* chi, const void* eps_w, const void* eps_a, const auxssm_arr* F, const auxssm_arr* b, const auxssm_arr* Q,
                                 double* post_out, int32_t* flags);

/* ---- EM for a time-invariant linear-Gaussian state-space model: the E-step's expected sufficient statistics and the M-step (csrc/lgssm_em.hip) ------------
 * x_0 ~ N(m0, P0), x_{t+1} = F x_t + b + N(0, Q), y_t = H x_t + c + N(0, R); z_t = [x_t; 1], n = dx + 1; dx <= 4, dy <= 8 (the narrow filter's range), T >= 2.
 * auxssm_kalman_smooth_stats: from ys (C,T,B,dy), the filtered covariances Ps and the smoothed moments sms, sPs (dense (C,T,B,.) as auxssm_kalman_filter /
 *   auxssm_kalman_smooth write them; ms is accepted beside them and not read) and the model's Fs, Qs (any chain or batch stride; time stride 0 on Fs, Qs, bs),
 *   for each of the C B sequences
 *     lag one       S_t = sym(F P_t F^T + Q), G_t = P_t F^T S_t^-1 (auxssm_kalman_smooth's gain, recomputed from P_t in double: Cholesky + two triangular solves),
 *                   X_t = Cov[x_{t+1}, x_t | y_{0:T-1}] = sPs[t+1] G_t^T,  t = 0 .. T-2      -> cross_out (C,T-1,B,dx,dx) of `dtype`, or NULL
 *     dynamics      S_zz = sum_{t<T-1} E[z_t z_t^T], S_xz = sum E[x_{t+1} z_t^T], S_xx = sum E[x_{t+1} x_{t+1}^T] with E[x_t x_t^T] = sPs[t] + sms[t] sms[t]^T and
 *                   E[x_{t+1} x_t^T] = X_t + sms[t+1] sms[t]^T: auxssm_dynamics_stats' sums in expectation (S_zz[dx, dx] is the number of transitions, exactly)
 *     observations  over the steps whose row of ys is entirely finite: So_zz = sum E[z_t z_t^T], S_yz = sum y_t E[z_t]^T
 *   -> stats_out (C B, NS) DEVICE doubles, per sequence [S_zz (n,n) | S_xz (dx,n) | S_xx (dx,dx) | So_zz (n,n) | S_yz (dy,n) | sms[0] (dx) | sPs[0] (dx,dx)],
 *   NS = 2 n n + dx n + dx dx + dy n + dx + dx dx.  Products and sums in double whatever `dtype`; a sequence's sums are added in an order that depends on T
 *   alone (lanes over 512-transition segments, a fixed tree inside the workgroup, the segments in ascending order; no atomics): the same bits alone and in a batch.
 *   A step whose S_t cannot be factorised (auxssm_dynamics_theta_update's pivot rule) puts NaN into its X_t and the sums it enters, which the M-step refuses.
 *   Refused before anything is enqueued: NULL arguments, dx > 4 or dy > 8 (AUXSSM_ERR_UNSUPPORTED), T < 2, a time stride other than 0 on Fs, Qs, bs, outputs
 *   overlapping inputs or each other, C B ceil((T-1)/512) > 2^31 - 1.
 * auxssm_lgssm_em_mstep: one small launch.  stats (nseq, NS) as above, added over the sequences in ascending order; syy_nobs: dy dy + 1 HOST doubles
 *   [S_yy = sum y_t y_t^T over the observed steps of all sequences | n_obs, their number]; prior NULL (maximum likelihood) or the matrix-normal inverse-Wishart
 *   prior of the dynamics (its chi_scale is not read).  update_mask: 1 dynamics, 2 observations, 4 initial state.
 *     dynamics      [F b] = S_xz S_zz^-1, Q = sym(S_xx - [F b] S_xz^T) / N_tr;  with a prior the joint mode of auxssm_dynamics_theta_update's posterior:
 *                   [F b] = M_n, Q = Psi_n / (nu_n + dx + n + 1)
 *     observations  [H c] = S_yz So_zz^-1, R = sym(S_yy - [H c] S_yz^T) / n_obs
 *     initial state m0 = mean_s sms_s[0], P0 = mean_s [sPs_s[0] + (sms_s[0] - m0)(sms_s[0] - m0)^T]
 *   Cholesky and triangular solves, no inverse; Q, R, P0 symmetric bit for bit.  F .. P0: where the parameters are written, rounded to `dtype` (->ptr; time stride
 *   0; arrays of blocks outside update_mask may be NULL) -- the arrays the next auxssm_kalman_filter reads.  flags: 4 DEVICE int32 [dynamics, observations,
 *   initial state, reserved = 0]: 0, or why the block was left UNCHANGED -- 1 the Gram matrix (S_zz, K_n, So_zz) could not be factorised or the block has no step,
 *   2 the residual covariance (Q, R, P0) is not positive definite, 3 a result is not finite in `dtype`.  A pivot below 2^-46 of its diagonal entry counts as
 *   failed.  Nothing non-finite is ever written into a model. */
int auxssm_kalman_smooth_stats(auxssm_handle h, int dtype, const auxssm_dims* dims, const auxssm_lgssm* lgssm, const auxssm_arr* ys, const void* ms, const void* Ps,
                               const void* sms, const void* sPs, void* cross_out, double* stats_out);
int auxssm_lgssm_em_mstep(auxssm_handle h, int dtype, int32_t dx, int32_t dy, int32_t nseq, const double* stats, const double* syy_nobs,
                          const auxssm_mniw_prior* prior, int update_mask, const auxssm_arr* F, const auxssm_arr* b, const auxssm_arr* Q, const auxssm_arr* H,
                          const auxssm_arr* c, const auxssm_arr* R, const auxssm_arr* m0, const auxssm_arr* P0, int32_t* flags);

/* ---- theta | x, y for the linear-Gaussian observation model y_t = H x_t + c + N(0, R): the conjugate step on (H, c, R) (csrc/observation_theta.hip) --------
 * With z_t = [x_t; 1] (n = dx + 1), A = [H c] (dy x n) and the steps t = 0 .. T - 1 whose row of yobs is entirely finite (a row with any non-finite entry is
 * skipped whole; n_obs rows remain):
 *   prior       R ~ IW(nu0, Psi0),  A | R ~ MN(M0, R, K0^-1)        K0 (n, n), Psi0 (dy, dy) symmetric positive definite, nu0 > dy - 1; auxssm_mniw_prior
 *               holds them as M0 (dy, n), K0 (n, n), Psi0 (dy, dy) row-major in the leading entries, chi_scale as in auxssm_dynamics_theta_update
 *   statistics  So_zz = sum z_t z_t^T,  S_yz = sum y_t z_t^T  (per chain, on the device: auxssm_kalman_smooth_stats' sums of the same names, without the expectation)
 *   data terms  S_yy = sum y_t y_t^T and n_obs: syy_nobs, dy dy + 1 HOST doubles, as auxssm_lgssm_em_mstep takes them
 *   update_mask 1 (H, c, R jointly)  K_n = K0 + So_zz,  M_n = (M0 K0 + S_yz) K_n^-1,  nu_n = nu0 + n_obs,  Psi_n = sym(Psi0 + S_yy + M0 K0 M0^T - M_n K_n M_n^T)
 *   update_mask 2 (R alone)          nu_n = nu0 + n_obs,  Psi_n = sym(Psi0 + S_yy - A S_yz^T - S_yz A^T + A So_zz A^T) with A the chain's present [H c]; M0 and
 *                                    K0 are neither checked nor read, eps_a may be NULL, H and c keep their bits
 *   draw        L = chol(Psi_n), U = chol(K_n), B lower triangular with B_ii = sqrt(chi_scale chi[c, i]), B_ij = eps_w[c, i, j] (i > j):
 *               R = L B^-T B^-1 L^T (symmetric bit for bit),  A = M_n + chol(R) eps_a[c] U^-1
 * x: the resident state, (C, T, dx) [AUXSSM_LAYOUT_DENSE] or (T, dx, C) [AUXSSM_LAYOUT_CHAIN_MINOR] of `dtype`; yobs (T, dy) of `dtype`, shared by the chains
 * (chain stride 0, time stride >= dy); dx, dy <= 4, T >= 2.  Products and sums are formed in double whatever `dtype`; a chain's sums are added in an order that
 * depends on T and the layout alone (512-step segments of the time axis in ascending order, no atomics): the same bits alone and inside any batch.
 * auxssm_observation_stats: stats_out (C, n n + dy n) DEVICE doubles, per chain [So_zz (n, n) | S_yz (dy, n)], each row-major.
 * auxssm_observation_theta_update: chi (C, dy), eps_w (C, dy, dy) (the strict lower triangle is read), eps_a (C, dy, n): DEVICE arrays of `dtype`.  H, c, R: where
 *   chain c's (dy, dx), (dy), (dy, dy) are written, rounded to `dtype`, at ptr + c * chain stride (time stride 0; with C > 1 the chain strides must keep the chains
 *   apart) -- the arrays model->Hs / cs / Rs of the next AUXSSM_KMODEL_LG_CONCAT sweep point at.  post_out (C, dy n + n n + 1 + dy dy) DEVICE doubles
 *   [M_n | K_n | nu_n | Psi_n] (R alone: [A | So_zz | nu_n | Psi_n]), may be NULL.  flags (C) DEVICE int32: 0, or why chain c was left UNCHANGED -- 1 chol(K_n)
 *   failed or no row is observed, 2 chol(Psi_n) failed (or Psi_n's diagonal is rounding noise of the terms it is the difference of), 3 a chi that is not positive
 *   and finite, 4 chol(R) failed or a result is not finite in `dtype`.  A pivot below 2^-46 of its diagonal entry counts as failed.  Nothing non-finite is ever
 *   written into H, c, R.
 * Refused before anything is enqueued: dx > 4 or dy > 4 (AUXSSM_ERR_UNSUPPORTED), T < 2, NULL arguments, an unknown layout or update_mask, a prior or data
 * terms that are not finite, a prior that is not symmetric, positive definite or has nu0 <= dy - 1 (M0 and K0: update_mask 1 only), yobs with a chain stride
 * other than 0, a time stride other than 0 on H, c, R, chain strides below dy dx, dy, dy dy at C > 1, and what one launch cannot hold:
 * C x ceil(T / 512) > 2^31 - 1, or, chain-minor, C > 65535 x 64 = 4194240 chains.
 * The LG_CONCAT sweep reads such a per-chain observation model (chain strides on Hs, Rs, cs; time stride 0; yobs shared) on its register path
 * (dx <= 4, dy <= 4) in the dense layout; see auxssm_kalman_sweep. */
int auxssm_observation_stats(auxssm_handle h, int dtype, int32_t C, int32_t T, int32_t dx, int32_t dy, int layout, const void* x, const auxssm_arr* yobs,
                             double* stats_out);
int auxssm_observation_theta_update(auxssm_handle h, int dtype, int32_t C, int32_t T, int32_t dx, int32_t dy, int layout, const void* x, const auxssm_arr* yobs,
                                    const double* syy_nobs, const auxssm_mniw_prior* prior, int update_mask, const void* chi, const void* eps_w,
                                    const void* eps_a, const auxssm_arr* H, const auxssm_arr* c, const auxssm_arr* R, double* post_out, int32_t* flags);

#ifdef __cplusplus
}
#endif
#endif /* AUXSSM_H */
