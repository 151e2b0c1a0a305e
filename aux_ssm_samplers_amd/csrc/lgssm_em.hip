// lgssm_em.hip -- EM for a time-invariant linear-Gaussian state-space model on the device: the expected sufficient statistics of the E-step from the filtered
// and smoothed moments (with the lag-one smoothing covariances they need), and the closed-form M-step.  The arithmetic is lgssm_em.h (also compiled by g++ for
// tests/hostsim_lgssm_em).  auxssm_kalman_smooth_stats is three launches:
//   1. dynamics      grid (sequence, time segment), 256 lanes over the segment's transitions (consecutive lanes read consecutive rows): per transition the lag-one
//                    covariance X_t = sP_{t+1} G_t^T from P_t (one SPD solve), then the 45 packed sums (at dx = 4) in registers, products and sums in double
//   2. observations  the same grid over the segment's steps (the last segment also takes step T - 1): So_zz and S_yz over the rows of y that are entirely finite
//                    Both reduce in a fixed order -- a shuffle tree inside each wave, the waves in ascending order through LDS -- and write one packed partial per
//                    (sequence, segment) to the workspace.  No atomics; the segment length depends on T alone (dt_segment_len): a sequence's sums do not depend on its batch.
//   3. reduce        one lane per (sequence, packed sum): the partials added in ascending segment order, written FULL; (sm_0, sP_0) copied beside them
// auxssm_lgssm_em_mstep is one launch of one lane: the sequences' statistics added in ascending order, the selected blocks solved, the parameters rounded to the
// model's dtype and written through their descriptors; a block whose factorisation fails (or whose result is not finite) keeps its values and raises its flag.
// Built with -ffp-contract=off (as dynamics_theta.hip): the sums are then the restatement's expressions.
#include "ctx.h"
#include "lgssm_em.h"

namespace ax {

// block-wide sum of the lanes' packed statistics in a fixed order (dynamics_theta.hip::dt_block_sum): result in sh[0 .. P) after the caller's ascending wave sum
template <int P> __device__ __forceinline__ void em_block_sum(double* acc, double* sh /*[waves][P]*/) {
#pragma unroll
    for (int k = 0; k < P; ++k) {
        double v = acc[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        acc[k] = v;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < P; ++k) sh[wave * P + k] = acc[k];
    }
    __syncthreads();
}
template <int P> __device__ __forceinline__ void em_write_partial(const double* sh, double* out) {
    if (threadIdx.x < P) {
        double s = sh[threadIdx.x];
#pragma unroll
        for (int w = 1; w < EM_THREADS / 64; ++w) s += sh[w * P + threadIdx.x];
        out[threadIdx.x] = s;
    }
}

// where sequence (c, b) lives: its rows of the dense (C, T, B, .) moments are (c T + t) B + b
struct EmSeq {
    int T, B, L, nseg, PP;  // PP: doubles of one packed partial (dynamics + observations)
};

template <typename R, int D, bool CROSS>
__global__ void __launch_bounds__(EM_THREADS) k_em_stats_dyn(EmSeq q, const R* __restrict__ Fp, long long sFc, long long sFb, const R* __restrict__ Qp, long long sQc,
                                                             long long sQb, const R* __restrict__ Ps, const R* __restrict__ sms, const R* __restrict__ sPs,
                                                             R* __restrict__ cross, double* __restrict__ part) {
    constexpr int P = DtDims<D>::PACKED, DD = D * D;
    __shared__ double sh[(EM_THREADS / 64) * P];
    const long long blk = blockIdx.x;
    const int seq = (int)(blk / q.nseg), seg = (int)(blk - (long long)seq * q.nseg);
    const int c = seq / q.B, b = seq - c * q.B;
    const int t0 = seg * q.L, t1 = min(t0 + q.L, q.T - 1);
    double F[DD], Q[DD];
#pragma unroll
    for (int k = 0; k < DD; ++k) F[k] = (double)Fp[c * sFc + b * sFb + k], Q[k] = (double)Qp[c * sQc + b * sQb + k];
    double acc[P];
#pragma unroll
    for (int k = 0; k < P; ++k) acc[k] = 0.0;
    for (int t = t0 + (int)threadIdx.x; t < t1; t += EM_THREADS) {
        const long long r0 = ((long long)c * q.T + t) * q.B + b, r1 = r0 + q.B;
        double Pt[DD], sPt[DD], sPn[DD], smt[D], smn[D], X[DD];
#pragma unroll
        for (int k = 0; k < DD; ++k) Pt[k] = (double)Ps[r0 * DD + k], sPt[k] = (double)sPs[r0 * DD + k], sPn[k] = (double)sPs[r1 * DD + k];
#pragma unroll
        for (int k = 0; k < D; ++k) smt[k] = (double)sms[r0 * D + k], smn[k] = (double)sms[r1 * D + k];
        em_lag_one<D>(F, Q, Pt, sPn, X);
        if (CROSS) {
            const long long rc = ((long long)c * (q.T - 1) + t) * q.B + b;
#pragma unroll
            for (int k = 0; k < DD; ++k) cross[rc * DD + k] = (R)X[k];
        }
        em_acc_dyn<D>(smt, sPt, smn, sPn, X, acc);
    }
    em_block_sum<P>(acc, sh);
    em_write_partial<P>(sh, part + blk * q.PP);
}

template <typename R, int D, int DY>
__global__ void __launch_bounds__(EM_THREADS) k_em_stats_obs(EmSeq q, const R* __restrict__ ys, long long syc, long long syt, long long syb,
                                                             const R* __restrict__ sms, const R* __restrict__ sPs, double* __restrict__ part) {
    constexpr int n = D + 1, P = n * (n + 1) / 2 + DY * n, DD = D * D;
    __shared__ double sh[(EM_THREADS / 64) * P];
    const long long blk = blockIdx.x;
    const int seq = (int)(blk / q.nseg), seg = (int)(blk - (long long)seq * q.nseg);
    const int c = seq / q.B, b = seq - c * q.B;
    const int t0 = seg * q.L, t1 = seg == q.nseg - 1 ? q.T : t0 + q.L;  // the last segment also takes step T - 1
    double acc[P];
#pragma unroll
    for (int k = 0; k < P; ++k) acc[k] = 0.0;
    for (int t = t0 + (int)threadIdx.x; t < t1; t += EM_THREADS) {
        const R* yr = ys + c * syc + (long long)t * syt + b * syb;
        double y[DY];
        bool seen = true;
#pragma unroll
        for (int k = 0; k < DY; ++k) y[k] = (double)yr[k], seen = seen && finite_(y[k]);
        if (!seen) continue;
        const long long r0 = ((long long)c * q.T + t) * q.B + b;
        double sP[DD], sm[D];
#pragma unroll
        for (int k = 0; k < DD; ++k) sP[k] = (double)sPs[r0 * DD + k];
#pragma unroll
        for (int k = 0; k < D; ++k) sm[k] = (double)sms[r0 * D + k];
        em_acc_obs<D, DY>(y, sm, sP, acc);
    }
    em_block_sum<P>(acc, sh);
    em_write_partial<P>(sh, part + blk * q.PP + DtDims<D>::PACKED);
}

// one lane per (sequence, packed sum or entry of (sm_0, sP_0)): ascending segments; a sum goes to its one or two places of the FULL layout
template <typename R, int D>
__global__ void __launch_bounds__(256) k_em_reduce(long long nseq, EmSeq q, int dy, const double* __restrict__ part, const R* __restrict__ sms,
                                                   const R* __restrict__ sPs, double* __restrict__ stats) {
    using S = DtDims<D>;
    constexpr int n = S::n;
    const int OZZ = n * (n + 1) / 2, init = D + D * D, per = q.PP + init, NS = em_ns(D, dy);
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= nseq * per) return;
    const long long s_ = g / per;
    int k = (int)(g - s_ * per);
    double* f = stats + s_ * NS;
    if (k >= q.PP) {  // (sm_0, sP_0) of this sequence
        k -= q.PP;
        const long long c = s_ / q.B, b = s_ - c * q.B, r0 = c * q.T * q.B + b;
        f[S::FULL + em_obs_full(D, dy) + k] = k < D ? (double)sms[r0 * D + k] : (double)sPs[r0 * D * D + (k - D)];
        return;
    }
    double s = 0.0;
    for (int seg = 0; seg < q.nseg; ++seg) s += part[(s_ * q.nseg + seg) * q.PP + k];
    const auto tri_store = [&](double* m, int kk, int ld) {
        int i = 0;
        while (dt_tri(i + 1, 0) <= kk) ++i;
        const int j = kk - dt_tri(i, 0);
        m[i * ld + j] = s;
        m[j * ld + i] = s;
    };
    if (k < S::ZZ) tri_store(f, k, n);
    else if (k < S::ZZ + S::XZ) f[n * n + (k - S::ZZ)] = s;
    else if (k < S::PACKED) tri_store(f + n * n + S::XZ, k - S::ZZ - S::XZ, D);
    else if (k < S::PACKED + OZZ) tri_store(f + S::FULL, k - S::PACKED, n);
    else f[S::FULL + n * n + (k - S::PACKED - OZZ)] = s;
}

template <int DY> struct EmData {
    double Syy[DY * DY], nobs;
};
template <typename R> struct EmOut {
    R *F, *b, *Q, *H, *c, *Rm, *m0, *P0;
};

template <typename R, int D, int DY>
__global__ void __launch_bounds__(64) k_em_mstep(int nseq, const double* __restrict__ stats, EmData<DY> dat, int has_prior, DtPrior<D> pr, int mask, EmOut<R> o,
                                                 int32_t* __restrict__ flags) {
    constexpr int n = D + 1, dy = DY, DF = DtDims<D>::FULL, OF = n * n + DY * n, NT = DF + OF, NS = NT + D + D * D;
    constexpr int RMAX = DY > D ? DY : D;
    // the one lane's matrices live in LDS: it indexes them in loops the compiler need not unroll
    __shared__ double tot[NT], work[EmWork<n, RMAX>::SIZE], coef[RMAX * n], res[RMAX * RMAX], syy[DY * DY];
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    for (int k = 0; k < NT; ++k) {
        double s = 0.0;
        for (int q = 0; q < nseq; ++q) s += stats[(long long)q * NS + k];
        tot[k] = s;
    }
    const auto all_finite = [](const double* a, int m) {
        bool fin = true;
        for (int k = 0; k < m; ++k) fin = fin && finite_(a[k]) && finite_((R)a[k]);  // (rounding to R may overflow a finite double)
        return fin;
    };
    int f_dyn = EM_OK, f_obs = EM_OK, f_init = EM_OK;
    if (mask & EM_DYNAMICS) {
        double *A = coef, *Q = res;
        f_dyn = has_prior ? em_mstep_dyn_map<D>(tot, pr, A, Q) : em_mstep_dyn_ml<D>(tot, A, Q, work);
        if (f_dyn == EM_OK && !(all_finite(A, D * n) && all_finite(Q, D * D))) f_dyn = EM_FAIL_FINITE;
        if (f_dyn == EM_OK)
            for (int i = 0; i < D; ++i) {
                for (int j = 0; j < D; ++j) o.F[i * D + j] = (R)A[i * n + j], o.Q[i * D + j] = (R)Q[i * D + j];
                o.b[i] = (R)A[i * n + D];
            }
    }
    if (mask & EM_OBSERVATIONS) {
        double *HC = coef, *Rr = res;
        for (int k = 0; k < DY * DY; ++k) syy[k] = dat.Syy[k];
        f_obs = em_mstep_obs<D, DY>(tot + DF, syy, dat.nobs, HC, Rr, work);
        if (f_obs == EM_OK && !(all_finite(HC, dy * n) && all_finite(Rr, dy * dy))) f_obs = EM_FAIL_FINITE;
        if (f_obs == EM_OK)
            for (int i = 0; i < dy; ++i) {
                for (int j = 0; j < D; ++j) o.H[i * D + j] = (R)HC[i * n + j];
                o.c[i] = (R)HC[i * n + D];
                for (int j = 0; j < dy; ++j) o.Rm[i * dy + j] = (R)Rr[i * dy + j];
            }
    }
    if (mask & EM_INITIAL) {
        double m0[D], P0[D * D];
        f_init = em_mstep_init<D>(nseq, stats + NT, NS, m0, P0);
        if (f_init == EM_OK && !(all_finite(m0, D) && all_finite(P0, D * D))) f_init = EM_FAIL_FINITE;
        if (f_init == EM_OK)
            for (int i = 0; i < D; ++i) {
                o.m0[i] = (R)m0[i];
                for (int j = 0; j < D; ++j) o.P0[i * D + j] = (R)P0[i * D + j];
            }
    }
    flags[0] = f_dyn, flags[1] = f_obs, flags[2] = f_init, flags[3] = 0;
}

template <typename F> static int em_by_d(int dx, F&& f) {
    switch (dx) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        default: return f(std::integral_constant<int, 4>{});
    }
}
template <typename F> static void em_by_dy(int dy, F&& f) {
    switch (dy) {
        case 1: f(std::integral_constant<int, 1>{}); break;
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 3: f(std::integral_constant<int, 3>{}); break;
        case 4: f(std::integral_constant<int, 4>{}); break;
        case 5: f(std::integral_constant<int, 5>{}); break;
        case 6: f(std::integral_constant<int, 6>{}); break;
        case 7: f(std::integral_constant<int, 7>{}); break;
        default: f(std::integral_constant<int, 8>{}); break;
    }
}

static int em_check_sizes(int dtype, int dx, int dy) {
    if (int rc = check_dtype(dtype)) return rc;
    if (dx < 1 || dy < 1) {
        set_error("need dx >= 1 and dy >= 1 (got dx=%d, dy=%d)", dx, dy);
        return AUXSSM_ERR_ARG;
    }
    if (dx > DT_MAX_D || dy > EM_MAX_DY) {
        set_error("EM covers the narrow filter's range, dx <= %d and dy <= %d (got dx=%d, dy=%d)", DT_MAX_D, EM_MAX_DY, dx, dy);
        return AUXSSM_ERR_UNSUPPORTED;
    }
    return AUXSSM_OK;
}

template <typename R, int D>
static void em_launch_stats(auxssm_ctx* h, const auxssm_dims* dims, const auxssm_lgssm* lg, const auxssm_arr* ys, const void* Ps, const void* sms, const void* sPs,
                            void* cross, double* part, double* stats) {
    const int T = dims->T, dy = dims->dy;
    const long long nseq = (long long)dims->C * dims->B;
    const EmSeq q{T, dims->B, dt_segment_len(T), dt_num_segments(T), DtDims<D>::PACKED + em_obs_packed(D, dy)};
    const dim3 grid((unsigned)(nseq * q.nseg)), block(EM_THREADS);
    const R *F = (const R*)lg->Fs.ptr, *Q = (const R*)lg->Qs.ptr;
    if (cross)
        hipLaunchKernelGGL((k_em_stats_dyn<R, D, true>), grid, block, 0, h->stream, q, F, (long long)lg->Fs.sc, (long long)lg->Fs.sb, Q, (long long)lg->Qs.sc,
                           (long long)lg->Qs.sb, (const R*)Ps, (const R*)sms, (const R*)sPs, (R*)cross, part);
    else
        hipLaunchKernelGGL((k_em_stats_dyn<R, D, false>), grid, block, 0, h->stream, q, F, (long long)lg->Fs.sc, (long long)lg->Fs.sb, Q, (long long)lg->Qs.sc,
                           (long long)lg->Qs.sb, (const R*)Ps, (const R*)sms, (const R*)sPs, (R*)nullptr, part);
    em_by_dy(dy, [&](auto e) {
        constexpr int DY = decltype(e)::value;
        hipLaunchKernelGGL((k_em_stats_obs<R, D, DY>), grid, block, 0, h->stream, q, (const R*)ys->ptr, (long long)ys->sc, (long long)ys->st, (long long)ys->sb,
                           (const R*)sms, (const R*)sPs, part);
    });
    const long long work = nseq * (q.PP + D + D * D);
    hipLaunchKernelGGL((k_em_reduce<R, D>), dim3((unsigned)((work + 255) / 256)), dim3(256), 0, h->stream, nseq, q, dy, (const double*)part, (const R*)sms,
                       (const R*)sPs, stats);
}

// the caller's prior -> the kernels' (dynamics_theta.hip::dt_prior's rules; chi_scale takes no part in a mode), or a message
template <int D> static int em_prior(const auxssm_mniw_prior* p, DtPrior<D>& pr) {
    constexpr int n = D + 1;
    bool fin = std::isfinite(p->nu0);
    for (int k = 0; k < D * n; ++k) fin = fin && std::isfinite(p->M0[k]);
    for (int k = 0; k < n * n; ++k) fin = fin && std::isfinite(p->K0[k]);
    for (int k = 0; k < D * D; ++k) fin = fin && std::isfinite(p->Psi0[k]);
    if (!fin || !(p->nu0 > (double)(D - 1))) {
        set_error("the prior needs finite M0 (%d, %d), K0 (%d, %d), Psi0 (%d, %d) and nu0 > dx - 1 = %d", D, n, n, n, D, D, D - 1);
        return AUXSSM_ERR_ARG;
    }
    for (int k = 0; k < D * n; ++k) pr.M0[k] = p->M0[k];
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) pr.K0[i * n + j] = 0.5 * (p->K0[i * n + j] + p->K0[j * n + i]);
    for (int i = 0; i < D; ++i)
        for (int j = 0; j < D; ++j) pr.Psi0[i * D + j] = 0.5 * (p->Psi0[i * D + j] + p->Psi0[j * D + i]);
    pr.nu0 = p->nu0;
    pr.chi_scale = 1.0;
    double l[n * n];
    if (!dt_chol<n>(pr.K0, l) || !dt_chol<D>(pr.Psi0, l)) {
        set_error("K0 (%d, %d) and Psi0 (%d, %d) must be positive definite", n, n, D, D);
        return AUXSSM_ERR_ARG;
    }
    return AUXSSM_OK;
}

static bool em_overlap(const void* p, size_t np, const void* q, size_t nq) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return p && q && a < b + nq && b < a + np;
}

}  // namespace ax

using namespace ax;

extern "C" {

int auxssm_kalman_smooth_stats(auxssm_handle h, int dtype, const auxssm_dims* dims, const auxssm_lgssm* lgssm, const auxssm_arr* ys, const void* ms, const void* Ps,
                               const void* sms, const void* sPs, void* cross_out, double* stats_out) {
    AX_NEED_H(h);
    if (!dims || !lgssm || !ys || !ys->ptr || !ms || !Ps || !sms || !sPs || !stats_out || !lgssm->Fs.ptr || !lgssm->Qs.ptr || !lgssm->bs.ptr) {
        set_error("dims/lgssm(Fs,Qs,bs)/ys/ms/Ps/sms/sPs/stats_out must be non-NULL (cross_out may be NULL)");
        return AUXSSM_ERR_ARG;
    }
    if (int rc = em_check_sizes(dtype, dims->dx, dims->dy)) return rc;
    if (dims->C < 0 || dims->B < 1 || dims->T < 2) {
        set_error("need C >= 0 chains, B >= 1 and T >= 2 time steps, i.e. at least one transition (got C=%d, B=%d, T=%d)", dims->C, dims->B, dims->T);
        return AUXSSM_ERR_ARG;
    }
    if (lgssm->Fs.st != 0 || lgssm->Qs.st != 0 || lgssm->bs.st != 0) {
        set_error("the statistics are those of time-invariant dynamics: the time strides of Fs, Qs and bs must be 0");
        return AUXSSM_ERR_ARG;
    }
    const long long nseq = (long long)dims->C * dims->B;
    if (nseq * dt_num_segments(dims->T) > 0x7fffffffLL) {
        set_error("C x B x segments = %lld exceeds one launch (2^31 - 1 workgroups)", nseq * dt_num_segments(dims->T));
        return AUXSSM_ERR_ARG;
    }
    const int dx = dims->dx, dy = dims->dy, NS = em_ns(dx, dy);
    {  // no output may overlap an input (or the other output); ys is bounded by its largest stride
        const size_t rs = dtype == AUXSSM_F32 ? 4 : 8;
        const size_t nm = (size_t)nseq * dims->T * dx * rs, nP = nm * dx, nX = (size_t)nseq * (dims->T - 1) * dx * dx * rs, nS = (size_t)nseq * NS * sizeof(double);
        const size_t nY = ((size_t)(dims->C - 1) * (size_t)llabs(ys->sc) + (size_t)(dims->T - 1) * (size_t)llabs(ys->st) +
                           (size_t)(dims->B - 1) * (size_t)llabs(ys->sb) + dy) * rs;
        const void* in[5] = {ms, Ps, sms, sPs, ys->ptr};
        const size_t nin[5] = {nm, nP, nm, nP, nY};
        for (int k = 0; k < 5; ++k)
            if (em_overlap(stats_out, nS, in[k], nin[k]) || em_overlap(cross_out, nX, in[k], nin[k])) {
                set_error("stats_out / cross_out may not alias ys / ms / Ps / sms / sPs");
                return AUXSSM_ERR_ARG;
            }
        if (em_overlap(stats_out, nS, cross_out, nX)) {
            set_error("stats_out and cross_out may not alias each other");
            return AUXSSM_ERR_ARG;
        }
    }
    if (nseq == 0) return AUXSSM_OK;
    double* part;
    WsPlan ws;
    ws.add(part, (size_t)nseq * dt_num_segments(dims->T) * (em_dyn_packed(dx) + em_obs_packed(dx, dy)) * sizeof(double));
    if (int rc = ws.reserve(h)) return rc;
    em_by_d(dx, [&](auto d) {
        constexpr int D = decltype(d)::value;
        if (dtype == AUXSSM_F32) em_launch_stats<float, D>(h, dims, lgssm, ys, Ps, sms, sPs, cross_out, part, stats_out);
        else em_launch_stats<double, D>(h, dims, lgssm, ys, Ps, sms, sPs, cross_out, part, stats_out);
        return AUXSSM_OK;
    });
    AX_HIP(hipGetLastError());
    return AUXSSM_OK;
}

int auxssm_lgssm_em_mstep(auxssm_handle h, int dtype, int32_t dx, int32_t dy, int32_t nseq, const double* stats, const double* syy_nobs,
                          const auxssm_mniw_prior* prior, int update_mask, const auxssm_arr* F, const auxssm_arr* b, const auxssm_arr* Q, const auxssm_arr* H,
                          const auxssm_arr* c, const auxssm_arr* R, const auxssm_arr* m0, const auxssm_arr* P0, int32_t* flags) {
    AX_NEED_H(h);
    if (int rc = em_check_sizes(dtype, dx, dy)) return rc;
    const auxssm_arr* arrs[8] = {F, b, Q, H, c, R, m0, P0};
    if (!stats || !syy_nobs || !flags) {
        set_error("stats/syy_nobs/flags must be non-NULL (prior may be NULL)");
        return AUXSSM_ERR_ARG;
    }
    if (nseq < 1 || (update_mask & ~(EM_DYNAMICS | EM_OBSERVATIONS | EM_INITIAL))) {
        set_error("need nseq >= 1 and update_mask a combination of 1 (dynamics), 2 (observations), 4 (initial state) (got nseq=%d, mask=%d)", nseq, update_mask);
        return AUXSSM_ERR_ARG;
    }
    for (int k = 0; k < 8; ++k) {
        const bool wanted = (update_mask & (k < 3 ? EM_DYNAMICS : k < 6 ? EM_OBSERVATIONS : EM_INITIAL)) != 0;
        if (wanted && (!arrs[k] || !arrs[k]->ptr)) {
            set_error("the parameter arrays of every block in update_mask must be non-NULL (F, b, Q | H, c, R | m0, P0)");
            return AUXSSM_ERR_ARG;
        }
        if (wanted && k < 6 && arrs[k]->st != 0) {
            set_error("the M-step writes a time-invariant model: the time strides of F, b, Q, H, c, R must be 0");
            return AUXSSM_ERR_ARG;
        }
    }
    const auto ptr = [&](int k) { return arrs[k] ? const_cast<void*>(arrs[k]->ptr) : nullptr; };
    return em_by_d(dx, [&](auto d) -> int {
        constexpr int D = decltype(d)::value;
        DtPrior<D> pr{};
        if (prior && (update_mask & EM_DYNAMICS)) {
            if (int rc = em_prior<D>(prior, pr)) return rc;
        }
        em_by_dy(dy, [&](auto e) {
            constexpr int DY = decltype(e)::value;
            EmData<DY> dat;
            for (int k = 0; k < DY * DY; ++k) dat.Syy[k] = syy_nobs[k];
            dat.nobs = syy_nobs[DY * DY];
            if (dtype == AUXSSM_F32) {
                EmOut<float> o{(float*)ptr(0), (float*)ptr(1), (float*)ptr(2), (float*)ptr(3), (float*)ptr(4), (float*)ptr(5), (float*)ptr(6), (float*)ptr(7)};
                hipLaunchKernelGGL((k_em_mstep<float, D, DY>), dim3(1), dim3(64), 0, h->stream, nseq, stats, dat, prior ? 1 : 0, pr, update_mask, o, flags);
            } else {
                EmOut<double> o{(double*)ptr(0), (double*)ptr(1), (double*)ptr(2), (double*)ptr(3), (double*)ptr(4), (double*)ptr(5), (double*)ptr(6),
                                (double*)ptr(7)};
                hipLaunchKernelGGL((k_em_mstep<double, D, DY>), dim3(1), dim3(64), 0, h->stream, nseq, stats, dat, prior ? 1 : 0, pr, update_mask, o, flags);
            }
        });
        AX_HIP(hipGetLastError());
        return AUXSSM_OK;
    });
}

}  // extern "C"
