// dynamics_theta.hip -- theta | x for the linear-Gaussian dynamics every Kalman-sampler model shares: (F, b, Q) | x under a matrix-normal inverse-Wishart
// prior, one draw per chain, on the resident state (dense (C, T, dx) or chain-minor (T, dx, C)); and the gamma fill its chi-square variates come from.
// The arithmetic is dynamics_theta.h (also compiled by g++ for tests/hostsim_dynamics_theta).  Three launches per update:
//   1. statistics   grid (time segment, chain) [dense: 256 lanes over the segment's transitions] or (time segment, block of 64 chains) [chain-minor: lanes over
//                   chains, 4 interleaved time slices]: the packed sums (45 at d = 4) in registers, products and sums in double, one partial per (chain, segment)
//                   written to the workspace.  No atomics; the segment length depends on T alone (dt_segment_len), so a chain's sums do not depend on its batch.
//   2. reduce       one lane per (chain, packed sum): the partials added in ascending segment order, written as FULL statistics (C, .)
//   3. finish       one lane per chain: posterior, draw, F / b / Q rounded to the model's dtype through their auxssm_arr descriptors; a failed factorisation
//                   leaves the chain's parameters as they are and raises flags[c].
// Built with -ffp-contract=off (as loop.hip): the sums are then the restatement's expressions.
#include "ctx.h"
#include "dynamics_theta.h"

namespace ax {

// block-wide sum of the lanes' packed statistics in a fixed order: butterfly-free shuffle tree inside each wave, then the waves in ascending order
template <int P> __device__ __forceinline__ void dt_block_sum(double* acc, double* sh /*[waves][P]*/, int nwaves) {
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

template <typename R, int D>
__global__ void __launch_bounds__(DT_THREADS) k_dt_stats_dense(int T, int L, int nseg, const R* __restrict__ x, double* __restrict__ part) {
    constexpr int P = DtDims<D>::PACKED;
    __shared__ double sh[(DT_THREADS / 64) * P];
    const long long blk = blockIdx.x;
    const int c = (int)(blk / nseg), seg = (int)(blk - (long long)c * nseg);
    const int t0 = seg * L, t1 = min(t0 + L, T - 1);
    const R* xc = x + (long long)c * T * D;
    double acc[P];
#pragma unroll
    for (int k = 0; k < P; ++k) acc[k] = 0.0;
    for (int t = t0 + (int)threadIdx.x; t < t1; t += DT_THREADS) {
        double xt[D], xn[D];
#pragma unroll
        for (int k = 0; k < D; ++k) xt[k] = (double)xc[(long long)t * D + k], xn[k] = (double)xc[(long long)(t + 1) * D + k];
        dt_accumulate<D>(xt, xn, acc);
    }
    dt_block_sum<P>(acc, sh, DT_THREADS / 64);
    if (threadIdx.x < P) {
        double s = sh[threadIdx.x];
#pragma unroll
        for (int w = 1; w < DT_THREADS / 64; ++w) s += sh[w * P + threadIdx.x];
        part[blk * P + threadIdx.x] = s;
    }
}

// chain-minor: lane <-> chain (loads of consecutive lanes are consecutive addresses), threadIdx.y = one of DT_CM_SLICES interleaved time slices of the segment;
// the slices are added in ascending order through LDS
template <typename R, int D>
__global__ void __launch_bounds__(DT_CM_LANES* DT_CM_SLICES) k_dt_stats_cm(int C, int T, int L, int nseg, const R* __restrict__ x, double* __restrict__ part) {
    constexpr int P = DtDims<D>::PACKED;
    __shared__ double sh[P * DT_CM_LANES];
    const int seg = blockIdx.x, lane = threadIdx.x, sl = threadIdx.y;
    const int c = blockIdx.y * DT_CM_LANES + lane;
    const bool live = c < C;
    const int t0 = seg * L, t1 = min(t0 + L, T - 1);
    double acc[P];
#pragma unroll
    for (int k = 0; k < P; ++k) acc[k] = 0.0;
    if (live)
        for (int t = t0 + sl; t < t1; t += DT_CM_SLICES) {
            double xt[D], xn[D];
#pragma unroll
            for (int k = 0; k < D; ++k) {
                xt[k] = (double)x[((long long)t * D + k) * C + c];
                xn[k] = (double)x[((long long)(t + 1) * D + k) * C + c];
            }
            dt_accumulate<D>(xt, xn, acc);
        }
    for (int s = 1; s < DT_CM_SLICES; ++s) {
        if (sl == s) {
#pragma unroll
            for (int k = 0; k < P; ++k) sh[k * DT_CM_LANES + lane] = acc[k];
        }
        __syncthreads();
        if (sl == 0) {
#pragma unroll
            for (int k = 0; k < P; ++k) acc[k] += sh[k * DT_CM_LANES + lane];
        }
        __syncthreads();
    }
    if (sl == 0 && live) {
        double* pc = part + ((long long)c * nseg + seg) * P;
#pragma unroll
        for (int k = 0; k < P; ++k) pc[k] = acc[k];
    }
}

// one lane per (chain, packed sum): ascending segments; the sum goes to its one or two places of the FULL layout
template <int D> __global__ void __launch_bounds__(256) k_dt_reduce(long long C, int nseg, const double* __restrict__ part, double* __restrict__ full) {
    using S = DtDims<D>;
    constexpr int P = S::PACKED, n = S::n;
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= C * P) return;
    const long long c = g / P;
    const int k = (int)(g - c * P);
    double s = 0.0;
    for (int seg = 0; seg < nseg; ++seg) s += part[(c * nseg + seg) * P + k];
    double* f = full + c * S::FULL;
    if (k < S::ZZ) {
        int i = 0;
        while (dt_tri(i + 1, 0) <= k) ++i;
        const int j = k - dt_tri(i, 0);
        f[i * n + j] = s;
        f[j * n + i] = s;
    } else if (k < S::ZZ + S::XZ) {
        f[n * n + (k - S::ZZ)] = s;
    } else {
        const int kk = k - S::ZZ - S::XZ;
        int i = 0;
        while (dt_tri(i + 1, 0) <= kk) ++i;
        const int j = kk - dt_tri(i, 0);
        f[n * n + S::XZ + i * D + j] = s;
        f[n * n + S::XZ + j * D + i] = s;
    }
}

template <typename R, int D>
__global__ void __launch_bounds__(64) k_dt_finish(int C, int ntrans, DtPrior<D> pr, const double* __restrict__ full, const R* __restrict__ chi,
                                                  const R* __restrict__ ew, const R* __restrict__ ea, R* __restrict__ F, long long sF, R* __restrict__ b,
                                                  long long sb, R* __restrict__ Q, long long sQ, double* __restrict__ post_out, int32_t* __restrict__ flags) {
    using S = DtDims<D>;
    constexpr int n = S::n;
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= C) return;
    double st[S::FULL], post[S::POST], U[n * n], L[D * D];
    for (int k = 0; k < S::FULL; ++k) st[k] = full[(long long)c * S::FULL + k];
    int flag = dt_posterior<D>(st, ntrans, pr, post, U, L);
    if (post_out)
        for (int k = 0; k < S::POST; ++k) post_out[(long long)c * S::POST + k] = post[k];
    if (flag == DT_OK) {
        double ch[D], w[D * D], e[D * n], Qd[D * D], A[D * n];
        for (int k = 0; k < D; ++k) ch[k] = (double)chi[(long long)c * D + k];
        for (int k = 0; k < D * D; ++k) w[k] = (double)ew[(long long)c * D * D + k];
        for (int k = 0; k < D * n; ++k) e[k] = (double)ea[(long long)c * D * n + k];
        flag = dt_draw<D>(post, U, L, pr.chi_scale, ch, w, e, Qd, A);
        if (flag == DT_OK) {
            // (rounding to R may overflow a finite double: then nothing of this chain is written either)
            bool fin = true;
            for (int k = 0; k < D * n; ++k) fin = fin && finite_((R)A[k]);
            for (int k = 0; k < D * D; ++k) fin = fin && finite_((R)Qd[k]);
            if (!fin) flag = DT_FAIL_Q;
        }
        if (flag == DT_OK) {
            for (int i = 0; i < D; ++i) {
                for (int j = 0; j < D; ++j) {
                    F[(long long)c * sF + i * D + j] = (R)A[i * n + j];
                    Q[(long long)c * sQ + i * D + j] = (R)Qd[i * D + j];
                }
                b[(long long)c * sb + i] = (R)A[i * n + D];
            }
        }
    }
    flags[c] = flag;
}

struct DtGammaArgs {
    DtGammaShape s[8];
};
template <typename R>
__global__ void __launch_bounds__(256) k_dt_gamma(uint32_t k0, uint32_t k1, uint32_t stream, long long total, int m, DtGammaArgs a, R* __restrict__ out) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= total) return;
    out[g] = (R)dt_gamma_draw(k0, k1, stream, (unsigned long long)g, a.s[(int)(g % m)]);
}

template <typename F> static int dt_by_d(int dx, F&& f) {
    switch (dx) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        default: return f(std::integral_constant<int, 4>{});
    }
}

// what the two entry points share: the arguments that describe the resident state
static int dt_check_state(int dtype, int32_t C, int32_t T, int32_t dx, int layout, const void* x) {
    if (int rc = check_dtype(dtype)) return rc;
    if (dx < 1 || dx > DT_MAX_D) {
        set_error("the dynamics step covers 1 <= dx <= %d (got dx=%d)", DT_MAX_D, dx);
        return AUXSSM_ERR_UNSUPPORTED;
    }
    if (C < 0 || T < 2) {
        set_error("need C >= 0 chains and T >= 2 time steps, i.e. at least one transition (got C=%d, T=%d)", C, T);
        return AUXSSM_ERR_ARG;
    }
    if (layout != AUXSSM_LAYOUT_DENSE && layout != AUXSSM_LAYOUT_CHAIN_MINOR) {
        set_error("layout must be AUXSSM_LAYOUT_DENSE (0) or AUXSSM_LAYOUT_CHAIN_MINOR (1)");
        return AUXSSM_ERR_ARG;
    }
    if (!x) {
        set_error("x must be non-NULL");
        return AUXSSM_ERR_ARG;
    }
    if ((long long)C * dt_num_segments(T) > 0x7fffffffLL) {
        set_error("C x segments = %lld exceeds one launch (2^31 - 1 workgroups)", (long long)C * dt_num_segments(T));
        return AUXSSM_ERR_ARG;
    }
    if (layout == AUXSSM_LAYOUT_CHAIN_MINOR && (C + DT_CM_LANES - 1) / DT_CM_LANES > 65535) {
        set_error("the chain-minor statistics pass takes at most 65535 blocks of %d chains, C <= %d (got C=%d)", DT_CM_LANES, 65535 * DT_CM_LANES, C);
        return AUXSSM_ERR_ARG;
    }
    return AUXSSM_OK;
}

// launches 1 and 2: x -> full (C, FULL); part is the workspace of C x segments x PACKED doubles
template <typename R, int D> static void dt_launch_stats(auxssm_ctx* h, int C, int T, int layout, const void* x, double* part, double* full) {
    constexpr int P = DtDims<D>::PACKED;
    const int L = dt_segment_len(T), nseg = dt_num_segments(T);
    if (layout == AUXSSM_LAYOUT_CHAIN_MINOR)
        hipLaunchKernelGGL((k_dt_stats_cm<R, D>), dim3((unsigned)nseg, (unsigned)((C + DT_CM_LANES - 1) / DT_CM_LANES)), dim3(DT_CM_LANES, DT_CM_SLICES), 0,
                           h->stream, C, T, L, nseg, (const R*)x, part);
    else
        hipLaunchKernelGGL((k_dt_stats_dense<R, D>), dim3((unsigned)((long long)C * nseg)), dim3(DT_THREADS), 0, h->stream, T, L, nseg, (const R*)x, part);
    const long long work = (long long)C * P;
    hipLaunchKernelGGL((k_dt_reduce<D>), dim3((unsigned)((work + 255) / 256)), dim3(256), 0, h->stream, (long long)C, nseg, (const double*)part, full);
}
static size_t dt_part_bytes(int C, int T, int dx) {
    const int n = dx + 1, P = n * (n + 1) / 2 + dx * n + dx * (dx + 1) / 2;
    return (size_t)C * dt_num_segments(T) * P * sizeof(double);
}

static bool dt_all_finite(const double* a, int k) {
    for (int i = 0; i < k; ++i)
        if (!std::isfinite(a[i])) return false;
    return true;
}
static bool dt_symmetric(const double* a, int n) {
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < i; ++j)
            if (!(fabs(a[i * n + j] - a[j * n + i]) <= 1e-12 * (fabs(a[i * n + i]) + fabs(a[j * n + j])))) return false;
    return true;
}
// the caller's prior -> the kernels' (its symmetric parts symmetrised), or a message
template <int D> static int dt_prior(const auxssm_mniw_prior* p, DtPrior<D>& pr) {
    constexpr int n = D + 1;
    if (!dt_all_finite(p->M0, D * n) || !dt_all_finite(p->K0, n * n) || !dt_all_finite(p->Psi0, D * D) || !std::isfinite(p->nu0) ||
        !std::isfinite(p->chi_scale)) {
        set_error("the prior has a non-finite entry (M0 (%d, %d), K0 (%d, %d), nu0, Psi0 (%d, %d), chi_scale)", D, n, n, n, D, D);
        return AUXSSM_ERR_ARG;
    }
    if (!(p->nu0 > (double)(D - 1))) {
        set_error("the prior needs nu0 > dx - 1 = %d (got %g)", D - 1, p->nu0);
        return AUXSSM_ERR_ARG;
    }
    if (!(p->chi_scale > 0.0)) {
        set_error("chi_scale must be positive (1: chi holds chi-square draws, 2: Gamma(shape / 2, 1) draws), got %g", p->chi_scale);
        return AUXSSM_ERR_ARG;
    }
    if (!dt_symmetric(p->K0, n) || !dt_symmetric(p->Psi0, D)) {
        set_error("K0 (%d, %d) and Psi0 (%d, %d) must be symmetric", n, n, D, D);
        return AUXSSM_ERR_ARG;
    }
    for (int k = 0; k < D * n; ++k) pr.M0[k] = p->M0[k];
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) pr.K0[i * n + j] = 0.5 * (p->K0[i * n + j] + p->K0[j * n + i]);
    for (int i = 0; i < D; ++i)
        for (int j = 0; j < D; ++j) pr.Psi0[i * D + j] = 0.5 * (p->Psi0[i * D + j] + p->Psi0[j * D + i]);
    pr.nu0 = p->nu0;
    pr.chi_scale = p->chi_scale;
    double l[n * n];
    if (!dt_chol<n>(pr.K0, l) || !dt_chol<D>(pr.Psi0, l)) {
        set_error("K0 (%d, %d) and Psi0 (%d, %d) must be positive definite", n, n, D, D);
        return AUXSSM_ERR_ARG;
    }
    return AUXSSM_OK;
}

}  // namespace ax

using namespace ax;

extern "C" {

int auxssm_dynamics_stats(auxssm_handle h, int dtype, int32_t C, int32_t T, int32_t dx, int layout, const void* x, double* stats_out) {
    AX_NEED_H(h);
    if (int rc = dt_check_state(dtype, C, T, dx, layout, x)) return rc;
    if (!stats_out) {
        set_error("stats_out must be non-NULL");
        return AUXSSM_ERR_ARG;
    }
    if (C == 0) return AUXSSM_OK;
    double* part;
    WsPlan ws;
    ws.add(part, dt_part_bytes(C, T, dx));
    if (int rc = ws.reserve(h)) return rc;
    dt_by_d(dx, [&](auto d) {
        constexpr int D = decltype(d)::value;
        if (dtype == AUXSSM_F32) dt_launch_stats<float, D>(h, C, T, layout, x, part, stats_out);
        else dt_launch_stats<double, D>(h, C, T, layout, x, part, stats_out);
        return AUXSSM_OK;
    });
    AX_HIP(hipGetLastError());
    return AUXSSM_OK;
}

int auxssm_dynamics_theta_update(auxssm_handle h, int dtype, int32_t C, int32_t T, int32_t dx, int layout, const void* x, const auxssm_mniw_prior* prior,
                                 const void* chi, const void* eps_w, const void* eps_a, const auxssm_arr* F, const auxssm_arr* b, const auxssm_arr* Q,
                                 double* post_out, int32_t* flags) {
    AX_NEED_H(h);
    if (int rc = dt_check_state(dtype, C, T, dx, layout, x)) return rc;
    if (!prior || !chi || !eps_w || !eps_a || !F || !b || !Q || !flags || !F->ptr || !b->ptr || !Q->ptr) {
        set_error("prior/chi/eps_w/eps_a/F/b/Q/flags must be non-NULL (post_out may be NULL)");
        return AUXSSM_ERR_ARG;
    }
    if (F->st != 0 || b->st != 0 || Q->st != 0) {
        set_error("the step writes time-invariant dynamics: the time strides of F, b and Q must be 0");
        return AUXSSM_ERR_ARG;
    }
    if (C > 1 && (F->sc < (int64_t)dx * dx || Q->sc < (int64_t)dx * dx || b->sc < dx)) {
        set_error("with C > 1 every chain needs its own F, b, Q: chain strides >= dx*dx, dx, dx*dx elements (got %lld, %lld, %lld)", (long long)F->sc,
                  (long long)b->sc, (long long)Q->sc);
        return AUXSSM_ERR_ARG;
    }
    return dt_by_d(dx, [&](auto d) -> int {
        constexpr int D = decltype(d)::value;
        DtPrior<D> pr;
        if (int rc = dt_prior<D>(prior, pr)) return rc;
        if (C == 0) return AUXSSM_OK;
        double *part, *full;
        WsPlan ws;
        ws.add(part, dt_part_bytes(C, T, dx));
        ws.add(full, (size_t)C * DtDims<D>::FULL * sizeof(double));
        if (int rc = ws.reserve(h)) return rc;
        const unsigned grid = (unsigned)((C + 63) / 64);
        if (dtype == AUXSSM_F32) {
            dt_launch_stats<float, D>(h, C, T, layout, x, part, full);
            hipLaunchKernelGGL((k_dt_finish<float, D>), dim3(grid), dim3(64), 0, h->stream, C, T - 1, pr, (const double*)full, (const float*)chi,
                               (const float*)eps_w, (const float*)eps_a, (float*)F->ptr, (long long)F->sc, (float*)b->ptr, (long long)b->sc, (float*)Q->ptr,
                               (long long)Q->sc, post_out, flags);
        } else {
            dt_launch_stats<double, D>(h, C, T, layout, x, part, full);
            hipLaunchKernelGGL((k_dt_finish<double, D>), dim3(grid), dim3(64), 0, h->stream, C, T - 1, pr, (const double*)full, (const double*)chi,
                               (const double*)eps_w, (const double*)eps_a, (double*)F->ptr, (long long)F->sc, (double*)b->ptr, (long long)b->sc,
                               (double*)Q->ptr, (long long)Q->sc, post_out, flags);
        }
        AX_HIP(hipGetLastError());
        return AUXSSM_OK;
    });
}

int auxssm_rng_gamma(auxssm_handle h, int dtype, uint32_t key0, uint32_t key1, uint32_t stream, int64_t n, int32_t m, const double* shapes, void* out) {
    AX_NEED_H(h);
    if (int rc = check_dtype(dtype)) return rc;
    if (n < 0 || m < 1 || m > 8 || !shapes || !out) {
        set_error("need n >= 0 rows, 1 <= m <= 8 shapes per row, shapes (host) and out non-NULL (got n=%lld, m=%d)", (long long)n, m);
        return AUXSSM_ERR_ARG;
    }
    DtGammaArgs a{};
    for (int i = 0; i < m; ++i) {
        if (!(shapes[i] > 0.0) || !std::isfinite(shapes[i])) {
            set_error("shapes[%d] = %g: a gamma shape must be positive and finite", i, shapes[i]);
            return AUXSSM_ERR_ARG;
        }
        a.s[i] = dt_gamma_shape(shapes[i]);
    }
    const long long total = (long long)n * m;
    // (a draw owns 2 x DT_GAMMA_ATTEMPTS blocks of the stream, whose block index has 48 bits: rng.h::stream_counter)
    if (total > (1LL << 42) || (total + 255) / 256 > 0x7fffffffLL) {
        set_error("n x m = %lld draws exceed one stream (2^42)", total);
        return AUXSSM_ERR_ARG;
    }
    if (total == 0) return AUXSSM_OK;
    ProfScope ps(h, AUXSSM_K_RNG);
    const unsigned grid = (unsigned)((total + 255) / 256);
    if (dtype == AUXSSM_F32) hipLaunchKernelGGL((k_dt_gamma<float>), dim3(grid), dim3(256), 0, h->stream, key0, key1, stream, total, m, a, (float*)out);
    else hipLaunchKernelGGL((k_dt_gamma<double>), dim3(grid), dim3(256), 0, h->stream, key0, key1, stream, total, m, a, (double*)out);
    AX_HIP(hipGetLastError());
    return AUXSSM_OK;
}

}  // extern "C"
