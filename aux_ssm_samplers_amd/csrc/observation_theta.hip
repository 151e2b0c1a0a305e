// observation_theta.hip -- theta | x, y for the linear-Gaussian observation model y_t = H x_t + c + N(0, R) of an LG_CONCAT model: (H, c, R) | x, y under a
// matrix-normal inverse-Wishart prior (or R alone, H and c fixed), one draw per chain, on the resident state (dense (C, T, dx) or chain-minor (T, dx, C)) and the
// data yobs (T, dy) the chains share.  The arithmetic is observation_theta.h (also compiled by g++ for tests/hostsim_observation_theta).  Three launches per update:
//   1. statistics   grid (chain x time segment) [dense: 256 lanes over the segment's steps] or (time segment, block of 64 chains) [chain-minor: lanes over
//                   chains, 4 interleaved time slices, y_t read once per wave by a uniform load]: the packed sums (35 at dx = dy = 4) in registers, products and
//                   sums in double, a row of y with a non-finite entry skipped whole, one partial per (chain, segment) written to the workspace.  No atomics; the
//                   segment length depends on T alone (dt_segment_len), so a chain's sums do not depend on its batch.
//   2. reduce       one lane per (chain, packed sum): the partials added in ascending segment order, written as FULL statistics (C, .)
//   3. finish       one lane per chain, its matrices in LDS: posterior, draw, H / c / R rounded to the model's dtype through their auxssm_arr descriptors; a failed
//                   factorisation leaves the chain's parameters as they are and raises flags[c].
// Built with -ffp-contract=off (as dynamics_theta.hip): the sums are then the restatement's expressions.
#include "ctx.h"
#include "observation_theta.h"

namespace ax {

template <typename R, int DX, int DY>
__global__ void __launch_bounds__(DT_THREADS) k_ot_stats_dense(int T, int L, int nseg, const R* __restrict__ x, const R* __restrict__ y, long long yst,
                                                               double* __restrict__ part) {
    constexpr int P = OtDims<DX, DY>::PACKED;
    __shared__ double sh[(DT_THREADS / 64) * P];
    const long long blk = blockIdx.x;
    const int c = (int)(blk / nseg), seg = (int)(blk - (long long)c * nseg);
    const int t0 = seg * L, t1 = min(t0 + L, T);
    const R* xc = x + (long long)c * T * DX;
    double acc[P];
#pragma unroll
    for (int k = 0; k < P; ++k) acc[k] = 0.0;
    for (int t = t0 + (int)threadIdx.x; t < t1; t += DT_THREADS) {
        // (both loads are issued before the row is judged: the state's load does not wait for y)
        double xt[DX], yt[DY];
#pragma unroll
        for (int k = 0; k < DY; ++k) yt[k] = (double)y[(long long)t * yst + k];
#pragma unroll
        for (int k = 0; k < DX; ++k) xt[k] = (double)xc[(long long)t * DX + k];
        if (ot_row_observed<DY>(yt)) ot_accumulate<DX, DY>(xt, yt, acc);
    }
    // block-wide sum in a fixed order: a shuffle tree inside each wave, then the waves in ascending order
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
    if (threadIdx.x < P) {
        double s = sh[threadIdx.x];
#pragma unroll
        for (int w = 1; w < DT_THREADS / 64; ++w) s += sh[w * P + threadIdx.x];
        part[blk * P + threadIdx.x] = s;
    }
}

// chain-minor: lane <-> chain (loads of consecutive lanes are consecutive addresses), threadIdx.y = the wave = one of DT_CM_SLICES interleaved time slices of the
// segment.  y_t is the same for the 64 chains of a wave: its address is wave-uniform (the slice index goes through readfirstlane), one load per wave and step.
// The slices are added in ascending order through LDS.
template <typename R, int DX, int DY>
__global__ void __launch_bounds__(DT_CM_LANES* DT_CM_SLICES)
    k_ot_stats_cm(int C, int T, int L, int nseg, const R* __restrict__ x, const R* __restrict__ y, long long yst, double* __restrict__ part) {
    constexpr int P = OtDims<DX, DY>::PACKED;
    __shared__ double sh[P * DT_CM_LANES];
    const int seg = blockIdx.x, lane = threadIdx.x;
    const int sl = __builtin_amdgcn_readfirstlane((int)threadIdx.y);
    const int c = blockIdx.y * DT_CM_LANES + lane;
    const bool live = c < C;
    const int t0 = seg * L, t1 = min(t0 + L, T);
    double acc[P];
#pragma unroll
    for (int k = 0; k < P; ++k) acc[k] = 0.0;
    if (live)
        for (int t = t0 + sl; t < t1; t += DT_CM_SLICES) {
            // (both loads are issued before the row is judged: the state's load does not wait for y; the whole wave takes the same branch)
            double xt[DX], yt[DY];
#pragma unroll
            for (int k = 0; k < DY; ++k) yt[k] = (double)y[(long long)t * yst + k];
#pragma unroll
            for (int k = 0; k < DX; ++k) xt[k] = (double)x[((long long)t * DX + k) * C + c];
            if (ot_row_observed<DY>(yt)) ot_accumulate<DX, DY>(xt, yt, acc);
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
template <int DX, int DY> __global__ void __launch_bounds__(256) k_ot_reduce(long long C, int nseg, const double* __restrict__ part, double* __restrict__ full) {
    using S = OtDims<DX, DY>;
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
    } else {
        f[n * n + (k - S::ZZ)] = s;
    }
}

// what the finish kernel takes by value: the prior (its blocks packed to the model's sizes) and the data-only terms
template <int DX, int DY> struct OtArgs {
    double M0[DY * (DX + 1)], K0[(DX + 1) * (DX + 1)], Psi0[DY * DY], Syy[DY * DY], nu0, chi_scale, nobs;
};

// one lane per chain, OT_FIN_LANES chains per workgroup.  Each lane's matrices live in LDS (W doubles per lane), the prior once per workgroup: the loops of
// observation_theta.h then index memory, not registers or scratch.
template <typename R, int DX, int DY>
__global__ void __launch_bounds__(OT_FIN_LANES)
    k_ot_finish(int C, int mode, OtArgs<DX, DY> a, const double* __restrict__ full, const R* __restrict__ chi, const R* __restrict__ ew, const R* __restrict__ ea,
                R* __restrict__ H, long long sH, R* __restrict__ cv_, long long sc, R* __restrict__ Rm_, long long sR, double* __restrict__ post_out,
                int32_t* __restrict__ flags) {
    using S = OtDims<DX, DY>;
    constexpr int n = S::n, YZ = S::YZ, YY = DY * DY;
    constexpr int O_ST = 0, O_POST = O_ST + S::FULL, O_U = O_POST + S::POST, O_L = O_U + n * n, O_WORK = O_L + YY, O_CHI = O_WORK + S::WORK, O_EW = O_CHI + DY,
                  O_EA = O_EW + YY, O_R = O_EA + YZ, O_A = O_R + YY, W = O_A + YZ;
    __shared__ double sh[OT_FIN_LANES * W];
    __shared__ double pM0[YZ], pK0[n * n], pPsi0[YY], pSyy[YY];
    if (threadIdx.x == 0) {
        for (int k = 0; k < YZ; ++k) pM0[k] = a.M0[k];
        for (int k = 0; k < n * n; ++k) pK0[k] = a.K0[k];
        for (int k = 0; k < YY; ++k) pPsi0[k] = a.Psi0[k], pSyy[k] = a.Syy[k];
    }
    __syncthreads();
    const int c = blockIdx.x * OT_FIN_LANES + threadIdx.x;
    if (c >= C) return;
    double* my = sh + threadIdx.x * W;
    double *st = my + O_ST, *post = my + O_POST, *U = my + O_U, *L = my + O_L, *work = my + O_WORK, *ch = my + O_CHI, *w = my + O_EW, *e = my + O_EA,
           *Rd = my + O_R, *A = my + O_A;
    const bool joint = mode == OT_JOINT;
    for (int k = 0; k < S::FULL; ++k) st[k] = full[(long long)c * S::FULL + k];
    int flag;
    if (joint) {
        flag = ot_posterior_joint<DX, DY>(st, pSyy, a.nobs, pM0, pK0, pPsi0, a.nu0, post, U, L, work);
    } else {
        for (int i = 0; i < DY; ++i) {
            for (int j = 0; j < DX; ++j) A[i * n + j] = (double)H[(long long)c * sH + i * DX + j];
            A[i * n + DX] = (double)cv_[(long long)c * sc + i];
        }
        flag = ot_posterior_r<DX, DY>(st, pSyy, a.nobs, pPsi0, a.nu0, A, post, L, work);
    }
    if (post_out)
        for (int k = 0; k < S::POST; ++k) post_out[(long long)c * S::POST + k] = post[k];
    if (flag == DT_OK) {
        for (int k = 0; k < DY; ++k) ch[k] = (double)chi[(long long)c * DY + k];
        for (int k = 0; k < YY; ++k) w[k] = (double)ew[(long long)c * YY + k];
        if (joint)
            for (int k = 0; k < YZ; ++k) e[k] = (double)ea[(long long)c * YZ + k];
        flag = ot_draw<DX, DY>(joint, post, U, L, a.chi_scale, ch, w, e, Rd, A, work);
        if (flag == DT_OK) {
            // (rounding to R may overflow a finite double: then nothing of this chain is written either)
            bool fin = true;
            if (joint)
                for (int k = 0; k < YZ; ++k) fin = fin && finite_((R)A[k]);
            for (int k = 0; k < YY; ++k) fin = fin && finite_((R)Rd[k]);
            if (!fin) flag = DT_FAIL_Q;
        }
        if (flag == DT_OK) {
            for (int i = 0; i < DY; ++i) {
                if (joint) {
                    for (int j = 0; j < DX; ++j) H[(long long)c * sH + i * DX + j] = (R)A[i * n + j];
                    cv_[(long long)c * sc + i] = (R)A[i * n + DX];
                }
                for (int j = 0; j < DY; ++j) Rm_[(long long)c * sR + i * DY + j] = (R)Rd[i * DY + j];
            }
        }
    }
    flags[c] = flag;
}

template <typename F> static int ot_by_d(int d, F&& f) {
    switch (d) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        default: return f(std::integral_constant<int, 4>{});
    }
}
template <typename F> static int ot_by_dims(int dx, int dy, F&& f) {
    return ot_by_d(dx, [&](auto a) { return ot_by_d(dy, [&](auto b) { return f(a, b); }); });
}

// what the two entry points share: the arguments that describe the resident state and the data
static int ot_check_state(int dtype, int32_t C, int32_t T, int32_t dx, int32_t dy, int layout, const void* x, const auxssm_arr* yobs) {
    if (int rc = check_dtype(dtype)) return rc;
    if (dx < 1 || dx > OT_MAX_D || dy < 1 || dy > OT_MAX_D) {
        set_error("the observation step covers 1 <= dx <= %d and 1 <= dy <= %d (got dx=%d, dy=%d)", OT_MAX_D, OT_MAX_D, dx, dy);
        return AUXSSM_ERR_UNSUPPORTED;
    }
    if (C < 0 || T < 2) {
        set_error("need C >= 0 chains and T >= 2 time steps (got C=%d, T=%d)", C, T);
        return AUXSSM_ERR_ARG;
    }
    if (layout != AUXSSM_LAYOUT_DENSE && layout != AUXSSM_LAYOUT_CHAIN_MINOR) {
        set_error("layout must be AUXSSM_LAYOUT_DENSE (0) or AUXSSM_LAYOUT_CHAIN_MINOR (1)");
        return AUXSSM_ERR_ARG;
    }
    if (!x || !yobs || !yobs->ptr) {
        set_error("x, yobs and yobs->ptr must be non-NULL");
        return AUXSSM_ERR_ARG;
    }
    if (yobs->sc != 0) {
        set_error("yobs (T, dy) is shared by the chains: its chain stride must be 0 (got %lld)", (long long)yobs->sc);
        return AUXSSM_ERR_ARG;
    }
    if (yobs->st < dy) {
        set_error("the rows of yobs (T, dy) must not overlap: time stride >= dy = %d elements (got %lld)", dy, (long long)yobs->st);
        return AUXSSM_ERR_ARG;
    }
    if ((long long)C * ot_num_segments(T) > 0x7fffffffLL) {
        set_error("C x segments = %lld exceeds one launch (2^31 - 1 workgroups)", (long long)C * ot_num_segments(T));
        return AUXSSM_ERR_ARG;
    }
    if (layout == AUXSSM_LAYOUT_CHAIN_MINOR && (C + DT_CM_LANES - 1) / DT_CM_LANES > 65535) {
        set_error("the chain-minor statistics pass takes at most 65535 blocks of %d chains, C <= %d (got C=%d)", DT_CM_LANES, 65535 * DT_CM_LANES, C);
        return AUXSSM_ERR_ARG;
    }
    return AUXSSM_OK;
}

// launches 1 and 2: (x, y) -> full (C, FULL); part is the workspace of C x segments x PACKED doubles
template <typename R, int DX, int DY>
static void ot_launch_stats(auxssm_ctx* h, int C, int T, int layout, const void* x, const auxssm_arr* yobs, double* part, double* full) {
    constexpr int P = OtDims<DX, DY>::PACKED;
    const int L = dt_segment_len(T), nseg = ot_num_segments(T);
    if (layout == AUXSSM_LAYOUT_CHAIN_MINOR)
        hipLaunchKernelGGL((k_ot_stats_cm<R, DX, DY>), dim3((unsigned)nseg, (unsigned)((C + DT_CM_LANES - 1) / DT_CM_LANES)), dim3(DT_CM_LANES, DT_CM_SLICES), 0,
                           h->stream, C, T, L, nseg, (const R*)x, (const R*)yobs->ptr, (long long)yobs->st, part);
    else
        hipLaunchKernelGGL((k_ot_stats_dense<R, DX, DY>), dim3((unsigned)((long long)C * nseg)), dim3(DT_THREADS), 0, h->stream, T, L, nseg, (const R*)x,
                           (const R*)yobs->ptr, (long long)yobs->st, part);
    const long long work = (long long)C * P;
    hipLaunchKernelGGL((k_ot_reduce<DX, DY>), dim3((unsigned)((work + 255) / 256)), dim3(256), 0, h->stream, (long long)C, nseg, (const double*)part, full);
}
static size_t ot_part_bytes(int C, int T, int dx, int dy) {
    const int n = dx + 1, P = n * (n + 1) / 2 + dy * n;
    return (size_t)C * ot_num_segments(T) * P * sizeof(double);
}

static bool ot_all_finite(const double* a, int k) {
    for (int i = 0; i < k; ++i)
        if (!std::isfinite(a[i])) return false;
    return true;
}
static bool ot_symmetric(const double* a, int n) {
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < i; ++j)
            if (!(fabs(a[i * n + j] - a[j * n + i]) <= 1e-12 * (fabs(a[i * n + i]) + fabs(a[j * n + j])))) return false;
    return true;
}
// the caller's prior and data terms -> the kernel's (symmetric parts symmetrised), or a message; R alone: M0 and K0 are neither checked nor read
template <int DX, int DY> static int ot_args(const auxssm_mniw_prior* p, const double* syy_nobs, bool joint, OtArgs<DX, DY>& a) {
    constexpr int n = DX + 1;
    a = OtArgs<DX, DY>{};
    if (!ot_all_finite(p->Psi0, DY * DY) || !std::isfinite(p->nu0) || !std::isfinite(p->chi_scale) ||
        (joint && (!ot_all_finite(p->M0, DY * n) || !ot_all_finite(p->K0, n * n)))) {
        set_error("the prior has a non-finite entry (M0 (%d, %d), K0 (%d, %d), nu0, Psi0 (%d, %d), chi_scale)", DY, n, n, n, DY, DY);
        return AUXSSM_ERR_ARG;
    }
    if (!(p->nu0 > (double)(DY - 1))) {
        set_error("the prior needs nu0 > dy - 1 = %d (got %g)", DY - 1, p->nu0);
        return AUXSSM_ERR_ARG;
    }
    if (!(p->chi_scale > 0.0)) {
        set_error("chi_scale must be positive (1: chi holds chi-square draws, 2: Gamma(shape / 2, 1) draws), got %g", p->chi_scale);
        return AUXSSM_ERR_ARG;
    }
    if (!ot_symmetric(p->Psi0, DY) || (joint && !ot_symmetric(p->K0, n))) {
        set_error("K0 (%d, %d) and Psi0 (%d, %d) must be symmetric", n, n, DY, DY);
        return AUXSSM_ERR_ARG;
    }
    if (!ot_all_finite(syy_nobs, DY * DY + 1) || !(syy_nobs[DY * DY] >= 0.0)) {
        set_error("syy_nobs (%d host doubles: S_yy (%d, %d), n_obs) must be finite with n_obs >= 0", DY * DY + 1, DY, DY);
        return AUXSSM_ERR_ARG;
    }
    double l[n * n > DY * DY ? n * n : DY * DY];
    for (int i = 0; i < DY; ++i)
        for (int j = 0; j < DY; ++j) {
            a.Psi0[i * DY + j] = 0.5 * (p->Psi0[i * DY + j] + p->Psi0[j * DY + i]);
            a.Syy[i * DY + j] = 0.5 * (syy_nobs[i * DY + j] + syy_nobs[j * DY + i]);
        }
    bool pd = dt_chol<DY>(a.Psi0, l);
    if (joint) {
        for (int k = 0; k < DY * n; ++k) a.M0[k] = p->M0[k];
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) a.K0[i * n + j] = 0.5 * (p->K0[i * n + j] + p->K0[j * n + i]);
        pd = pd && dt_chol<n>(a.K0, l);
    }
    if (!pd) {
        set_error("K0 (%d, %d) and Psi0 (%d, %d) must be positive definite", n, n, DY, DY);
        return AUXSSM_ERR_ARG;
    }
    a.nu0 = p->nu0;
    a.chi_scale = p->chi_scale;
    a.nobs = syy_nobs[DY * DY];
    return AUXSSM_OK;
}

}  // namespace ax

using namespace ax;

extern "C" {

int auxssm_observation_stats(auxssm_handle h, int dtype, int32_t C, int32_t T, int32_t dx, int32_t dy, int layout, const void* x, const auxssm_arr* yobs,
                             double* stats_out) {
    AX_NEED_H(h);
    if (int rc = ot_check_state(dtype, C, T, dx, dy, layout, x, yobs)) return rc;
    if (!stats_out) {
        set_error("stats_out must be non-NULL");
        return AUXSSM_ERR_ARG;
    }
    if (C == 0) return AUXSSM_OK;
    double* part;
    WsPlan ws;
    ws.add(part, ot_part_bytes(C, T, dx, dy));
    if (int rc = ws.reserve(h)) return rc;
    ot_by_dims(dx, dy, [&](auto a, auto b) {
        constexpr int DX = decltype(a)::value, DY = decltype(b)::value;
        if (dtype == AUXSSM_F32) ot_launch_stats<float, DX, DY>(h, C, T, layout, x, yobs, part, stats_out);
        else ot_launch_stats<double, DX, DY>(h, C, T, layout, x, yobs, part, stats_out);
        return AUXSSM_OK;
    });
    AX_HIP(hipGetLastError());
    return AUXSSM_OK;
}

int auxssm_observation_theta_update(auxssm_handle h, int dtype, int32_t C, int32_t T, int32_t dx, int32_t dy, int layout, const void* x, const auxssm_arr* yobs,
                                    const double* syy_nobs, const auxssm_mniw_prior* prior, int update_mask, const void* chi, const void* eps_w,
                                    const void* eps_a, const auxssm_arr* H, const auxssm_arr* c, const auxssm_arr* R, double* post_out, int32_t* flags) {
    AX_NEED_H(h);
    if (int rc = ot_check_state(dtype, C, T, dx, dy, layout, x, yobs)) return rc;
    if (update_mask != OT_JOINT && update_mask != OT_R_ALONE) {
        set_error("update_mask must be 1 (H, c and R jointly) or 2 (R alone, H and c fixed), got %d", update_mask);
        return AUXSSM_ERR_ARG;
    }
    const bool joint = update_mask == OT_JOINT;
    if (!syy_nobs || !prior || !chi || !eps_w || (joint && !eps_a) || !H || !c || !R || !flags || !H->ptr || !c->ptr || !R->ptr) {
        set_error("syy_nobs/prior/chi/eps_w/eps_a/H/c/R/flags must be non-NULL (post_out may be NULL; eps_a may be NULL when R alone is drawn)");
        return AUXSSM_ERR_ARG;
    }
    if (H->st != 0 || c->st != 0 || R->st != 0) {
        set_error("the step writes a time-invariant observation model: the time strides of H, c and R must be 0");
        return AUXSSM_ERR_ARG;
    }
    if (C > 1 && (H->sc < (int64_t)dy * dx || c->sc < dy || R->sc < (int64_t)dy * dy)) {
        set_error("with C > 1 every chain needs its own H, c, R: chain strides >= dy*dx, dy, dy*dy elements (got %lld, %lld, %lld)", (long long)H->sc,
                  (long long)c->sc, (long long)R->sc);
        return AUXSSM_ERR_ARG;
    }
    return ot_by_dims(dx, dy, [&](auto da, auto db) -> int {
        constexpr int DX = decltype(da)::value, DY = decltype(db)::value;
        OtArgs<DX, DY> a;
        if (int rc = ot_args<DX, DY>(prior, syy_nobs, joint, a)) return rc;
        if (C == 0) return AUXSSM_OK;
        double *part, *full;
        WsPlan ws;
        ws.add(part, ot_part_bytes(C, T, dx, dy));
        ws.add(full, (size_t)C * OtDims<DX, DY>::FULL * sizeof(double));
        if (int rc = ws.reserve(h)) return rc;
        const unsigned grid = (unsigned)((C + OT_FIN_LANES - 1) / OT_FIN_LANES);
        if (dtype == AUXSSM_F32) {
            ot_launch_stats<float, DX, DY>(h, C, T, layout, x, yobs, part, full);
            hipLaunchKernelGGL((k_ot_finish<float, DX, DY>), dim3(grid), dim3(OT_FIN_LANES), 0, h->stream, C, update_mask, a, (const double*)full, (const float*)chi,
                               (const float*)eps_w, (const float*)eps_a, (float*)H->ptr, (long long)H->sc, (float*)c->ptr, (long long)c->sc, (float*)R->ptr,
                               (long long)R->sc, post_out, flags);
        } else {
            ot_launch_stats<double, DX, DY>(h, C, T, layout, x, yobs, part, full);
            hipLaunchKernelGGL((k_ot_finish<double, DX, DY>), dim3(grid), dim3(OT_FIN_LANES), 0, h->stream, C, update_mask, a, (const double*)full,
                               (const double*)chi, (const double*)eps_w, (const double*)eps_a, (double*)H->ptr, (long long)H->sc, (double*)c->ptr,
                               (long long)c->sc, (double*)R->ptr, (long long)R->sc, post_out, flags);
        }
        AX_HIP(hipGetLastError());
        return AUXSSM_OK;
    });
}

}  // extern "C"
