// kalman_plin.hip -- the two kernels AUXSSM_KMODEL_POISSON_LIN_FIRST / _SECOND add to the auxiliary Kalman sweep (api.hip::sweep_plin): the observation factory of
// a Poisson potential behind a loading matrix, y_{t,j} ~ Poisson(exp(h_j' x_t + c_j)), and the rest of the five totals of the acceptance ratio.  Everything that
// depends on dy is here; the pseudo-observations live in the state space (dx <= 4), so the filter, the pathwise sampler and the joint densities are the register
// kernels the other sweeps run.
//
//   k_plin_obs    one lane per (chain, step): the step's 1 + D + D (D + 1) / 2 sums over the channels stay in registers (kalman_plin.h::PlinAcc).  A workgroup takes
//                 256 consecutive steps of PLIN_CG chains.  The counts go through LDS in column blocks of PLIN_JB channels -- a (256, dy) tile does not fit at
//                 dy = 1024 -- with the block's rows of H and c beside them: lane t reads its own row of the tile (row stride PLIN_JB + 1 elements: consecutive
//                 steps on different banks) and every lane the same H_j, c_j (broadcast).  A staged tile serves all the workgroup's chains before the next one
//                 is fetched; one exponential per (chain, step, channel).  Then the auxiliary observation of the sweep's order (plin_finish), the step's potential
//                 value to pot (C, T) in Acc, and at the first linearisation point u = x + sqrt(delta / 2) eps.
//   k_plin_obs_logistic   the same kernel with the channel body of the logit link (AUXSSM_KMODEL_LOGISTIC_LIN_*: plin_accum_logistic): it stages the two further
//                 dy-rows s and w of the size m = s + w y beside c (+ 2 x 64 reals of LDS) and spends one exponential, one reciprocal and one logarithm per (chain,
//                 step, channel).  A __global__ function of its own, so that k_plin_obs keeps its registers.
//   k_plin_terms  one workgroup per (chain, segment of PLIN_SEG steps): the potentials of x' and x summed from what the two factory launches left (no exponential),
//                 the Gaussian terms of the auxiliary observations under dense R (Cholesky in registers) or delta/2 I, and the correction sum -- lanes stride
//                 over the segment's steps, each in Acc, then a tree over the workgroup; k_plin_totals adds a chain's segments in ascending order.  The
//                 segments depend on T alone: a fixed order whatever the launch, no atomics.
#include "kalman_plin.h"

namespace ax {
namespace {

constexpr int PLIN_TT = 256;  // steps per workgroup (= lanes)
constexpr int PLIN_CG = 4;    // chains per workgroup: how often a staged y tile is used
constexpr int PLIN_LD = PLIN_JB + 1;
constexpr int PLIN_SEG = 2048;  // steps per workgroup of k_plin_terms (8 per lane): one chain of T = 16384 keeps 8 CUs busy, not 1

template <typename R> size_t plin_lds_bytes(int D, int link) {
    return ((size_t)PLIN_TT * PLIN_LD + (size_t)PLIN_JB * D + (size_t)PLIN_JB * (link == PLIN_LOGISTIC ? 3 : 1)) * sizeof(R);
}

template <typename R, int D>
__global__ void __launch_bounds__(PLIN_TT)
k_plin_obs(int C, int T, int dy, int order, int ntile, double delta_h, const double* __restrict__ dptr, const R* __restrict__ H, const R* __restrict__ c,
           const R* __restrict__ yobs, long long y_st, const R* __restrict__ xlin, const R* __restrict__ eps, R* __restrict__ u, R* __restrict__ ys,
           R* __restrict__ Rs, Acc* __restrict__ pot) {
    extern __shared__ __align__(16) unsigned char plin_smem[];
    R* sy = reinterpret_cast<R*>(plin_smem);  // [PLIN_TT][PLIN_LD]
    R* sH = sy + PLIN_TT * PLIN_LD;           // [PLIN_JB][D]
    R* sc = sH + PLIN_JB * D;                 // [PLIN_JB]
    const int tid = threadIdx.x;
    const long long t0 = (long long)(blockIdx.x % ntile) * PLIN_TT, t = t0 + tid;
    const int c0 = (int)(blockIdx.x / ntile) * PLIN_CG;
    const bool active = t < T;
    const R delta = (R)(dptr ? dptr[0] : delta_h);
    const R shd = (R)(dptr ? dptr[1] : sqrt(0.5 * delta_h));
    R x[PLIN_CG][D];
    PlinAcc<R, D> acc[PLIN_CG];
#pragma unroll
    for (int i = 0; i < PLIN_CG; ++i) {
        plin_zero(acc[i]);
        const bool on = active && c0 + i < C;  // (c0 + i < C is uniform over the workgroup)
#pragma unroll
        for (int k = 0; k < D; ++k) x[i][k] = on ? xlin[((long long)(c0 + i) * T + t) * D + k] : (R)0;
    }
    for (int j0 = 0; j0 < dy; j0 += PLIN_JB) {
        const int n = dy - j0 < PLIN_JB ? dy - j0 : PLIN_JB;  // (the last block may be ragged)
        __syncthreads();  // the block before has been read by every lane
        for (int idx = tid; idx < PLIN_TT * PLIN_JB; idx += PLIN_TT) {  // 64 consecutive lanes fetch one row's 64 consecutive channels
            const int row = idx / PLIN_JB, col = idx % PLIN_JB;
            const long long tt = t0 + row;
            sy[row * PLIN_LD + col] = (tt < T && col < n) ? yobs[tt * y_st + j0 + col] : r_nan<R>();
        }
        for (int idx = tid; idx < n * D; idx += PLIN_TT) sH[idx] = H[(long long)j0 * D + idx];
        for (int idx = tid; idx < n; idx += PLIN_TT) sc[idx] = c[j0 + idx];
        __syncthreads();
#pragma unroll
        for (int i = 0; i < PLIN_CG; ++i)
            if (c0 + i < C) plin_accum<R, D>(acc[i], x[i], sy + tid * PLIN_LD, sH, sc, n);
    }
#pragma unroll
    for (int i = 0; i < PLIN_CG; ++i) {
        if (!active || c0 + i >= C) continue;
        const long long ct = (long long)(c0 + i) * T + t, off = ct * D;
        R uu[D], yv[D], Om[symsize(D)];
#pragma unroll
        for (int k = 0; k < D; ++k) {
            if (eps) {
                uu[k] = x[i][k] + shd * eps[off + k];
                u[off + k] = uu[k];
            } else {
                uu[k] = u[off + k];
            }
        }
        plin_finish<R, D>(acc[i], x[i], uu, delta, order, yv, Om);
#pragma unroll
        for (int k = 0; k < D; ++k) ys[off + k] = yv[k];
        if (order == 2) {
#pragma unroll
            for (int k = 0; k < D; ++k)
#pragma unroll
                for (int l = 0; l < D; ++l) Rs[off * D + k * D + l] = Om[sidx(D, k, l)];
        }
        pot[ct] = acc[i].val;
    }
}

// k_plin_obs under the logit link: the block's three rows of [c; s; w] staged where k_plin_obs has c, and plin_accum_logistic for plin_accum.  (One body under a
// compile-time link, inlined into both kernels, was tried first: it moved k_plin_obs's registers -- fp32 D = 4 140 -> 134 VGPRs, six SGPRs in four of the eight.)
template <typename R, int D>
__global__ void __launch_bounds__(PLIN_TT)
k_plin_obs_logistic(int C, int T, int dy, int order, int ntile, double delta_h, const double* __restrict__ dptr, const R* __restrict__ H, const R* __restrict__ csw,
           const R* __restrict__ yobs, long long y_st, const R* __restrict__ xlin, const R* __restrict__ eps, R* __restrict__ u, R* __restrict__ ys,
           R* __restrict__ Rs, Acc* __restrict__ pot) {
    extern __shared__ __align__(16) unsigned char plin_smem[];
    R* sy = reinterpret_cast<R*>(plin_smem);  // [PLIN_TT][PLIN_LD]
    R* sH = sy + PLIN_TT * PLIN_LD;           // [PLIN_JB][D]
    R* sc = sH + PLIN_JB * D;                 // [3][PLIN_JB]: the block's c, s and w
    const int tid = threadIdx.x;
    const long long t0 = (long long)(blockIdx.x % ntile) * PLIN_TT, t = t0 + tid;
    const int c0 = (int)(blockIdx.x / ntile) * PLIN_CG;
    const bool active = t < T;
    const R delta = (R)(dptr ? dptr[0] : delta_h);
    const R shd = (R)(dptr ? dptr[1] : sqrt(0.5 * delta_h));
    R x[PLIN_CG][D];
    PlinAcc<R, D> acc[PLIN_CG];
#pragma unroll
    for (int i = 0; i < PLIN_CG; ++i) {
        plin_zero(acc[i]);
        const bool on = active && c0 + i < C;  // (c0 + i < C is uniform over the workgroup)
#pragma unroll
        for (int k = 0; k < D; ++k) x[i][k] = on ? xlin[((long long)(c0 + i) * T + t) * D + k] : (R)0;
    }
    for (int j0 = 0; j0 < dy; j0 += PLIN_JB) {
        const int n = dy - j0 < PLIN_JB ? dy - j0 : PLIN_JB;  // (the last block may be ragged)
        __syncthreads();  // the block before has been read by every lane
        for (int idx = tid; idx < PLIN_TT * PLIN_JB; idx += PLIN_TT) {  // 64 consecutive lanes fetch one row's 64 consecutive channels
            const int row = idx / PLIN_JB, col = idx % PLIN_JB;
            const long long tt = t0 + row;
            sy[row * PLIN_LD + col] = (tt < T && col < n) ? yobs[tt * y_st + j0 + col] : r_nan<R>();
        }
        for (int idx = tid; idx < n * D; idx += PLIN_TT) sH[idx] = H[(long long)j0 * D + idx];
        for (int idx = tid; idx < 3 * n; idx += PLIN_TT) {  // (3 n <= 192 < PLIN_TT: one pass)
            const int q = idx / n, col = idx % n;
            sc[q * PLIN_JB + col] = csw[(long long)q * dy + j0 + col];
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < PLIN_CG; ++i)
            if (c0 + i < C) plin_accum_logistic<R, D>(acc[i], x[i], sy + tid * PLIN_LD, sH, sc, sc + PLIN_JB, sc + 2 * PLIN_JB, n);
    }
#pragma unroll
    for (int i = 0; i < PLIN_CG; ++i) {
        if (!active || c0 + i >= C) continue;
        const long long ct = (long long)(c0 + i) * T + t, off = ct * D;
        R uu[D], yv[D], Om[symsize(D)];
#pragma unroll
        for (int k = 0; k < D; ++k) {
            if (eps) {
                uu[k] = x[i][k] + shd * eps[off + k];
                u[off + k] = uu[k];
            } else {
                uu[k] = u[off + k];
            }
        }
        plin_finish<R, D>(acc[i], x[i], uu, delta, order, yv, Om);
#pragma unroll
        for (int k = 0; k < D; ++k) ys[off + k] = yv[k];
        if (order == 2) {
#pragma unroll
            for (int k = 0; k < D; ++k)
#pragma unroll
                for (int l = 0; l < D; ++l) Rs[off * D + k * D + l] = Om[sidx(D, k, l)];
        }
        pot[ct] = acc[i].val;
    }
}

template <typename R, int D>
__global__ void __launch_bounds__(256)
k_plin_terms(int C, int T, int nseg, double delta_h, const double* __restrict__ dptr, const R* __restrict__ x, const R* __restrict__ xp, const R* __restrict__ u,
             const R* __restrict__ ys1, const R* __restrict__ ys2, const R* __restrict__ R1, const R* __restrict__ R2, const Acc* __restrict__ pot1,
             const Acc* __restrict__ pot2, Acc* __restrict__ part) {
    __shared__ Acc sh[256];
    const int c = (int)(blockIdx.x / nseg), seg = (int)(blockIdx.x % nseg), tid = threadIdx.x;
    const long long t_end = (long long)(seg + 1) * PLIN_SEG < T ? (long long)(seg + 1) * PLIN_SEG : T;
    const R delta = (R)(dptr ? dptr[0] : delta_h);
    const R sd = sqrt_((R)0.5 * delta), lsd = log_(sd);
    Acc acc[5] = {0, 0, 0, 0, 0};
    for (long long t = (long long)seg * PLIN_SEG + tid; t < t_end; t += 256) {
        const long long ct = (long long)c * T + t, off = ct * D;
        R a[D], b[D], y1[D], y2[D];
        R l1 = 0, l2 = 0, cr = 0;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            a[k] = xp[off + k];
            b[k] = x[off + k];
            y1[k] = ys1[off + k];
            y2[k] = ys2[off + k];
            const R uu = u[off + k], e1 = a[k] - uu, e2 = b[k] - uu;
            cr += (e1 * e1 - e2 * e2) / delta;
        }
        if (R1) {
            R O1[symsize(D)], O2[symsize(D)];
#pragma unroll
            for (int k = 0; k < D; ++k)
#pragma unroll
                for (int l = k; l < D; ++l) {
                    O1[sidx_u(D, k, l)] = R1[off * D + k * D + l];
                    O2[sidx_u(D, k, l)] = R2[off * D + k * D + l];
                }
            l1 = plin_norm_logpdf<R, D>(y1, a, O1);
            l2 = plin_norm_logpdf<R, D>(y2, b, O2);
        } else {
#pragma unroll
            for (int k = 0; k < D; ++k) {
                const R z1 = (y1[k] - a[k]) / sd, z2 = (y2[k] - b[k]) / sd;
                l1 += (R)-0.5 * z1 * z1 - lsd - (R)(0.5 * LOG_2PI);
                l2 += (R)-0.5 * z2 * z2 - lsd - (R)(0.5 * LOG_2PI);
            }
        }
        acc[0] += pot2[ct];
        acc[1] += pot1[ct];
        acc[2] += isnan_(l1) ? (Acc)0 : (Acc)l1;  // a step whose term is NaN is dropped (the reference's nansum over time steps)
        acc[3] += isnan_(l2) ? (Acc)0 : (Acc)l2;
        acc[4] += (Acc)cr;
    }
    for (int q = 0; q < 5; ++q) {
        sh[tid] = acc[q];
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (tid < s) sh[tid] += sh[tid + s];
            __syncthreads();
        }
        if (tid == 0) part[((long long)q * C + c) * nseg + seg] = sh[0];
        __syncthreads();
    }
}
// out [5][C]: total q of chain c = its segments' parts, ascending
template <typename R> __global__ void k_plin_totals(int n, int nseg, const Acc* __restrict__ part, R* __restrict__ out) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    Acc v = 0;
    for (int s = 0; s < nseg; ++s) v += part[(long long)g * nseg + s];
    out[g] = (R)v;
}

template <typename R, int D> int run_obs_t(auxssm_ctx* h, const PlinObsArgs& a) {
    const long long ntile = ((long long)a.T + PLIN_TT - 1) / PLIN_TT, ngroup = ((long long)a.C + PLIN_CG - 1) / PLIN_CG;
    if (ntile * ngroup > 0x7fffffffLL) {
        set_error("%s sweep: %lld x %lld workgroups is beyond one launch", a.link == PLIN_LOGISTIC ? "logistic-linear" : "Poisson-linear", ntile, ngroup);
        return AUXSSM_ERR_UNSUPPORTED;
    }
    const size_t lds = plin_lds_bytes<R>(D, a.link);
    const auto kernel = a.link == PLIN_LOGISTIC ? k_plin_obs_logistic<R, D> : k_plin_obs<R, D>;
    if (lds > 48 * 1024) AX_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kernel, dim3((unsigned)(ntile * ngroup)), dim3(PLIN_TT), lds, h->stream, a.C, a.T, a.dy, a.order, (int)ntile, a.delta, a.dptr,
                       (const R*)a.H, (const R*)a.c, (const R*)a.yobs, a.y_st, (const R*)a.xlin, (const R*)a.eps, (R*)a.u, (R*)a.ys, (R*)a.Rs, a.pot);
    AX_HIP(hipGetLastError());
    return AUXSSM_OK;
}
int plin_nseg(int T) { return (T + PLIN_SEG - 1) / PLIN_SEG; }
template <typename R, int D> int run_terms_t(auxssm_ctx* h, const PlinTermsArgs& a) {
    const int nseg = plin_nseg(a.T);
    if ((long long)a.C * nseg > 0x7fffffffLL) {
        set_error("Poisson-linear sweep: %d x %d workgroups is beyond one launch", a.C, nseg);
        return AUXSSM_ERR_UNSUPPORTED;
    }
    hipLaunchKernelGGL((k_plin_terms<R, D>), dim3((unsigned)((long long)a.C * nseg)), dim3(256), 0, h->stream, a.C, a.T, nseg, a.delta, a.dptr, (const R*)a.x,
                       (const R*)a.xp, (const R*)a.u, (const R*)a.ys1, (const R*)a.ys2, (const R*)a.R1, (const R*)a.R2, a.pot1, a.pot2, a.part);
    hipLaunchKernelGGL((k_plin_totals<R>), dim3((5 * a.C + 255) / 256), dim3(256), 0, h->stream, 5 * a.C, nseg, (const Acc*)a.part, (R*)a.out);
    AX_HIP(hipGetLastError());
    return AUXSSM_OK;
}

#define PLIN_DISPATCH(FN, ARGS)                                                 \
    switch (a.D) {                                                              \
        case 1: return dtype == AUXSSM_F32 ? FN<float, 1> ARGS : FN<double, 1> ARGS; \
        case 2: return dtype == AUXSSM_F32 ? FN<float, 2> ARGS : FN<double, 2> ARGS; \
        case 3: return dtype == AUXSSM_F32 ? FN<float, 3> ARGS : FN<double, 3> ARGS; \
        case 4: return dtype == AUXSSM_F32 ? FN<float, 4> ARGS : FN<double, 4> ARGS; \
    }                                                                           \
    set_error("Poisson-linear sweep: dx = %d is not instantiated (1 <= dx <= 4)", a.D); \
    return AUXSSM_ERR_UNSUPPORTED;

}  // namespace

size_t plin_terms_part_bytes(int C, int T) { return (size_t)5 * C * plin_nseg(T) * sizeof(Acc); }
int run_plin_obs(auxssm_ctx* h, int dtype, const PlinObsArgs& a) { PLIN_DISPATCH(run_obs_t, (h, a)) }
int run_plin_terms(auxssm_ctx* h, int dtype, const PlinTermsArgs& a) { PLIN_DISPATCH(run_terms_t, (h, a)) }

}  // namespace ax
