// kalman_mvt.hip -- the spatial example's auxiliary Kalman sampler (examples/spatial/auxiliary_kalman.py) as batched scalar sweeps.
//
// The example batches its model: the state is (T, d, 1), the dynamics are d independent scalar random walks, H = 1 and R is one scalar per component.  The
// components meet only in the gradient of the multivariate-t log-potential and in the log target, so a sweep of C chains is C * d independent scalar Kalman
// filters / pathwise samplers of length T around a gradient kernel that is elementwise in time:
//
//   k_mvt_obs   one wave per (chain, t), lane = component: r = y_t - x_t, w = prec r (prec in LDS, odd row stride, one row read serving four items; r_j by
//               v_readlane), q = r . w, the auxiliary observation of the sweep's order and the step's potential value; at the first linearisation point also
//               u = x + sqrt(delta / 2) eps
//   k_mvt_fwd   one lane per (chain, component), sequential in t: the scalar filter (1 - K = R / S, never 1 - P / S), filtered moments, per-lane log-likelihood
//               (one reciprocal per step, one logarithm per chunk of eight); REV: no moments, but the densities of x under the reverse model in the same walk
//   k_mvt_bwd   one lane per (chain, component), backwards in t: the pathwise sampler, and in the same walk posterior_logpdf's terms at x', the prior part of the
//               log target and the correction sum
//   k_mvt_sums  one wave per chain: the per-lane totals and the per-step potential values in a fixed order that does not depend on C
//
// Every per-chain total is accumulated in Acc (fp64) from the per-lane increments on, also in fp32 sweeps: the increments themselves are formed in Acc from the
// working-precision moments, so an fp32 sweep rounds its state and its moments, not its log-densities.
#include "kalman_mvt.h"

namespace ax {
namespace {

__device__ __forceinline__ float fma_(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ __forceinline__ float max_real(float) { return 3.402823466e+38f; }
__device__ __forceinline__ double max_real(double) { return 1.7976931348623157e+308; }
// jnp.nan_to_num: NaN -> 0, +-inf -> +-the largest finite value
template <typename R> __device__ __forceinline__ R nan_to_num_(R v) {
    if (v != v) return (R)0;
    if (!finite_(v)) return v > 0 ? max_real(v) : -max_real(v);
    return v;
}
// scipy.stats.norm.logpdf with the variance's inverse and half its logarithm given (both loop invariants of the walks): the increments are formed in Acc
__device__ __forceinline__ Acc norm_lp(Acc diff, Acc ivar, Acc half_log_var) { return -0.5 * diff * diff * ivar - half_log_var - 0.5 * LOG_2PI; }
__device__ __forceinline__ void add_finite(Acc& tot, Acc v) {  // nansum
    if (v == v) tot += v;
}
__device__ __forceinline__ Acc wave_sum(Acc v) {  // butterfly: the same order whatever the launch, every lane ends with the total
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// the auxiliary observation's variance of component k: delta / 2 (first order) or Omega_k = 1 / (-h_k + 2 / delta), h_k = -nu prec_kk / (nu - 2) (second order)
template <typename R, int ORDER> __device__ __forceinline__ R aux_var(R delta, R nu, R pkk, R& h) {
    if (ORDER == 1) {
        h = (R)0;
        return (R)0.5 * delta;
    }
    h = -nu * pkk / (nu - (R)2);
    return (R)1 / (-h + (R)2 / delta);
}

constexpr int OBS_WAVES = 4, OBS_ITEMS = 4;
// the value lane j holds, in every lane (j wave-uniform)
__device__ __forceinline__ float lane_bcast(float v, int j) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j)); }
__device__ __forceinline__ double lane_bcast(double v, int j) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), j), __builtin_amdgcn_readlane(__double2loint(v), j));
}

template <typename R, int ORDER, bool FIRST>
__global__ void __launch_bounds__(64 * OBS_WAVES)
k_mvt_obs(int C, int T, int D, double delta_h, const double* __restrict__ dptr, const R* __restrict__ prec, const R* __restrict__ nu_p,
          const R* __restrict__ yobs, long long y_st, const R* __restrict__ xlin, const R* __restrict__ eps, R* __restrict__ u, R* __restrict__ ys,
          Acc* __restrict__ pot) {
    extern __shared__ __align__(16) unsigned char mvt_smem[];
    R* sp = reinterpret_cast<R*>(mvt_smem);
    const int ld = D | 1;  // odd row stride: lane k reads prec[k][j], the lanes of a group on distinct banks
    for (int i = threadIdx.x; i < D * D; i += 64 * OBS_WAVES) sp[(i / D) * ld + (i % D)] = prec[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool on = lane < D;
    const R delta = (R)(dptr ? dptr[0] : delta_h);
    const R shd = (R)(dptr ? dptr[1] : sqrt(0.5 * delta_h));
    const R nu = nu_p[0];
    const R* row = sp + (on ? lane : 0) * ld;
    R h;
    const R om = aux_var<R, ORDER>(delta, nu, row[on ? lane : 0], h);
    const long long items = (long long)C * T, stride = (long long)gridDim.x * OBS_WAVES;
    // OBS_ITEMS (chain, t) items per pass: one read of prec[k][j] from LDS serves them all; r_j comes from lane j's register (v_readlane, j is wave-uniform)
    for (long long it0 = (long long)blockIdx.x * OBS_WAVES + wave; it0 < items; it0 += stride * OBS_ITEMS) {
        R xv[OBS_ITEMS], uv[OBS_ITEMS], r[OBS_ITEMS], w[OBS_ITEMS];
#pragma unroll
        for (int i = 0; i < OBS_ITEMS; ++i) {
            const long long it = it0 + i * stride;
            xv[i] = uv[i] = r[i] = w[i] = 0;
            if (on && it < items) {
                const long long off = it * D + lane;
                xv[i] = xlin[off];
                uv[i] = FIRST ? xv[i] + shd * eps[off] : u[off];
                r[i] = yobs[(it % T) * y_st + lane] - xv[i];
            }
        }
        for (int j = 0; j < D; ++j) {  // ascending j
            const R p = row[j];
#pragma unroll
            for (int i = 0; i < OBS_ITEMS; ++i) w[i] = fma_(p, lane_bcast(r[i], j), w[i]);
        }
#pragma unroll
        for (int i = 0; i < OBS_ITEMS; ++i) {
            const long long it = it0 + i * stride;
            if (it >= items) break;  // (wave-uniform)
            const long long off = it * D + lane;
            const R q = (R)wave_sum(on ? (Acc)(r[i] * w[i]) : (Acc)0);
            R g = ((nu + (R)D) * w[i]) / (nu + q);
            R yv;
            if (ORDER == 1) {
                g = nan_to_num_(g);
                yv = uv[i] + ((R)0.5 * delta) * g;
            } else {
                yv = om * ((R)2 * uv[i] / delta + g - h * xv[i]);
            }
            if (on) {
                if (FIRST) u[off] = uv[i];
                ys[off] = yv;
            }
            if (lane == 0) {
                const Acc v = -0.5 * ((Acc)nu + (Acc)D) * log1p((Acc)q / (Acc)nu);
                pot[it] = v != v ? (Acc)0 : v;
            }
        }
    }
}

// lanes[q][C * D]: 0 ell_prop | 1 obs + prior terms of x' | 2 prior terms of x' | 3 correction | 4 ell_rev | 5 obs + prior terms of x (reverse model) | 6 prior terms of x
constexpr int MVT_NQ = 7;
constexpr int WALK_CHUNK = 8;  // steps fetched ahead by the sequential walks

template <typename R, int ORDER, bool REV>
__global__ void __launch_bounds__(64)
k_mvt_fwd(int C, int T, int D, double delta_h, const double* __restrict__ dptr, const R* __restrict__ m0, const R* __restrict__ P0, const R* __restrict__ F,
          const R* __restrict__ Q, const R* __restrict__ b, const R* __restrict__ prec, const R* __restrict__ nu_p, const R* __restrict__ ys,
          const R* __restrict__ x, R* __restrict__ ms, R* __restrict__ Ps, Acc* __restrict__ lanes) {
    const long long CD = (long long)C * D, g = (long long)blockIdx.x * 64 + threadIdx.x;
    if (g >= CD) return;
    const int k = (int)(g % D);
    const long long base = (g / D) * T * D + k;  // consecutive lanes = consecutive components: a wave's loads at one t are contiguous runs of the (C, T, D) arrays
    const R delta = (R)(dptr ? dptr[0] : delta_h);
    R h;
    const R Rk = aux_var<R, ORDER>(delta, nu_p[0], prec[(long long)k * D + k], h);
    const R m0k = m0[k], P0k = P0[k], Fk = F[k], Qk = Q[k], bk = b[k];
    const Acc hlR = 0.5 * log((Acc)Rk), hlQ = 0.5 * log((Acc)Qk), hlP0 = 0.5 * log((Acc)P0k);
    const Acc iR = 1.0 / (Acc)Rk, iQ = 1.0 / (Acc)Qk, iP0 = 1.0 / (Acc)P0k;
    R m = m0k, P = P0k;
    Acc ell = 0, jp = 0, pr = 0;
    // The loads do not depend on the recurrence: a chunk of U steps is fetched while the chunk before it is walked (one step ahead would leave a load's whole
    // latency on every step of a lane that has the SIMD to itself)
    constexpr int U = WALK_CHUNK;
    R yn[U], xn[U], xprev = 0;
#pragma unroll
    for (int i = 0; i < U; ++i) {
        yn[i] = i < T ? ys[base + (long long)i * D] : (R)0;
        xn[i] = REV && i < T ? x[base + (long long)i * D] : (R)0;
    }
    for (int t0 = 0; t0 < T; t0 += U) {
        R yc[U], xc[U];
        Acc sprod = 1;  // the chunk's innovation variances multiplied up: one logarithm per chunk instead of one per step (U factors: far inside the range)
#pragma unroll
        for (int i = 0; i < U; ++i) {
            yc[i] = yn[i];
            xc[i] = xn[i];
            const int tn = t0 + U + i;
            yn[i] = tn < T ? ys[base + (long long)tn * D] : (R)0;
            if (REV) xn[i] = tn < T ? x[base + (long long)tn * D] : (R)0;
        }
#pragma unroll
        for (int i = 0; i < U; ++i) {
            const int t = t0 + i;
            if (t >= T) break;
            const R y = yc[i];
            if (t > 0) {
                m = Fk * m + bk;
                P = Fk * P * Fk + Qk;
            }
            if (finite_(y)) {  // a missing auxiliary observation is skipped: predicted moments pass through, no log-likelihood increment
                const R S = Rk + P, iS = (R)1 / S;
                sprod *= (Acc)S;
                add_finite(ell, norm_lp((Acc)y - (Acc)m, (Acc)iS, (Acc)0));
                m = m + (P * iS) * (y - m);
                P = P * (Rk * iS);  // 1 - K = R / S
            }
            if (!REV) {
                ms[base + (long long)t * D] = m;
                Ps[base + (long long)t * D] = P;
            } else {
                add_finite(jp, norm_lp((Acc)y - (Acc)xc[i], iR, hlR));
                const Acc p = t == 0 ? norm_lp((Acc)xc[i] - (Acc)m0k, iP0, hlP0) : norm_lp((Acc)xc[i] - ((Acc)Fk * (Acc)xprev + (Acc)bk), iQ, hlQ);
                add_finite(pr, p);
                xprev = xc[i];
            }
        }
        add_finite(ell, -0.5 * log(sprod));
    }
    if (!REV) {
        lanes[g] = ell;
    } else {
        lanes[4 * CD + g] = ell;
        lanes[5 * CD + g] = jp + pr;
        lanes[6 * CD + g] = pr;
    }
}

template <typename R, int ORDER>
__global__ void __launch_bounds__(64)
k_mvt_bwd(int C, int T, int D, double delta_h, const double* __restrict__ dptr, const R* __restrict__ m0, const R* __restrict__ P0, const R* __restrict__ F,
          const R* __restrict__ Q, const R* __restrict__ b, const R* __restrict__ prec, const R* __restrict__ nu_p, const R* __restrict__ ys,
          const R* __restrict__ ms, const R* __restrict__ Ps, const R* __restrict__ eps, const R* __restrict__ x, const R* __restrict__ u, R* __restrict__ xp,
          Acc* __restrict__ lanes) {
    const long long CD = (long long)C * D, g = (long long)blockIdx.x * 64 + threadIdx.x;
    if (g >= CD) return;
    const int k = (int)(g % D);
    const long long base = (g / D) * T * D + k;
    const Acc delta = dptr ? dptr[0] : delta_h;
    R h;
    const R Rk = aux_var<R, ORDER>((R)delta, nu_p[0], prec[(long long)k * D + k], h);
    const R m0k = m0[k], P0k = P0[k], Fk = F[k], Qk = Q[k], bk = b[k];
    const Acc hlR = 0.5 * log((Acc)Rk), hlQ = 0.5 * log((Acc)Qk), hlP0 = 0.5 * log((Acc)P0k);
    const Acc iR = 1.0 / (Acc)Rk, iQ = 1.0 / (Acc)Qk, iP0 = 1.0 / (Acc)P0k, idelta = 1.0 / delta;
    Acc jp = 0, pr = 0, corr = 0;
    R xnext = 0;
    constexpr int U = WALK_CHUNK;
    R mn[U], Pn[U], en[U], yn[U], xn[U], un[U];  // steps T - 1 - i of the chunk ahead (see k_mvt_fwd)
#pragma unroll
    for (int i = 0; i < U; ++i) {
        const int t = T - 1 - i;
        const long long o = base + (long long)(t < 0 ? 0 : t) * D;
        mn[i] = ms[o]; Pn[i] = Ps[o]; en[i] = eps[o]; yn[i] = ys[o]; xn[i] = x[o]; un[i] = u[o];
    }
    for (int t0 = T - 1; t0 >= 0; t0 -= U) {
        R mc[U], Pc[U], ec[U], yc[U], xc[U], uc[U];
#pragma unroll
        for (int i = 0; i < U; ++i) {
            mc[i] = mn[i]; Pc[i] = Pn[i]; ec[i] = en[i]; yc[i] = yn[i]; xc[i] = xn[i]; uc[i] = un[i];
            const int t = t0 - U - i;
            const long long o = base + (long long)(t < 0 ? 0 : t) * D;  // (past the start: a valid address, never used)
            mn[i] = ms[o]; Pn[i] = Ps[o]; en[i] = eps[o]; yn[i] = ys[o]; xn[i] = x[o]; un[i] = u[o];
        }
#pragma unroll
        for (int i = 0; i < U; ++i) {
            const int t = t0 - i;
            if (t < 0) break;
            const R m = mc[i], P = Pc[i], e = ec[i];
            R xs;
            if (t == T - 1) {
                xs = m + nan_to_num_(sqrt_(P)) * e;
            } else {  // sampling.py::mean_and_chol in one dimension; the increment's variance P - gain S gain = P Q / S without the cancellation
                const R S = Fk * P * Fk + Qk, iS = (R)1 / S;
                const R gain = P * Fk * iS;
                const R L = nan_to_num_(sqrt_(P * Qk * iS));
                const R inc = (m - gain * (Fk * m + bk)) + L * e;
                xs = gain * xnext + inc;
                add_finite(pr, norm_lp((Acc)xnext - ((Acc)Fk * (Acc)xs + (Acc)bk), iQ, hlQ));
            }
            xp[base + (long long)t * D] = xs;
            add_finite(jp, norm_lp((Acc)yc[i] - (Acc)xs, iR, hlR));
            const Acc dp = (Acc)xs - (Acc)uc[i], dc = (Acc)xc[i] - (Acc)uc[i];
            corr += (dp * dp - dc * dc) * idelta;
            if (t == 0) add_finite(pr, norm_lp((Acc)xs - (Acc)m0k, iP0, hlP0));
            xnext = xs;
        }
    }
    lanes[1 * CD + g] = jp + pr;
    lanes[2 * CD + g] = pr;
    lanes[3 * CD + g] = corr;
}

// one wave per chain: sums [5][C] = lp_prop, lp_rev (log-likelihoods taken off here, in Acc), lt_prop, lt_rev, corr
template <typename R>
__global__ void __launch_bounds__(64) k_mvt_sums(int C, int T, int D, const Acc* __restrict__ lanes, const Acc* __restrict__ pot1, const Acc* __restrict__ pot2,
                                                 Acc* __restrict__ sums, R* __restrict__ ell0) {
    const int c = blockIdx.x, lane = threadIdx.x;
    const long long CD = (long long)C * D;
    Acc v[MVT_NQ];
#pragma unroll
    for (int q = 0; q < MVT_NQ; ++q) v[q] = wave_sum(lane < D ? lanes[q * CD + (long long)c * D + lane] : (Acc)0);
    Acc p1 = 0, p2 = 0;
    for (int t = lane; t < T; t += 64) {
        p1 += pot1[(long long)c * T + t];
        p2 += pot2[(long long)c * T + t];
    }
    p1 = wave_sum(p1);
    p2 = wave_sum(p2);
    if (lane == 0) {
        sums[c] = v[1] - v[0];
        sums[C + c] = v[5] - v[4];
        sums[2 * C + c] = v[2] + p2;  // log target at x': prior + potential at the second linearisation point
        sums[3 * C + c] = v[6] + p1;
        sums[4 * C + c] = v[3];
        ell0[c] = (R)0;
    }
}

template <typename R, int ORDER> int run_mvt_t(auxssm_ctx* h, const MvtArgs& a) {
    const int C = a.C, T = a.T, D = a.D;
    const size_t CTD = (size_t)C * T * D, sR = sizeof(R);
    R* u = (R*)ws_take(h, CTD * sR);
    R* ys = (R*)ws_take(h, CTD * sR);
    R* ms = (R*)ws_take(h, CTD * sR);
    R* Ps = (R*)ws_take(h, CTD * sR);
    Acc* pot1 = (Acc*)ws_take(h, (size_t)C * T * sizeof(Acc));
    Acc* pot2 = (Acc*)ws_take(h, (size_t)C * T * sizeof(Acc));
    Acc* lanes = (Acc*)ws_take(h, (size_t)MVT_NQ * C * D * sizeof(Acc));
    if (!u || !ys || !ms || !Ps || !pot1 || !pot2 || !lanes) return AUXSSM_ERR_NOMEM;
    const R *m0 = (const R*)a.m0, *P0 = (const R*)a.P0, *F = (const R*)a.F, *Q = (const R*)a.Q, *b = (const R*)a.b, *prec = (const R*)a.prec, *nu = (const R*)a.nu;
    const R *x = (const R*)a.x, *yobs = (const R*)a.yobs;
    R* xp = (R*)a.xp;
    const long long items = (long long)C * T;
    const long long want = (items + OBS_WAVES * OBS_ITEMS - 1) / (OBS_WAVES * OBS_ITEMS), cap = (long long)h->num_cu * 4;
    const dim3 og((unsigned)(want < cap ? want : cap)), ob(64 * OBS_WAVES);
    const size_t lds = (size_t)D * (D | 1) * sR;
    const dim3 lg((unsigned)(((long long)C * D + 63) / 64)), lb(64);
    {  // observations linearised at x (with u formed on the way), filter, pathwise sample
        ProfScope ps(h, AUXSSM_K_FACTORY);
        hipLaunchKernelGGL((k_mvt_obs<R, ORDER, true>), og, ob, lds, h->stream, C, T, D, a.delta, a.dptr, prec, nu, yobs, a.y_st, x, (const R*)a.eps_aux, u, ys, pot1);
    }
    {
        ProfScope ps(h, AUXSSM_K_FILTER_SCAN);
        hipLaunchKernelGGL((k_mvt_fwd<R, ORDER, false>), lg, lb, 0, h->stream, C, T, D, a.delta, a.dptr, m0, P0, F, Q, b, prec, nu, (const R*)ys, (const R*)nullptr, ms, Ps,
                           lanes);
    }
    {
        ProfScope ps(h, AUXSSM_K_SAMPLE_SCAN);
        hipLaunchKernelGGL((k_mvt_bwd<R, ORDER>), lg, lb, 0, h->stream, C, T, D, a.delta, a.dptr, m0, P0, F, Q, b, prec, nu, (const R*)ys, (const R*)ms, (const R*)Ps,
                           (const R*)a.eps_samp, x, (const R*)u, xp, lanes);
    }
    {  // reverse move: observations linearised at x', the filter for its marginal likelihood with the densities of x in the same walk
        ProfScope ps(h, AUXSSM_K_FACTORY);
        hipLaunchKernelGGL((k_mvt_obs<R, ORDER, false>), og, ob, lds, h->stream, C, T, D, a.delta, a.dptr, prec, nu, yobs, a.y_st, (const R*)xp, (const R*)nullptr, u, ys,
                           pot2);
    }
    {
        ProfScope ps(h, AUXSSM_K_FILTER_SCAN);
        hipLaunchKernelGGL((k_mvt_fwd<R, ORDER, true>), lg, lb, 0, h->stream, C, T, D, a.delta, a.dptr, m0, P0, F, Q, b, prec, nu, (const R*)ys, x, (R*)nullptr,
                           (R*)nullptr, lanes);
    }
    {
        ProfScope ps(h, AUXSSM_K_LOGPDF);
        hipLaunchKernelGGL((k_mvt_sums<R>), dim3(C), dim3(64), 0, h->stream, C, T, D, (const Acc*)lanes, (const Acc*)pot1, (const Acc*)pot2, a.sums, (R*)a.ell0);
    }
    AX_HIP(hipGetLastError());
    return AUXSSM_OK;
}

}  // namespace

size_t mvt_ws_bytes(int dtype, int C, int T, int D) {
    const size_t sR = dtype == AUXSSM_F32 ? 4 : 8, CT = (size_t)C * T;
    return 4 * (CT * D * sR + 256) + 2 * (CT * sizeof(Acc) + 256) + (size_t)MVT_NQ * C * D * sizeof(Acc) + 256;
}

int run_mvt(auxssm_ctx* h, int dtype, const MvtArgs& a) {
    if (dtype == AUXSSM_F32) return a.order == 1 ? run_mvt_t<float, 1>(h, a) : run_mvt_t<float, 2>(h, a);
    return a.order == 1 ? run_mvt_t<double, 1>(h, a) : run_mvt_t<double, 2>(h, a);
}

}  // namespace ax
