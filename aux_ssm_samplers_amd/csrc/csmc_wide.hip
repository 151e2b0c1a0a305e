// csmc_wide.hip -- the conditional-SMC sweep for WIDE states with FEW particles: 4 < dx <= 32, N <= 64 (the reference's own timed stochastic-volatility
// protocol is D = 30, N = 25, T = 250: examples/stochastic_volatility/experiment.sh:1-10, experiment.py:38-55, auxiliary_csmc.py:14-46).
//
// Same algorithm, same sweep contract (csmc_sweep.h: unnormalised weights shifted by a bound or the exact maximum, DPP-order cumsum, descent search,
// ballot-counted single draw, reciprocal Cholesky diagonals, det_exp / det_log, explicit fma) and the same oracle (oracle/csmc_ref.c, MAXD = 32) as the
// register kernels of csmc.hip -- what changes is where a particle lives (the register kernels keep R x[D], eps[D], mu[D], z[D] per lane and the model BY VALUE
// in the kernel arguments, which stops at dx = 4): here a particle's dx components sit ACROSS the 32 lanes of a half-wave, two particles per wave, 16 waves per
// chain while there are CUs to spare (8 beyond), the model's matrices in LDS.  Linear-Gaussian transitions, every potential / proposal of the family,
// gradient-informed proposals (csmc/independent.py:57-75 gradient=True, :173-190, :252-268; both AUXSSM_GRAD_* weightings: the reference's own SV protocol
// exposes --gradient at D = 30) and time-varying transitions (the step's F_t, b_t, chol Q_t re-staged into LDS before the step's first barrier) since round 4.
// Guided proposals (AUXSSM_PROP_AUX_GUIDED, csmc_sweep.h::GuidedT) are a compile-time variant of the forward kernel (k_cw2_fwd<R, NW2, true>): the step's K_t and chol Lambda_t staged
// into LDS like a time-varying transition, one more row product and one more blocked log-density per particle; the backward kernel is shared.
// A coupled potential (csmc_sweep.h::PotV: the multivariate-t potential AUXSSM_POT_MVT, the linear-Gaussian observation potential AUXSSM_POT_LIN_GAUSS) is a compile-time
// variant in the same way (k_cw2_fwd<R, NW2, GD, V>): its matrix (the precision matrix / the whitened observation matrix) staged once per workgroup, one more row
// product per particle (coupled_half); its sweeps carry no bound array (csmc.hip), every step shifts by its exact maximum.
// (The first version of this file -- one wave per chain, one lane per particle walking its dx x dx products alone: 30.5 ms per sweep of the SV protocol against
// 2.6 now -- is in the history)
//
// In-kernel draws (AUXSSM_NOISE_THREEFRY) use the NATURAL flat indices of the explicit arrays -- eps_prop[c][t][n][k] = normal ((c T + t) N + n) dx + k of
// stream 2, u_res[c][s][n] = uniform (c (T-1) + s) N + n of stream 3, u_bwd[c][t] = uniform c T + t of stream 4 -- not the two-steps-per-block packing
// of the register kernels (csmc/_device.py::key_noise(wide=True) builds the equivalent arrays).
#include "csmc_wide_shared.h"

namespace ax {

// e_i = exp(lw_i - max lw) over ONE wave (csmc_sweep.h::block_expmax)
template <typename R> __device__ __forceinline__ R wave_expmax(R lw, R* m_out) {
    R m = wave_max_dpp(lw);
    if (!(m - m == 0)) m = 0;
    if (m_out) *m_out = m;
    return det_exp(lw - m);
}
// the descent search of the sweep contract on a wave's cumulative weights held in LDS (unpadded: at most 64 entries)
template <typename R> __device__ __forceinline__ int search_w(const R* c, int N, R r) {
    int s0 = 1;
    while (s0 * 2 < N) s0 *= 2;
    int pos = 0;
    for (int s = s0; s > 0; s >>= 1) {
        const int q = pos + s - 1;
        pos += (q < N && c[q < N ? q : N - 1] < r) ? s : 0;
    }
    return pos < N - 1 ? pos : N - 1;
}

// =================================================================================================================================================
// Both passes: NW2 waves per chain, a particle's dx components ACROSS the 32 lanes of a half-wave (two particles per wave, particle
// i = 2 NW2 s + 2 wave + half in pass s of ceil(N / (2 NW2))).  Everything the contract orders is kept in its order:
//   * a mean component is one dot product, accumulated over j = 0 .. dx - 1 by the lane that owns the component;
//   * the forward substitution runs COLUMN by column -- z_j = acc_j / L_jj is final once columns < j have been applied, it is broadcast inside the
//     half-wave by v_readlane and every lane k > j applies acc_k = fma(-L_kj, z_j, acc_k): each acc_k receives the same updates in the same order
//     as the row-oriented loop of the contract (csmc_sweep.h::gauss_chol_logpdf), so z, q = sum z_k^2 (accumulated in k order by every lane alike) and the densities are bit-identical;
//   * the potential's sum over components is accumulated in component order from readlane broadcasts of the per-component terms;
//   * weights, cumulative sums, searches and the single draw of the backward pass are done by wave 0 with one lane per particle, exactly as before.
// Two workgroup barriers per time step in either pass.  In-kernel draws keep the natural flat indices (and use both normals of a Threefry block).
template <typename R> struct Cw2Lds {
    int D, S;
    R *F, *LQ, *b, *iL, *c, *lwv, *xa, *xb, *eps, *blk;
    int* idx;
    R *Kg, *Lg, *blkg, *dv;  // guided proposals only (behind idx): the step's K_t and chol Lambda_t, the block table of chol Lambda_t, u~ - pred of every half-wave
    R* pot_mat;              // coupled potentials only (behind everything else): the potential's matrix, rows zero-padded like F's
    __device__ Cw2Lds(char* smem, int D_, bool guided = false, bool coupled = false) : D(D_), S(CSW_MAXD + 1) {  // rows padded with zeros to 32 columns (+ 1: odd stride): every component loop runs 32 steps, unrolled
        F = (R*)smem;           // [D][S]
        LQ = F + D * S;         // [D][S]
        b = LQ + D * S;
        iL = b + D;
        c = iL + D;             // [64]
        lwv = c + 64;           // [64]
        xa = lwv + 64;          // [64][S]
        xb = xa + 64 * S;       // [64][S]
        eps = xb + 64 * S;      // [64][S]
        blk = eps + 64 * S;     // [8][12] the 4 x 4 diagonal blocks of chol Q and the reciprocal diagonal, in the order gauss_half_blk reads them
        idx = (int*)(blk + 96);  // [64]
        if (guided) {
            Kg = (R*)(idx + 64);  // [D][S]
            Lg = Kg + D * S;      // [D][S]
            blkg = Lg + D * S;    // [8][12]
            dv = blkg + 96;       // [32][S]
        }
        if (coupled) pot_mat = guided ? dv + 32 * S : (R*)(idx + 64);  // [D][S]
    }
    static constexpr size_t pot_mat_bytes(int D) { return (size_t)D * (CSW_MAXD + 1) * sizeof(R); }
    static constexpr size_t guided_bytes(int D) { return ((size_t)2 * D * (CSW_MAXD + 1) + 96 + (size_t)32 * (CSW_MAXD + 1)) * sizeof(R); }
    static constexpr size_t bytes(int D) { return ((size_t)2 * D * (CSW_MAXD + 1) + 2 * D + 128 + (size_t)3 * 64 * (CSW_MAXD + 1) + 96) * sizeof(R) + 64 * sizeof(int) + 64; }
    // the forward pass's plan: guided adds two D x 33 matrices, one block table and 32 rows of u~ - pred (96 320 bytes in all at dx = 32 in fp64), a coupled
    // potential its D x 33 matrix (with the guided tables 104 768 bytes, the largest plan of this file)
    static constexpr size_t fwd_bytes(int D, bool guided, bool coupled) { return bytes(D) + (guided ? guided_bytes(D) : 0) + (coupled ? pot_mat_bytes(D) : 0); }
};
static_assert(Cw2Lds<double>::fwd_bytes(CSW_MAXD, true, false) <= 160 * 1024, "the guided forward pass must fit the 160 KB of LDS of a CU");
static_assert(Cw2Lds<double>::fwd_bytes(CSW_MAXD, true, true) <= 160 * 1024, "the guided forward pass with a coupled potential must fit the 160 KB of LDS of a CU");
// entry `tid` (< 96) of the block table gauss_half_blk reads, for the lower factor Lf (leading dimension D) with reciprocal diagonal iLf:
// block jb = 4 (tid / 12): [L10 L20 L21 L30 L31 L32 | i0 i1 i2 i3 | 0 0], zeros beyond D
template <typename R> __device__ __forceinline__ R cw2_blk_entry(const R* Lf, const R* iLf, int D, int tid) {
    const int bq = tid / 12, e = tid - 12 * bq, jb = 4 * bq;
    const int rr[6] = {1, 2, 2, 3, 3, 3}, cc[6] = {0, 0, 1, 0, 1, 2};
    R v = 0;
    if (e < 6) {
        const int r = jb + rr[e], q = jb + cc[e];
        v = r < D ? Lf[r * D + q] : (R)0;
    } else if (e < 10) {
        v = jb + e - 6 < D ? iLf[jb + e - 6] : (R)0;
    }
    return v;
}
template <typename R> __device__ __forceinline__ void cw2_stage(const FkW<R>& m, Cw2Lds<R>& L, int tid, int nt) {
    const int D = m.D, S = L.S;
    for (int i = tid; i < D * S; i += nt) {
        const int r = i / S, q = i - r * S;
        L.F[i] = q < D ? m.F[r * D + q] : (R)0;
        L.LQ[i] = q < D ? m.LQ[r * D + q] : (R)0;
    }
    for (int i = tid; i < D; i += nt) L.b[i] = m.b[i], L.iL[i] = m.iLQ[i];
    for (int i = tid; i < 64 * S; i += nt) L.xa[i] = 0, L.xb[i] = 0, L.eps[i] = 0;
    if (tid < 96) L.blk[tid] = cw2_blk_entry<R>(m.LQ, m.iLQ, D, tid);
    __syncthreads();
}
// time-varying transitions: the rows of transition tt -> tt + 1 replace the staged model (same layout; called by every thread between the two barriers that
// separate the particle sections of consecutive steps, so no section reads a half-written model)
template <typename R> __device__ __forceinline__ void cw2_stage_t(const FkW<R>& m, Cw2Lds<R>& L, long long tt, int tid, int nt) {
    const int D = m.D, S = L.S;
    const R* F = m.Ft + tt * D * D;
    const R* LQ = m.LQt + tt * D * D;
    const R* b = m.bt + tt * D;
    const R* iL = m.idt + tt * D;
    for (int i = tid; i < D * S; i += nt) {
        const int r = i / S, q = i - r * S;
        L.F[i] = q < D ? F[r * D + q] : (R)0;
        L.LQ[i] = q < D ? LQ[r * D + q] : (R)0;
    }
    for (int i = tid; i < D; i += nt) L.b[i] = b[i], L.iL[i] = iL[i];
    if (tid < 96) L.blk[tid] = cw2_blk_entry<R>(LQ, iL, D, tid);
}
// guided proposals: the step's K_t and chol Lambda_t (row t of the table k_csmc_gtab built) into LDS, rows zero-padded like the model's, and the block table of
// chol Lambda_t in the order gauss_half_blk reads it; called where cw2_stage_t is, between the two barriers that separate the particle sections of two steps
template <typename R> __device__ __forceinline__ void cw2_stage_g(const GuidedT<R>& g, Cw2Lds<R>& L, int tid, int nt) {
    const int D = L.D, S = L.S;
    for (int i = tid; i < D * S; i += nt) {
        const int r = i / S, q = i - r * S;
        L.Kg[i] = q < D ? g.K[r * D + q] : (R)0;
        L.Lg[i] = q < D ? g.L[r * D + q] : (R)0;
    }
    if (tid < 96) L.blkg[tid] = cw2_blk_entry<R>(g.L, g.iL, D, tid);
}
// coupled potentials: the potential's matrix into LDS, once per workgroup (it does not change over time), rows zero-padded to 32 columns
template <typename R> __device__ __forceinline__ void cw2_stage_pot_mat(const FkW<R>& m, Cw2Lds<R>& L, int tid, int nt) {
    const int D = m.D, S = L.S;
    for (int i = tid; i < D * S; i += nt) {
        const int r = i / S, q = i - r * S;
        L.pot_mat[i] = q < D ? m.pot_mat[r * D + q] : (R)0;
    }
}
// sum_k log N(x_k; u_k, s^2) = c_u - sum_k ((x_k - u_k) / s)^2 / 2 of the particle whose component k this lane holds (csmc_sweep.h::guided_weight: component order)
template <typename R> __device__ __forceinline__ R nu_half(int D, int k, R xk, R uk, R inv_s, R c_u) {
    const R z = k < D ? (xk - uk) * inv_s : (R)0;
    R q = 0;
    static_for<0, CSW_MAXD>([&](auto jc) {
        const R zj = half_bcast<R, decltype(jc)::value>(z);
        q = fma_(zj, zj, q);
    });
    return fma_((R)-0.5, q, c_u);
}
// this step's proposal noise into the LDS rows eps[n][k]: natural flat index ((ch T + t) N + n) D + k of stream 2, both normals of every Threefry block used
template <typename R> __device__ __forceinline__ void cw2_draw(const CsmcArgs& a, Cw2Lds<R>& L, int ch, int t, int r, int nr) {
    const int N = a.N, D = L.D, S = L.S, ND = N * D;
    const long long base = (((long long)ch * a.T + t) * N) * D;
    if (a.noise_mode == 0) {
        for (int e = r; e < ND; e += nr) {
            const int n = e / D, k = e - n * D;
            L.eps[n * S + k] = ((const R*)a.eps_prop)[base + e];
        }
        return;
    }
    const long long b0 = base >> 1, b1 = (base + ND - 1) >> 1;
    for (long long blk = b0 + r; blk <= b1; blk += nr) {
        R z0, z1;
        stream_normal2<R>(a.key0, a.key1, STREAM_EPS_PROP, (unsigned long long)blk, z0, z1);
        const long long e0 = 2 * blk - base, e1 = e0 + 1;
        if (e0 >= 0 && e0 < ND) {
            const int n = (int)e0 / D, k = (int)e0 - n * D;
            L.eps[n * S + k] = z0;
        }
        if (e1 >= 0 && e1 < ND) {
            const int n = (int)e1 / D, k = (int)e1 - n * D;
            L.eps[n * S + k] = z1;
        }
    }
}

// GD: the guided proposals, a compile-time variant; false: the kernel as it was, holding none of their code
// V: the potential's variant (csmc_sweep.h::PotV), a compile-time choice in the same way: a coupled potential has its matrix staged in LDS and coupled_half in place of
// the separable sum (potential_half)
template <typename R, int NW2, bool GD = false, PotV V = PotV::SEP> __global__ void __launch_bounds__(64 * NW2) k_cw2_fwd(CsmcArgs a, FkW<R> m) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NT_ = 64 * NW2;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, N = a.N, T = a.T, D = m.D;
    const bool hi = lane >= 32;
    const int k = lane & 31;
    constexpr bool coupled = pot_has_matrix(V);
    Cw2Lds<R> L(smem, D, GD, coupled);
    if constexpr (coupled) cw2_stage_pot_mat<R>(m, L, tid, NT_);  // (published by cw2_stage's barrier)
    cw2_stage<R>(m, L, tid, NT_);
    const int S = L.S, nslot = (N + 2 * NW2 - 1) / (2 * NW2);
    const int ch = a.c0 + blockIdx.x;
    const R* xstar = (const R*)a.x + (long long)ch * T * D;
    const R* uaux = (const R*)a.u + (long long)ch * T * D;
    const bool grad = m.gradient != 0 && (GD || m.proposal == 1), tv = m.Ft != nullptr;  // (guided: a.grad holds the shifted u the proposal mean reads)
    const R* gaux = grad ? (const R*)a.grad + (long long)ch * T * D : uaux;
    const R* yv = (const R*)a.y;
    R* xs = (R*)a.xs + (long long)ch * T * N * D;
    R* lws = (R*)a.lws + (long long)ch * T * N;
    int32_t* As = a.As ? a.As + (long long)ch * (T - 1) * N : nullptr;
    R* fmax = a.fmax ? (R*)a.fmax + (long long)ch * T : nullptr;
    const R* gbp = (const R*)a.gb;
    const bool bmode = gbp != nullptr && !(grad && m.gradient == 2);  // (the exact-gradient correction is unbounded in x: csmc.hip)
    const R ninf = -INFINITY;
    R bk = k < D ? L.b[k] : (R)0;
    const R* Frow = L.F + (k < D ? k : 0) * S;
    const R* Lrow = L.LQ + (k < D ? k : 0) * S;
    // guided: this lane's rows of the staged K_t / chol Lambda_t and its half-wave's row of u~ - pred
    const R* Kgrow = GD ? L.Kg + (k < D ? k : 0) * S : nullptr;
    const R* Lgrow = GD ? L.Lg + (k < D ? k : 0) * S : nullptr;
    R* dvr = GD ? L.dv + (2 * wv + (hi ? 1 : 0)) * S : nullptr;
    const R* Mrow = coupled ? L.pot_mat + (k < D ? k : 0) * S : nullptr;

    // ---- t = 0 (csmc.py:74-80)
    cw2_draw<R>(a, L, ch, 0, tid, NT_);
    if constexpr (GD) cw2_stage_g<R>(guided_at<R>(a.gtab, D, 0), L, tid, NT_);
    __syncthreads();
    for (int s = 0; s < nslot; ++s) {
        const int i = s * 2 * NW2 + 2 * wv + (hi ? 1 : 0);
        const bool pl = i < N;  // (uniform per half-wave)
        const int ir = pl ? i : 0;
        R xk = 0, acc0 = 0, pmk = 0;
        if constexpr (GD) {  // pred = m0, P = P0: x ~ N(m0 + K_0 (u~_0 - m0), Lambda_0)
            const R m0k = k < D ? m.m0[k] : (R)0;
            dvr[k] = k < D ? gaux[k] - m0k : (R)0;
            __builtin_amdgcn_wave_barrier();  // (a half-wave reads back only its own row: ordered inside the wave)
            pmk = m0k;
#pragma unroll
            for (int j = 0; j < CSW_MAXD; ++j) pmk = fma_(Kgrow[j], dvr[j], pmk);
            R acc = pmk;
#pragma unroll
            for (int j = 0; j < CSW_MAXD; ++j) acc = j <= k ? fma_(Lgrow[j], L.eps[ir * S + j], acc) : acc;
            if (k < D) {
                xk = i == 0 ? xstar[k] : acc;
                acc0 = xk - m0k;
            }
        } else if (k < D) {
            if (m.proposal == 0) {
                R acc = m.m0[k];
                for (int j = 0; j <= k; ++j) acc = fma_(m.LP0[k * D + j], L.eps[ir * S + j], acc);
                xk = acc;
            } else {  // AuxiliaryM0: N(u_0 [+ delta_0 / 2 grad_0], delta_0 / 2 I)  (independent.py:143-158)
                const R s0 = ((const R*)a.shd)[0];
                pmk = grad ? fma_(s0 * s0, gaux[k], uaux[k]) : uaux[k];
                xk = fma_(s0, L.eps[ir * S + k], pmk);
            }
            if (i == 0) xk = xstar[k];
            acc0 = xk - m.m0[k];
        }
        const R yk = (yv && k < D) ? yv[k] : (R)0;
        R g;
        if constexpr (V == PotV::LOGI) g = logistic_half<R>(D, k, xk, yk, yv, T, 0);
        else g = potential_half<R, V>(m, k, hi, xk, yk, Mrow);
        if (m.proposal == 1) g = g + gauss_half<R>(D, k, hi, acc0, m.LP0 + (long long)(k < D ? k : 0) * D, k < D ? m.iLP0[k] : (R)0, m.c_init);  // AuxiliaryG0
        if constexpr (GD) {  // log g + log N(x; m0, P0) + sum_k log N(x_k; u_k, s^2) - log N(x; mu, Lambda_0)
            const GuidedT<R> gd = guided_at<R>(a.gtab, D, 0);
            g = g + gauss_half<R>(D, k, hi, acc0, m.LP0 + (long long)(k < D ? k : 0) * D, k < D ? m.iLP0[k] : (R)0, m.c_init);
            g = g + nu_half<R>(D, k, xk, k < D ? uaux[k] : (R)0, gd.inv_s, gd.c_u);
            g = g - gauss_half_blk<R>(D, k, xk - pmk, Lgrow, L.blkg, gd.c_lam);
        } else if (grad) g = g + grad_corr_half<R>(D, k, xk, k < D ? uaux[k] : (R)0, pmk, ((const R*)a.shd)[0]);  // GradientAuxiliaryG0 (:173-190)
        if (pl && k < D) {
            L.xa[i * S + k] = xk;
            xs[(long long)i * D + k] = xk;
        }
        if (pl && k == 0) {
            L.lwv[i] = g;
            lws[i] = g;
        }
    }
    __syncthreads();
    R* xprev = L.xa;
    R* xcur = L.xb;
    for (int t = 1; t < T; ++t) {
        // the step's rows from global memory, requested before the resampling section and its barrier
        const R yk = (yv && k < D) ? yv[(long long)t * D + k] : (R)0;
        const R st = m.proposal != 0 ? ((const R*)a.shd)[t] : (R)0;
        const R uk = (m.proposal != 0 && k < D) ? uaux[(long long)t * D + k] : (R)0;
        const R xsk = k < D ? xstar[(long long)t * D + k] : (R)0;
        const R gk = (grad && k < D) ? gaux[(long long)t * D + k] : (R)0;
        const R ctr = tv ? m.ctt[t - 1] : m.c_trans;  // the transition t - 1 -> t (time-varying: row t - 1)
        if (tv) cw2_stage_t<R>(m, L, t - 1, tid, NT_);  // (the previous step's particle section is behind its barrier)
        R c_lam = 0, c_u = 0, inv_s = 0;
        if constexpr (GD) {
            const GuidedT<R> gd = guided_at<R>(a.gtab, D, t);
            c_lam = gd.c_lam, c_u = gd.c_u, inv_s = gd.inv_s;
            cw2_stage_g<R>(gd, L, tid, NT_);
        }
        if (wv == 0) {
            // weights of step t - 1 and the conditional multinomial resampling (resamplings.py:14-37), one lane per particle
            const bool live = lane < N;
            const R lw = live ? L.lwv[lane] : ninf;
            const int tp = t - 1;
            R Mb = (bmode ? gbp[tp] : (R)0) + (m.proposal == 1 ? (tv && tp >= 1 ? m.ctt[tp - 1] : m.c_trans) : (R)0);
            const bool used_bound = bmode && tp >= 1 && tp < T - 1 && (Mb - Mb == 0);
            R mstep, w;
            if (used_bound) {
                w = det_exp(lw - Mb);
                mstep = Mb;
            } else {
                w = wave_expmax<R>(lw, &mstep);
            }
            R cv = wave_scan_dpp(w);
            R tot = readlane_(cv, 63);
            if (used_bound && !(tot > (R)0)) {  // every weight underflowed under its bound: the exact maximum after all
                w = wave_expmax<R>(lw, &mstep);
                cv = wave_scan_dpp(w);
                tot = readlane_(cv, 63);
            }
            if (fmax && lane == 0) fmax[tp] = mstep;
            L.c[lane] = cv;
            __builtin_amdgcn_wave_barrier();
            const R un = (live && lane > 0) ? noise_uniform<R>(a, a.u_res, STREAM_U_RES, ((long long)ch * (T - 1) + (t - 1)) * N + lane) : (R)0;
            int idx = 0;
            if (live && lane > 0) idx = search_w<R>(L.c, N, tot * ((R)1 - un));
            L.idx[lane] = idx;
            if (live && As) As[(long long)(t - 1) * N + lane] = idx;
            cw2_draw<R>(a, L, ch, t, lane, NT_);  // (its share of the draws: the other waves start with theirs)
        } else {
            cw2_draw<R>(a, L, ch, t, tid, NT_);
        }
        __syncthreads();
        if (tv) bk = k < D ? L.b[k] : (R)0;
        for (int s = 0; s < nslot; ++s) {
            const int i = s * 2 * NW2 + 2 * wv + (hi ? 1 : 0);
            const bool pl = i < N;
            const int ir = pl ? i : 0;
            const R* xp = xprev + L.idx[ir] * S;
            // the parent's transition mean, component k (csmc.py:91-92)
            R mu = bk;
#pragma unroll
            for (int j = 0; j < CSW_MAXD; ++j) mu = fma_(Frow[j], xp[j], mu);  // (columns beyond D are zeros on both sides: fma(0, 0, mu) = mu)
            R xk = 0, pmk = 0;
            if constexpr (GD) {  // x ~ N(mu + K_t (u~_t - mu), Lambda_t): one more row product, the draw as the bootstrap branch has it
                dvr[k] = k < D ? (grad ? gk : uk) - mu : (R)0;
                __builtin_amdgcn_wave_barrier();  // (a half-wave reads back only its own row: ordered inside the wave)
                pmk = mu;
#pragma unroll
                for (int j = 0; j < CSW_MAXD; ++j) pmk = fma_(Kgrow[j], dvr[j], pmk);
                R acc = pmk;
#pragma unroll
                for (int j = 0; j < CSW_MAXD; ++j) acc = j <= k ? fma_(Lgrow[j], L.eps[ir * S + j], acc) : acc;
                if (k < D) xk = i == 0 ? xsk : acc;
            } else if (k < D) {
                if (m.proposal == 0) {
                    R acc = mu;
#pragma unroll
                    for (int j = 0; j < CSW_MAXD; ++j) acc = j <= k ? fma_(Lrow[j], L.eps[ir * S + j], acc) : acc;
                    xk = acc;
                } else {  // AuxiliaryMtDynamics: N(u_t [+ delta_t / 2 grad_t], delta_t / 2 I) (independent.py:192-198)
                    pmk = grad ? fma_(st * st, gk, uk) : uk;
                    xk = fma_(st, L.eps[ir * S + k], pmk);
                }
                if (i == 0) xk = xsk;
            }
            // weights (csmc.py:95-96)
            R g;
            if constexpr (V == PotV::LOGI) g = logistic_half<R>(D, k, xk, yk, yv, T, t);
            else g = potential_half<R, V>(m, k, hi, xk, yk, Mrow);
            if (m.proposal == 1) g = gauss_half_blk<R>(D, k, xk - mu, Lrow, L.blk, ctr) + g;  // AuxiliaryGt = Mt.logpdf + Gt (independent.py:238-248)
            // GradientAuxiliaryGt (:252-268): summed over the particles in the reference, i.e. a constant of the step (AUXSSM_GRAD_REFERENCE: nothing to add);
            // AUXSSM_GRAD_EXACT applies it per particle
            if constexpr (GD) {  // log g + log N(x; pred, Q) + sum_k log N(x_k; u_k, s^2) - log N(x; mu_t, Lambda_t)
                g = g + gauss_half_blk<R>(D, k, xk - mu, Lrow, L.blk, ctr);
                g = g + nu_half<R>(D, k, xk, uk, inv_s, c_u);
                g = g - gauss_half_blk<R>(D, k, xk - pmk, Lgrow, L.blkg, c_lam);
            } else if (grad && m.gradient == 2) g = g + grad_corr_half<R>(D, k, xk, uk, pmk, st);
            if (pl && k < D) {
                xcur[i * S + k] = xk;
                xs[((long long)t * N + i) * D + k] = xk;
            }
            if (pl && k == 0) {
                L.lwv[i] = g;
                lws[(long long)t * N + i] = g;
            }
        }
        __syncthreads();
        R* tmp = xprev;
        xprev = xcur;
        xcur = tmp;
    }
    if (wv == 0) {  // the weights of the last step: exact maximum
        const bool live = lane < N;
        const R lw = live ? L.lwv[lane] : ninf;
        R mstep;
        const R w = wave_expmax<R>(lw, &mstep);
        if (fmax && lane == 0) fmax[T - 1] = mstep;
        if (live) ((R*)a.wT)[(long long)ch * N + lane] = w;
    }
}

template <typename R, int NW2> __global__ void __launch_bounds__(64 * NW2) k_cw2_bwd(CsmcArgs a, FkW<R> m) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NT_ = 64 * NW2;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, N = a.N, T = a.T, D = m.D;
    const bool hi = lane >= 32;
    const int k = lane & 31;
    Cw2Lds<R> L(smem, D);
    cw2_stage<R>(m, L, tid, NT_);
    const int S = L.S, nslot = (N + 2 * NW2 - 1) / (2 * NW2);
    const int ch = a.c0 + blockIdx.x;
    const R* xs = (const R*)a.xs + (long long)ch * T * N * D;
    const R* lws = (const R*)a.lws + (long long)ch * T * N;
    const int32_t* As = a.As ? a.As + (long long)ch * (T - 1) * N : nullptr;
    R* xout = (R*)a.x + (long long)ch * T * D;
    int32_t* anc = a.anc + (long long)ch * T;
    const R* fmax = (const R*)a.fmax + (long long)ch * T;
    const R ninf = -INFINITY;
    const bool tv = m.Ft != nullptr;
    R bk = k < D ? L.b[k] : (R)0;
    const R* Frow = L.F + (k < D ? k : 0) * S;
    const R* Lrow = L.LQ + (k < D ? k : 0) * S;
    // B_T ~ choice(w_T) by wave 0
    if (wv == 0) {
        const bool live = lane < N;
        const R w = live ? ((const R*)a.wT)[(long long)ch * N + lane] : (R)0;
        const R cv = wave_scan_dpp(w);
        const R tot = readlane_(cv, 63);
        const R un = ((const R*)a.u_bwd)[(long long)ch * T + (T - 1)];
        int B = __popcll(__ballot(live && cv < tot * ((R)1 - un)));
        B = B < N - 1 ? B : N - 1;
        if (lane == 0) L.idx[0] = B, anc[T - 1] = B;
    }
    __syncthreads();
    int B = L.idx[0];
    R xn = k < D ? xs[((long long)(T - 1) * N + B) * D + k] : (R)0;  // x_{t+1}, component k (every half-wave holds a copy)
    if (wv == 0 && !hi && k < D) xout[(long long)(T - 1) * D + k] = xn;
    if (!a.backward) {
        if (tid == 0) {
            for (int t = T - 1; t >= 1; --t) {
                B = As[(long long)(t - 1) * N + B];
                for (int q = 0; q < D; ++q) xout[(long long)(t - 1) * D + q] = xs[((long long)(t - 1) * N + B) * D + q];
                anc[t - 1] = B;
            }
        }
        return;
    }
    constexpr int NSL = 64 / (2 * NW2);  // passes at N = 64
    R xi_nx[NSL], lw_nx[NSL];  // the rows of step t, requested one step ahead (they do not depend on the draws)
#pragma unroll
    for (int s = 0; s < NSL; ++s) {
        const int i = s * 2 * NW2 + 2 * wv + (hi ? 1 : 0), ir = i < N ? i : 0;
        xi_nx[s] = (T >= 2 && k < D) ? xs[((long long)(T - 2) * N + ir) * D + k] : (R)0;
        lw_nx[s] = T >= 2 ? lws[(long long)(T - 2) * N + ir] : (R)0;
    }
    for (int t = T - 2; t >= 0; --t) {
        __syncthreads();  // (the draw of the step before has been read by everybody)
        const R ctr = tv ? m.ctt[t] : m.c_trans;  // the transition t -> t + 1 (time-varying: row t)
        if (tv) {
            cw2_stage_t<R>(m, L, t, tid, NT_);
            __syncthreads();
            bk = k < D ? L.b[k] : (R)0;
        }
#pragma unroll
        for (int s = 0; s < NSL; ++s) {
            if (s >= nslot) break;
            const int i = s * 2 * NW2 + 2 * wv + (hi ? 1 : 0);
            const bool pl = i < N;
            const int ir = pl ? i : 0;
            const R xik = xi_nx[s], lwik = lw_nx[s];
            if (t > 0) {
                xi_nx[s] = k < D ? xs[((long long)(t - 1) * N + ir) * D + k] : (R)0;
                lw_nx[s] = lws[(long long)(t - 1) * N + ir];
            }
            if (k < D) L.xa[ir * S + k] = xik;  // (a half-wave reads back only its own row: ordered inside the wave)
            __builtin_amdgcn_wave_barrier();
            const R* xi = L.xa + ir * S;
            R mu = bk;
#pragma unroll
            for (int j = 0; j < CSW_MAXD; ++j) mu = fma_(Frow[j], xi[j], mu);
            const R lwt = gauss_half_blk<R>(D, k, xn - mu, Lrow, L.blk, ctr) + lwik;  // Pt.logpdf(x_{t+1}, xs_t) + log_ws_t (csmc.py:136)
            if (pl && k == 0) L.lwv[i] = lwt;
        }
        __syncthreads();
        if (wv == 0) {
            const bool live = lane < N;
            const R lw = live ? L.lwv[lane] : ninf;
            R Mb = fmax[t] + ctr;
            if (!(Mb - Mb == 0)) Mb = 0;
            R w = det_exp(lw - Mb);
            R cv = wave_scan_dpp(w);
            R tot = readlane_(cv, 63);
            if (!(tot > (R)0)) {
                w = wave_expmax<R>(lw, nullptr);
                cv = wave_scan_dpp(w);
                tot = readlane_(cv, 63);
            }
            const R un = ((const R*)a.u_bwd)[(long long)ch * T + t];
            int Bn = __popcll(__ballot(live && cv < tot * ((R)1 - un)));
            Bn = Bn < N - 1 ? Bn : N - 1;
            if (lane == 0) L.idx[0] = Bn, anc[t] = Bn;
        }
        __syncthreads();
        B = L.idx[0];
        xn = k < D ? L.xa[B * S + k] : (R)0;
        if (wv == 0 && !hi && k < D) xout[(long long)t * D + k] = xn;
    }
}

// The passes of (model, sweep); wide16: fp32 and no more chains than CUs (run_cw); V: the variant of the model's potential (csmc_sweep.h::with_pot).
//   forward   guided                 k_cw2_fwd<R, 8, true, V>                    eight waves whatever the chain count
//             otherwise              k_cw2_fwd<R, wide16 ? 16 : 8, false, V>
//   backward                         k_cw2_bwd<R, wide16 ? 16 : 8>               the base LDS plan (Cw2Lds::bytes)
// The forward pass's LDS is Cw2Lds::fwd_bytes(D, guided, pot_has_matrix(V)): the coupled potentials' matrices share one slot, so neither plan exceeds the other's.
// (guided: under the 128 registers of a 1024-lane workgroup the two extra row products and the second blocked density spill, 360 bytes per lane in fp32:
// 7.47 ms against 5.11 ms per sweep of the SV protocol at 256 chains)
template <typename R> using WideKernel = void (*)(CsmcArgs, FkW<R>);
template <typename R> static WideKernel<R> cw_fwd_kernel(bool guided, int potential, bool wide16) {
    return with_pot(potential, [&](auto pv) -> WideKernel<R> {
        constexpr PotV V = decltype(pv)::value;
        if (guided) return k_cw2_fwd<R, 8, true, V>;
        return wide16 ? k_cw2_fwd<R, 16, false, V> : k_cw2_fwd<R, 8, false, V>;
    });
}
template <typename R> static WideKernel<R> cw_bwd_kernel(bool wide16) { return wide16 ? k_cw2_bwd<R, 16> : k_cw2_bwd<R, 8>; }

// host: the model as one device block [m0 | LP0 | iLP0 | F | b | LQ | iLQ | the matrix of a coupled potential] (csmc_host.h::fk_model, leading dimension D)
template <typename R> int cw_model(auxssm_ctx* h, const auxssm_fk_model* fk, FkW<R>& m) {
    const int D = fk->dx;
    memset(&m, 0, sizeof(m));
    const bool coupled = pot_kind(fk->potential).matrix != nullptr;  // (a potential with a matrix in the block)
    std::vector<R> block((size_t)3 * D * D + 4 * D + (coupled ? (size_t)D * D : 0));
    R* const host_block = block.data();
    R *hm0 = host_block, *hLP0 = hm0 + D, *hiLP0 = hLP0 + D * D, *hF = hiLP0 + D, *hb = hF + D * D, *hLQ = hb + D, *hiLQ = hLQ + D * D, *hpot_mat = hiLQ + D;
    fk_model<R>(fk, m, D, hm0, hLP0, hiLP0, hF, hb, hLQ, hiLQ, hpot_mat);
    const size_t nb = block.size() * sizeof(R);
    {   // the handle's copy of the block: a new upload only when the content differs from the last one (a model that changes between sweeps pays one
        // stream synchronisation -- earlier sweeps may still be reading the old block -- a fixed model none: include/auxssm.h, auxssm_csmc_sweep)
        const int hdr[2] = {(int)sizeof(R), D};
        const bool same = h->cw_dev && h->cw_host.size() == sizeof(hdr) + nb && memcmp(h->cw_host.data(), hdr, sizeof(hdr)) == 0 &&
                          memcmp(h->cw_host.data() + sizeof(hdr), host_block, nb) == 0;
        if (!same) {
            AX_HIP(hipStreamSynchronize(h->stream));
            if (h->cw_dev_bytes < nb) {
                if (h->cw_dev) (void)hipFree(h->cw_dev);
                h->cw_dev = nullptr, h->cw_dev_bytes = 0;
                h->cw_host.clear();
                AX_HIP(hipMalloc(&h->cw_dev, nb));
                h->cw_dev_bytes = nb;
            }
            AX_HIP(hipMemcpy(h->cw_dev, host_block, nb, hipMemcpyHostToDevice));
            h->cw_host.resize(sizeof(hdr) + nb);
            memcpy(h->cw_host.data(), hdr, sizeof(hdr));
            memcpy(h->cw_host.data() + sizeof(hdr), host_block, nb);
        }
    }
    const R* d = (const R*)h->cw_dev;
    m.m0 = d; d += D;
    m.LP0 = d; d += D * D;
    m.iLP0 = d; d += D;
    m.F = d; d += D * D;
    m.b = d; d += D;
    m.LQ = d; d += D * D;
    m.iLQ = d; d += D;
    m.pot_mat = coupled ? d : nullptr;
    return AUXSSM_OK;
}
template int cw_model<float>(auxssm_ctx*, const auxssm_fk_model*, FkW<float>&);
template int cw_model<double>(auxssm_ctx*, const auxssm_fk_model*, FkW<double>&);

template <typename R> static int run_cw(auxssm_ctx* h, const auxssm_fk_model* fk, CsmcArgs& a, void* ctt) {
    const int D = fk->dx;
    FkW<R> m;
    int rc = cw_model<R>(h, fk, m);
    if (rc) return rc;
    const bool coupled = m.pot_mat != nullptr;
    rc = csmc_prologue<R>(h, fk, a, ctt, m, false, [&] {
        cw_grad_launch<R>(h, a, m);
        return AUXSSM_OK;
    });
    if (rc) return rc;
    const bool guided = fk->proposal == AUXSSM_PROP_AUX_GUIDED;
    const int cb = a.cb > 0 ? a.cb : a.C;
    // sixteen waves per chain (every particle of N <= 32 in its own half-wave at once: the shortest step) while the chains leave CUs to spare, eight (no idle
    // waves at N = 25, two passes) once there are more chains than CUs
    const bool wide16 = sizeof(R) == 4 && a.C <= h->num_cu;  // (fp64: the unrolled loops need more than the 128 registers of a 1024-lane workgroup)
    const int fwd_waves = wide16 && !guided ? 16 : 8, bwd_waves = wide16 ? 16 : 8;
    for (int c0 = 0; c0 < a.C; c0 += cb) {
        const CsmcArgs ab = csmc_batch(a, c0, cb);
        {
            ProfScope ps(h, AUXSSM_K_CSMC_FWD);
            if ((rc = launch(h, cw_fwd_kernel<R>(guided, m.potential, wide16), dim3(ab.C), dim3(64 * fwd_waves), Cw2Lds<R>::fwd_bytes(D, guided, coupled), ab, m))) return rc;
        }
        {
            ProfScope ps(h, AUXSSM_K_CSMC_BWD);
            if ((rc = launch(h, cw_bwd_kernel<R>(wide16), dim3(ab.C), dim3(64 * bwd_waves), Cw2Lds<R>::bytes(D), ab, m))) return rc;
        }
    }
    AX_HIP(hipGetLastError());
    return AUXSSM_OK;
}

// called by auxssm_csmc_sweep (csmc.hip) for dx > CS_MAXD
int run_csmc_wide(auxssm_ctx* h, int dtype, const auxssm_fk_model* fk, CsmcArgs& a, void* ctt) {
    if (dtype == AUXSSM_F32) return run_cw<float>(h, fk, a, ctt);
    return run_cw<double>(h, fk, a, ctt);
}

}  // namespace ax
