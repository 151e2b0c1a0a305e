// fused_shared.h -- the chain-shared LG_CONCAT sweep in three streaming passes (round 3; included at the end of kernels.hip.h).
//
// What the chain-shared sweep of affine_shared.h moved per chain and time step (reals of d components; 8.06 GB at C2 / 256 chains, fp64):
//   filter reduce  r x, w eps_aux | filter down r x, r eps_aux, w ms | sampler reduce r ms, w eps_samp | sampler down r ms, r eps_samp, w x'
//   log-density r x, r x', r eps_aux | select r x', w x                                                  = 15 d
// Round 3 (7 d = 3.76 GB): A (r x, w u), C (r u, w inc), E (r inc, r u, w x').  Round 4 (6 d = 3.22 GB): passes A and C are ONE pass --
//   AC (k_fs_ac) r x            w u, inc0  draws eps_aux, u = x + sqrt(delta/2) eps; the MH terms of the CURRENT state x (prior, observation, auxiliary:
//                                         kalman/generic.py:88-89, :103-105); the filter's chunk fold h_t = Mb h_{t-1} + kc + K u_t FROM A ZERO START (the chunk's first
//                                         mean is not known yet), which is at the same time the chunk-LOCAL filtered mean: m_t = h_t + Phi_t m_start with the
//                                         chain-shared prefix product Phi_t of the chunk's Mb (k_fs_fprod); and, in the same walk, the sampler's LOCAL increments
//                                         inc0_t = M1_t h_t - gb_t + Lc_t eps_t (sampling.py:108-112; draws eps_samp) with their chunk aggregate
//                                         e0 = sum_t (G_ta ... G_{t-1}) inc0_t against the table of within-chunk gain products (k_fs_gpre)
//   --  (k_fs_mid)                        one workgroup per chain: m_start of every (chain, chunk) by the aggregate scan of the folds; the sampler's aggregates
//                                         completed by the part that is linear in m_start, e = e0 + Psi_chunk m_start, Psi = sum_t (G_ta ... G_{t-1}) M1_t Phi_t
//                                         (chain-shared, k_fs_psi), and scanned in turn.  Both scans carry the chain's D-vector offsets only: the matrices of the
//                                         aggregates are chain-shared, and the one a Kogge-Stone stage needs comes from a table of the model stage (k_fs_gtab)
//   E  (k_fs_e)  r inc0, r u    w x'      sampler walk (descending) x'_t = G_t x'_{t+1} + inc0_t + N_t m_start, N_t = M1_t Phi_t (in the pass's coefficient row), and the MH
//                                         terms of the PROPOSAL x' where it is in registers
// The filtered means never go to memory, u is written once and read once, and the chain passes are two kernels bound by HBM (AC: 3 d at 615 instructions per
// chain-step; E: 3 d) instead of three.
// FIVE ARRAY PASSES (5 d): u is not stored at all.  AC (r x, w inc0) keeps u in registers for the fold and forms no MH terms; E (r inc0, r x, w x') rebuilds
// u_{t+1} = x_{t+1} + sqrt(delta / 2) eps_aux_{t+1} from the keyed draw (fs_aux_u, the helper pass AC calls: the same bits) and forms the MH terms of BOTH states, x and x',
// from one read of its log-density row (fs_terms_fast2).  Pass AC was short of issue slots and pass E had them idle.
// plus the kernel between them (k_fs_mid: the values of k_aff_aggs' scans bit for bit), one lane per chain for the t = 0 terms (k_fs_head) and the accept step (k_fs_accept).
// There is no select pass: with a `sel` array the state is LAZY -- chain c lives in buffer sel[c] of a ping-pong pair, reads its x from there, writes
// its proposal to the other buffer, and acceptance flips sel[c] (auxssm_kalman_sweep_lazy); without one, x' goes to a scratch buffer and the
// caller runs the usual select.  Same tables as affine_shared.h / kalman_bodies.h (GainRow, SampShared, LogShared), same per-term arithmetic and NaN
// policy as FilterMeanOp / SampleAffOp / body_sweep_logpdf_shared; the per-chain totals are summed per (chain, chunk) lane and then over chunks, so
// they agree with the unfused path to rounding, not bitwise (tests/test_gpu_fused.py: 1e-9 relative on x', 1e-7 absolute on log alpha at C2 size, on the
// benchmark's model; tests/test_gpu_fused_models.py: the same bars against the oracle and the keyed sweep on time-varying models with dy != dx, missing data under
// both NaN policies, rejected chains and a non-finite chain in the wave, for every (D, PO)).
#pragma once
// (included inside namespace ax by kernels.hip.h)
#include "fs_chunk.h"  // the chunk rule: a plain integer function, also checked on the CPU (tests/test_fused_chunk_host.py)

struct FusedArgs {
    int C, T, E, nchunk;
    const void* xa;      // (T, D, C) chain-minor; chain c reads its state from xa (sel null or sel[c] == 0) or xb,
    void* xb;            //                         and writes its proposal to the other one
    const int32_t* sel;
    void* u;             // (D, C): u_0, written by the caller (the t = 0 terms; fs_dropped_joint).  u_t, t >= 1, is never stored: see k_fs_e
    void* inc;           // (T, D, C)
    const void* gain;    // n rows GainRow<R, D, P>      (transition i -> i + 1)
    const void* samp;    // T rows SampShared<R, D>
    const void* logt;    // n rows LogShared<R, D, PO>
    const void* gpre;    // T rows D*D: product of the sampler gains of the chunk's earlier steps, G_ta ... G_{t-1} (I at the chunk's first step)
    const void* m0p;     // (D, C): filtered mean at t = 0
    void* agg_f; void* pre_f; void* agg_s; void* pre_s;  // chunk aggregates / exclusive prefixes of the two scans (k_aff_aggs layout)
    Acc* pa;             // (3, C, nchunk): sums over the chunk of [q(x | u) terms, target(x) terms, |x - u|^2 / delta]
    Acc* pe;             // (3, C, nchunk): the same of x'
    void* pell;          // (C, nchunk) -1/2 sum |eps_samp|^2 of the chunk: the data part of log q(x' | u) (R)
    const Acc* clog;     // sum_t (sum_i log Lc_t[i][i] + D/2 log 2 pi): the chain-shared part of log q(x' | u) (k_fs_clog, model stage)
    const int* nanrow;   // != 0: some log-density row is not finite, i.e. (reference policy) an observation is missing and the nansum rule drops that step (k_fs_rows, model stage)
    unsigned ka0, ka1, ks0, ks1;  // keys of eps_aux / eps_samp (stream 0 of auxssm_rng_normal at the (T, D, C) flat index)
    const void* eps0s;   // (D, C): row 0 of eps_samp (fill kernel)
    double delta, shd;
    const double* dptr;  // device-resident {delta, sqrt(delta / 2)} or null
    int nan_policy;
    const int* memo;     // model-stage memo (FilterArgs::memo): the stage kernels return at once when *memo == 0
    int pack, cp;        // few chains (PK instantiations of the two chain passes): one wave walks `pack` consecutive chunks side by side, lane = sub * cp + chain, cp = the
                         // chain count rounded up to a power of two; 1 / 0 otherwise
};
AX_HD void fs_resolve(FusedArgs& a) {
    const double* p = a.dptr;
    a.dptr = nullptr;
    if (p) a.delta = p[0], a.shd = p[1];
}

// the chunk [ch E, (ch + 1) E) of time steps and the (chain, chunk) lane: same block-id swizzle as the affine passes
__device__ __forceinline__ bool fs_decode(const FusedArgs& a, int& ch, int& s) { return decode_aff(a.C, a.nchunk, ch, s); }

// ---- model stage: chunk products of the filter's matrices; within-chunk prefix products + chunk products of the sampler's gains ------------
template <typename R, int D, int P> __global__ void __launch_bounds__(TB_CM) k_fs_fprod(FusedArgs a, R* __restrict__ cprod, R* __restrict__ fpre) {
    if (memo_skip(a)) return;
    using TG = GainRow<R, D, P>;
    const int ch = blockIdx.x * TB_CM + threadIdx.x;
    if (ch >= a.nchunk) return;
    const int t0 = ch * a.E, ta = max(1, t0), tb = min(a.T, t0 + a.E);
    R M[D * D];
#pragma unroll
    for (int k = 0; k < D * D; ++k) M[k] = (k / D == k % D) ? (R)1 : (R)0;
    if (ch == 0) {
#pragma unroll
        for (int k = 0; k < D * D; ++k) fpre[k] = 0;  // t = 0
    }
    for (int t = ta; t < tb; ++t) {
        const R* row = (const R*)a.gain + (long long)(t - 1) * TG::NPAD;
        R G[D * D], o[D * D];
#pragma unroll
        for (int k = 0; k < D * D; ++k) G[k] = row[TG::oM + k];
        mm<R, D, D, D>(G, M, o);
#pragma unroll
        for (int k = 0; k < D * D; ++k) M[k] = o[k];
        // Phi_t = Mb_{t-1} ... Mb_{ta-1}: what the chunk's (unknown) first mean contributes to the mean at t.  Chunk 0 starts from the true m_0: nothing to add.
#pragma unroll
        for (int k = 0; k < D * D; ++k) fpre[(long long)t * D * D + k] = ch == 0 ? (R)0 : M[k];
    }
#pragma unroll
    for (int k = 0; k < D * D; ++k) cprod[(long long)ch * D * D + k] = M[k];
}
template <typename R, int D> __global__ void __launch_bounds__(TB_CM) k_fs_gpre(FusedArgs a, R* __restrict__ gpre, R* __restrict__ cprod) {
    if (memo_skip(a)) return;  // (k_fs_psi below completes the chain-shared tables)
    using TS = SampShared<R, D>;
    const int ch = blockIdx.x * TB_CM + threadIdx.x;
    if (ch >= a.nchunk) return;
    const int ta = ch * a.E, tb = min(a.T, (ch + 1) * a.E);
    R M[D * D];
#pragma unroll
    for (int k = 0; k < D * D; ++k) M[k] = (k / D == k % D) ? (R)1 : (R)0;
    for (int t = ta; t < tb; ++t) {
#pragma unroll
        for (int k = 0; k < D * D; ++k) gpre[(long long)t * D * D + k] = M[k];
        const R* row = (const R*)a.samp + (long long)t * TS::NPAD;
        R G[D * D], o[D * D];
#pragma unroll
        for (int k = 0; k < D * D; ++k) G[k] = row[TS::oG + k];
        mm<R, D, D, D>(M, G, o);  // (G_ta ... G_{t-1}) G_t
#pragma unroll
        for (int k = 0; k < D * D; ++k) M[k] = o[k];
    }
    // scan position of the sampler = reversed time: chunk ch is aggregate nchunk - 1 - ch
#pragma unroll
    for (int k = 0; k < D * D; ++k) cprod[(long long)(a.nchunk - 1 - ch) * D * D + k] = M[k];
}

// N_t = M1_t Phi_t (the sampler increment's dependence on the chunk's first mean) and Psi_chunk = sum_t (G_ta ... G_{t-1}) N_t (the same for the sampler's chunk aggregate)
template <typename R, int D> __global__ void __launch_bounds__(TB_CM) k_fs_psi(FusedArgs a, const R* __restrict__ gpre, const R* __restrict__ fpre, R* __restrict__ ntab,
                                                                              R* __restrict__ psi) {
    if (memo_skip(a)) return;
    using TS = SampShared<R, D>;
    const int ch = blockIdx.x * TB_CM + threadIdx.x;
    if (ch >= a.nchunk) return;
    const int t0 = ch * a.E, tb = min(a.T, t0 + a.E);
    R Ps[D * D];
#pragma unroll
    for (int k = 0; k < D * D; ++k) Ps[k] = 0;
    for (int t = t0; t < tb; ++t) {
        const R* row = (const R*)a.samp + (long long)t * TS::NPAD;
        R M1[D * D], Ph[D * D], Gp[D * D], Nt[D * D], o[D * D];
#pragma unroll
        for (int k = 0; k < D * D; ++k) M1[k] = row[TS::oM + k], Ph[k] = fpre[(long long)t * D * D + k], Gp[k] = gpre[(long long)t * D * D + k];
        mm<R, D, D, D>(M1, Ph, Nt);
        mm<R, D, D, D>(Gp, Nt, o);
#pragma unroll
        for (int k = 0; k < D * D; ++k) ntab[(long long)t * D * D + k] = Nt[k], Ps[k] += o[k];
    }
#pragma unroll
    for (int k = 0; k < D * D; ++k) psi[(long long)ch * D * D + k] = Ps[k];
}
// ---- between the passes: the two aggregate scans of a chain in ONE workgroup, offsets only ------------------------------------------------------------------
// The aggregate of (chain, chunk) is the affine map (G_chunk, e): G_chunk is chain-shared (cprod), only e is the chain's.  k_aff_aggs (kernels.hip.h) scans
// the full elements, so every chain's workgroup repeats the same chain of matrix products.  The only matrix the offset half of a combine reads is the RIGHT
// operand's, o.e = G_right e_left + e_right (kalman_math.h::sample_offset): in the serial and down phases that is cprod[j]; in Kogge-Stone stage s it is the lane's
// own accumulated matrix as it stands at the start of the stage, which depends on the model alone.  k_fs_gtab (model stage, memoised with cprod) runs k_aff_aggs'
// schedule on the matrices -- the same mm calls in the same operand order -- and records that matrix per (stage, lane); k_fs_mid scans D reals per record with
// the matrix from the table: every offset is produced by the same multiply-adds on the same inputs as k_aff_aggs produces it (tests/test_fused_mid_host.py).
// LANE-MINOR TABLES.  A lane owns E2 consecutive chunks, so at step i of its serial walk the lanes of a wave read records E2 records apart: with cprod's
// record layout every 16-byte load instruction of a wave touches 64 different cache lines, and the kernel is bound by the address rate of the CU's one texture
// path, not by latency (measured: 100 us with record-layout tables against 92 us for the three launches it replaces).  k_fs_gtab therefore also lays the
// matrices the serial and down phases read (cprod[j], and Psi of the sampler's scan) out the way the lanes walk them: element k of step i for all 256 lanes side
// by side, tab[(i D^2 + k) 256 + lane] -- a wave's load is 512 contiguous bytes.  Same values; only where they are read from differs.
constexpr int FS_MID_STAGES = 8;
static_assert((1 << FS_MID_STAGES) == TB_AGGS, "one table row per Kogge-Stone stage of the aggregate scan");
// reals of the three tables of one scan: stage matrices | the lanes' serial matrices | (sampler's scan) the lanes' Psi
template <int D> AX_HD size_t fs_mid_ks_reals() { return (size_t)FS_MID_STAGES * D * D * TB_AGGS; }
template <int D> AX_HD size_t fs_mid_ser_reals(int nchunk) { return (size_t)((nchunk + TB_AGGS - 1) / TB_AGGS) * D * D * TB_AGGS; }
// psi: null for the filter's scan; scan position j of the sampler is chunk nchunk - 1 - j
template <typename R, int D>
__global__ void __launch_bounds__(TB_AGGS) k_fs_gtab(FusedArgs a, const R* __restrict__ cprod, const R* __restrict__ psi, R* __restrict__ gks, R* __restrict__ gser,
                                                     R* __restrict__ pser) {
    if (memo_skip(a)) return;
    constexpr int DD = D * D;
    __shared__ R sh[TB_AGGS * DD];
    const int tid = threadIdx.x, nchunk = a.nchunk;
    const int E2 = (nchunk + TB_AGGS - 1) / TB_AGGS;
    const int j0 = min(nchunk, tid * E2), j1 = min(nchunk, j0 + E2);
    for (int i = 0; i < E2; ++i) {  // (slots past the lane's range are never read: zeros)
        const int j = j0 + i;
#pragma unroll
        for (int k = 0; k < DD; ++k) {
            gser[((long long)i * DD + k) * TB_AGGS + tid] = j < j1 ? cprod[(long long)j * DD + k] : (R)0;
            if (psi) pser[((long long)i * DD + k) * TB_AGGS + tid] = j < j1 ? psi[(long long)(nchunk - 1 - j) * DD + k] : (R)0;
        }
    }
    R G[DD];
#pragma unroll
    for (int k = 0; k < DD; ++k) G[k] = (k / D == k % D) ? (R)1 : (R)0;
    if (j0 < j1) ld<R, DD>(cprod + (long long)j0 * DD, G);
    for (int j = j0 + 1; j < j1; ++j) {
        R e[DD], o[DD];
        ld<R, DD>(cprod + (long long)j * DD, e);
        mm<R, D, D, D>(e, G, o);  // sample_combine(acc, e)
#pragma unroll
        for (int k = 0; k < DD; ++k) G[k] = o[k];
    }
    for (int s = 0; s < FS_MID_STAGES; ++s) {
        const int off = 1 << s;
#pragma unroll
        for (int k = 0; k < DD; ++k) gks[((long long)s * DD + k) * TB_AGGS + tid] = G[k];
        st<R, DD>(sh + tid * DD, G);
        __syncthreads();
        R L[DD];
        if (tid >= off) ld<R, DD>(sh + (tid - off) * DD, L);
        __syncthreads();
        if (tid >= off) {
            R o[DD];
            mm<R, D, D, D>(G, L, o);  // sample_combine(left, acc)
#pragma unroll
            for (int k = 0; k < DD; ++k) G[k] = o[k];
        }
    }
}
// one scan of k_fs_mid: the aggregates agg[j] of the workgroup's chain -> their exclusive prefixes pre[j], with k_aff_aggs' lane ranges, phases and association
// order.  FIX (the sampler's scan; position j = chunk nchunk - 1 - j): an aggregate is completed on load by the part linear in the chunk's first mean,
// e += Psi_ch m_start(ch) (Psi_0 = 0; m_start = the first scan's prefixes, which this workgroup has just written) -- wherever it is loaded, with the same loop.
// A lane's loads do not depend on its running offset: the records of a block of NR chunks are fetched side by side (every load unconditional, at a clamped
// index: a load under a lane's condition costs a branch and a full wait each), then folded in order; with at most NR chunks per lane (nchunk <= 2048) the down
// phase finds the serial phase's records still in registers and reloads only the chain-shared matrices.
template <typename R, int D, bool FIX>
__device__ __forceinline__ void fs_mid_scan(R* lds, int nchunk, const R* agg, R* pre, const R* __restrict__ gks, const R* __restrict__ gser,
                                            const R* __restrict__ pser, const R* mst) {
    using Pre = SampPre<R, D>;
    constexpr int DD = D * D, NR = 8, NG = 4;
    const int tid = threadIdx.x;
    const int E2 = (nchunk + TB_AGGS - 1) / TB_AGGS;
    const int j0 = min(nchunk, tid * E2), j1 = min(nchunk, j0 + E2), jlast = j1 - 1;
    auto ldmat = [&](const R* tab, int i, R* G) {  // lane-minor table: row i, this lane's matrix
#pragma unroll
        for (int k = 0; k < DD; ++k) G[k] = tab[((long long)i * DD + k) * TB_AGGS + tid];
    };
    R e[NR][D];
    auto load_block = [&](int jb) {  // e[q] = the (completed) aggregate of chunk min(jb + q, jlast)
        if constexpr (FIX) {
#pragma unroll
            for (int h = 0; h < NR; h += NG) {
                R m[NG][D], Ps[NG][DD];
#pragma unroll
                for (int q = 0; q < NG; ++q) {
                    const int j = min(jb + h + q, jlast);
                    ldv<R, D>(agg + (long long)j * Pre::NPAD, e[h + q]);
                    ldv<R, D>(mst + (long long)(nchunk - 1 - j) * Pre::NPAD, m[q]);
                    ldmat(pser, j - j0, Ps[q]);
                }
#pragma unroll
                for (int q = 0; q < NG; ++q) {
                    const bool fix = nchunk - 1 - min(jb + h + q, jlast) != 0;
#pragma unroll
                    for (int i = 0; i < D; ++i) {
                        R v = e[h + q][i];
#pragma unroll
                        for (int k = 0; k < D; ++k) v += Ps[q][i * D + k] * m[q][k];
                        e[h + q][i] = fix ? v : e[h + q][i];
                    }
                }
            }
        } else {
#pragma unroll
            for (int q = 0; q < NR; ++q) ldv<R, D>(agg + (long long)min(jb + q, jlast) * Pre::NPAD, e[q]);
        }
    };
    R acc[D];
#pragma unroll
    for (int i = 0; i < D; ++i) acc[i] = 0;
    for (int jb = j0; jb < j1; jb += NR) {
        load_block(jb);
#pragma unroll
        for (int h = 0; h < NR; h += NG) {
            R G[NG][DD];
#pragma unroll
            for (int q = 0; q < NG; ++q) ldmat(gser, min(jb + h + q, jlast) - j0, G[q]);
#pragma unroll
            for (int q = 0; q < NG; ++q) {
                const int j = jb + h + q;
                if (j < j1) {
                    R o[D];
                    sample_offset<R, D>(G[q], acc, e[h + q], o);  // sample_combine(acc, e)
#pragma unroll
                    for (int i = 0; i < D; ++i) acc[i] = j == j0 ? e[h + q][i] : o[i];  // (the lane's first chunk is taken as it is)
                }
            }
        }
    }
    R Gs[DD];
    ldmat(gks, 0, Gs);
#pragma unroll
    for (int s = 0; s < FS_MID_STAGES; ++s) {  // Kogge-Stone inclusive scan of the per-lane totals
        const int off = 1 << s;
        R Gn[DD];
        ldmat(gks, s + 1 < FS_MID_STAGES ? s + 1 : s, Gn);  // (the next stage's matrix)
        stv<R, D>(lds + tid * Pre::NPAD, acc);
        __syncthreads();
        R left[D];
        ldv<R, D>(lds + max(tid - off, 0) * Pre::NPAD, left);
        __syncthreads();
        R o[D];
        sample_offset<R, D>(Gs, left, acc, o);  // sample_combine(left, acc)
#pragma unroll
        for (int i = 0; i < D; ++i) acc[i] = tid >= off ? o[i] : acc[i];
#pragma unroll
        for (int k = 0; k < DD; ++k) Gs[k] = Gn[k];
    }
    stv<R, D>(lds + tid * Pre::NPAD, acc);
    __syncthreads();
    R p[D];
    ldv<R, D>(lds + max(tid - 1, 0) * Pre::NPAD, p);
#pragma unroll
    for (int i = 0; i < D; ++i) p[i] = tid > 0 ? p[i] : (R)0;
    for (int jb = j0; jb < j1; jb += NR) {
        if (E2 > NR) load_block(jb);  // (else: the one block of the serial phase)
#pragma unroll
        for (int h = 0; h < NR; h += NG) {
            R G[NG][DD];
#pragma unroll
            for (int q = 0; q < NG; ++q) ldmat(gser, min(jb + h + q, jlast) - j0, G[q]);
#pragma unroll
            for (int q = 0; q < NG; ++q) {
                const int j = jb + h + q;
                if (j < j1) {
                    stv<R, D>(pre + (long long)j * Pre::NPAD, p);
                    R o[D];
                    sample_offset<R, D>(G[q], p, e[h + q], o);  // sample_apply(p, e): the last chunk's result is not used
#pragma unroll
                    for (int i = 0; i < D; ++i) p[i] = o[i];
                }
            }
        }
    }
}
// One workgroup per chain, TB_AGGS lanes.  Scan 1: the folds' aggregates -> the first filtered mean of every chunk (pre_f; pass E reads it too).  Barrier: the
// chain's pre_f records are this workgroup's own stores.  Scan 2: the sampler's aggregates, completed on load by Psi m_start -> the sampler's chunk starts (pre_s).
// No lane leaves before the last barrier and no loop waits for another workgroup: any nchunk >= 1 terminates.
template <typename R, int D>
__global__ void __launch_bounds__(TB_AGGS) k_fs_mid(FusedArgs a, const R* __restrict__ gtab_f, const R* __restrict__ gtab_s) {
    using Pre = SampPre<R, D>;
    __shared__ __attribute__((aligned(16))) R lds[TB_AGGS * Pre::NPAD];
    const long long base = (long long)blockIdx.x * a.nchunk * Pre::NPAD;
    R* pre_f = (R*)a.pre_f + base;
    const size_t nks = fs_mid_ks_reals<D>(), nser = fs_mid_ser_reals<D>(a.nchunk);  // [stage matrices | serial matrices | Psi] of each scan (k_fs_gtab)
    fs_mid_scan<R, D, false>(lds, a.nchunk, (const R*)a.agg_f + base, pre_f, gtab_f, gtab_f + nks, nullptr, nullptr);
    __syncthreads();  // pre_f of this chain is complete and visible to the workgroup; the LDS records of scan 1 are dead
    fs_mid_scan<R, D, true>(lds, a.nchunk, (const R*)a.agg_s + base, (R*)a.pre_s + base, gtab_s, gtab_s + nks, gtab_s + nks + nser, pre_f);
}

// ---- compact per-pass rows (model stage) ----------------------------------------------------------------------------------------------------
// The passes wait for their chain-shared coefficients more than they compute: read straight from the tables with scalar loads every chunk streams ~1 KB
// of rows per step through the scalar cache with no reuse, i.e. a dozen dependent L2 round trips per step (measured: pass C 0.92 ms against a VALU
// floor of 0.28).  So each pass gets its OWN row per time step, holding exactly what it reads, and a workgroup (all its chains x one chunk) copies the
// chunk's rows into LDS with one burst of coalesced loads; inside the time loop a coefficient is an LDS broadcast read.
template <typename R, int D, int PO> struct FsRows {
    static constexpr int P = D + PO;
    using TL = LogShared<R, D, PO>;
    static constexpr int VEC = 16 / sizeof(R);
    static constexpr int pad(int n) { return (n + VEC - 1) / VEC * VEC; }
    // pass AC, row t (t >= 0): [Mb | kc | K[:, :D] of transition t - 1 -> t | M1_t | gb_t | Lc_t (lower, packed) | gpre_t]; the filter part of row 0 is zero
    // (no transition into t = 0).  The pass forms no MH terms, so it carries no log-density row.
    static constexpr int cM = 0, cKc = D * D, cK = cKc + D, cM1 = cK + D * D, cGb = cM1 + D * D, cL = cGb + D, cGp = cL + symsize(D), NC = pad(cGp + D * D);
    // pass E, row t: [G_t | N_t = M1_t Phi_t | LogShared row t (transition t -> t + 1, observation at t + 1; zero for t = T - 1)]: the one log-density row serves
    // the terms of both states, x and x'
    static constexpr int eG = 0, eN = D * D, eL = 2 * D * D, NE = pad(eL + TL::N);
};
// where element k of a compact row comes from: {table (0 gain row t - 1, 1 sampler row t, 3 gpre row t, 4 log-density row t, 5 N row t, -1 zero), offset}.  Evaluated per element by one thread, so that consecutive threads write consecutive reals of the destination rows.
struct FsSrc { int tab, off; };
template <typename R, int D, int PO> __device__ __forceinline__ FsSrc fs_src_c(int k) {
    constexpr int P = D + PO;
    using F = FsRows<R, D, PO>; using TG = GainRow<R, D, P>; using TS = SampShared<R, D>;
    if (k < F::cKc) return {0, TG::oM + k};
    if (k < F::cK) return {0, TG::oKc + (k - F::cKc)};
    if (k < F::cM1) { const int q = k - F::cK; return {0, TG::oK + (q / D) * P + (q % D)}; }
    if (k < F::cGb) return {1, TS::oM + (k - F::cM1)};
    if (k < F::cL) return {1, TS::oGb + (k - F::cGb)};
    if (k < F::cGp) {  // packed lower index -> (i, j) of the dense D x D factor
        const int q = k - F::cL;
        int i = 0;
        while (lidx(i + 1, 0) <= q) ++i;
        return {1, TS::oL + i * D + (q - lidx(i, 0))};
    }
    if (k < F::cGp + D * D) return {3, k - F::cGp};
    return {-1, 0};
}
template <typename R, int D, int PO> __device__ __forceinline__ FsSrc fs_src_e(int k) {
    using F = FsRows<R, D, PO>; using TS = SampShared<R, D>; using TL = LogShared<R, D, PO>;
    if (k < F::eN) return {1, TS::oG + k};
    if (k < F::eL) return {5, k - F::eN};
    if (k < F::eL + TL::N) return {4, k - F::eL};
    return {-1, 0};
}
// one thread per destination element: blockIdx.y picks the row family (0 AC, 1 E), the flat index runs over (t, k)
template <typename R, int D, int PO> __global__ void __launch_bounds__(256) k_fs_rows(FusedArgs a, const R* __restrict__ ntab, R* __restrict__ rc, R* __restrict__ re,
                                                                                      int* __restrict__ nanrow) {
    if (memo_skip(a)) return;
    constexpr int P = D + PO;
    using F = FsRows<R, D, PO>; using TG = GainRow<R, D, P>; using TS = SampShared<R, D>; using TL = LogShared<R, D, PO>;
    const int fam = blockIdx.y;
    const int N = fam == 0 ? F::NC : F::NE;
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= (long long)a.T * N) return;
    const int t = (int)(g / N), k = (int)(g % N);
    const FsSrc sc = fam == 0 ? fs_src_c<R, D, PO>(k) : fs_src_e<R, D, PO>(k);
    R v = 0;
    if (sc.tab == 0) { if (t >= 1) v = ((const R*)a.gain)[(long long)(t - 1) * TG::NPAD + sc.off]; }
    else if (sc.tab == 1) v = ((const R*)a.samp)[(long long)t * TS::NPAD + sc.off];
    else if (sc.tab == 3) v = ((const R*)a.gpre)[(long long)t * D * D + sc.off];
    else if (sc.tab == 4) { if (t + 1 < a.T) v = ((const R*)a.logt)[(long long)t * TL::NPAD + sc.off]; }
    else if (sc.tab == 5) v = ntab[(long long)t * D * D + sc.off];
    (fam == 0 ? rc : re)[g] = v;
    if (sc.tab == 4 && !finite_(v)) *nanrow = 1;  // (every writer stores the same value; zeroed by k_fs_clog_sum, earlier on the stream)
}

// the chain-shared part of log q(x' | u): x'_t | x'_{t+1} = G_t x'_{t+1} + M1_t m_t - gb_t + Lc_t eps_t, so log q = sum_t (-1/2 |eps_t|^2 - sum_i log Lc_t[i][i] - D/2 log 2 pi).
// Two launches with a fixed shape (one lane per time step, a tree per workgroup, then one workgroup over the partial sums): deterministic, and a few microseconds
// on the model stage's chain of dependent launches (one workgroup walking all T steps took 0.6 ms there and made the stage the critical path).
template <typename R, int D> __global__ void __launch_bounds__(256) k_fs_clog_part(int T, const R* __restrict__ samp, Acc* __restrict__ part, const int* memo) {
    if (memo_skip_p(memo)) return;
    using TS = SampShared<R, D>;
    __shared__ Acc sh[256];
    const int t = blockIdx.x * 256 + threadIdx.x;
    R s = 0;
    if (t < T) {
        const R* row = samp + (long long)t * TS::NPAD;
#pragma unroll
        for (int i = 0; i < D; ++i) s += log_(row[TS::oL + i * D + i]);
    }
    sh[threadIdx.x] = (Acc)s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = sh[0];
}
template <int D> __global__ void __launch_bounds__(256) k_fs_clog_sum(int T, int nb, const Acc* __restrict__ part, Acc* __restrict__ out, int* __restrict__ nanrow,
                                                                      const int* memo) {
    if (memo_skip_p(memo)) return;
    if (threadIdx.x == 0) *nanrow = 0;  // (k_fs_rows, later on the stream, raises it)
    __shared__ Acc sh[256];
    Acc acc = 0;
    for (int b = threadIdx.x; b < nb; b += 256) acc += part[b];
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = sh[0] + (Acc)T * (Acc)D * (Acc)(0.5 * LOG_2PI);
}

// workgroup = all (up to 256) chains of one chunk; consecutive blocks = the chain groups of one chunk; the chunks in ascending order of the block index, or (down)
// from the last one
__device__ __forceinline__ void fs_block(const FusedArgs& a, int& ch, int& c, bool down = false) {
    const int groups = (a.C + (int)blockDim.x - 1) / (int)blockDim.x;
    const int q = blockIdx.x / groups;
    ch = down ? a.nchunk - 1 - q : q;
    c = (blockIdx.x % groups) * blockDim.x + threadIdx.x;
}
// copy rows [r0, r1) of a table with rows of N reals into LDS (N a multiple of 16 bytes): one burst of coalesced 16-byte loads
template <typename R, int N> __device__ __forceinline__ void fs_stage(const R* __restrict__ tab, int r0, int r1, R* __restrict__ lds) {
    using V = typename Vec16<R>::type;
    constexpr int W = Vec16<R>::W;
    const V* src = reinterpret_cast<const V*>(tab + (long long)r0 * N);
    V* dst = reinterpret_cast<V*>(lds);
    const int n = (r1 - r0) * (N / W), B = blockDim.x;
    // four loads in flight per trip (one load -> wait -> LDS write per trip left a one-wave workgroup a dozen serial memory latencies before its first step)
    for (int i = threadIdx.x; i < n; i += 4 * B) {
        const bool p1 = i + B < n, p2 = i + 2 * B < n, p3 = i + 3 * B < n;
        const V v0 = src[i], v1 = p1 ? src[i + B] : V{}, v2 = p2 ? src[i + 2 * B] : V{}, v3 = p3 ? src[i + 3 * B] : V{};
        dst[i] = v0;
        if (p1) dst[i + B] = v1;
        if (p2) dst[i + 2 * B] = v2;
        if (p3) dst[i + 3 * B] = v3;
    }
    __syncthreads();
}

// packed form (few chains): rows [r0, r1) = `pack` consecutive chunks of E rows, each chunk's block shifted by one 16-byte slot more than the one before it -- the lanes
// of different chunks read the SAME row offset of their own block at the same time, and E N reals is a multiple of the bank count, so without the shift every read
// would be a `pack`-way bank conflict
template <typename R, int N> __device__ __forceinline__ void fs_stage_pk(const R* __restrict__ tab, int r0, int r1, int E, R* __restrict__ lds) {
    using V = typename Vec16<R>::type;
    constexpr int W = Vec16<R>::W, NV = N / W;
    const V* src = reinterpret_cast<const V*>(tab + (long long)r0 * N);
    V* dst = reinterpret_cast<V*>(lds);
    const int n = (r1 - r0) * NV, B = blockDim.x;
    for (int i = threadIdx.x; i < n; i += 8 * B) {   // eight loads in flight per trip
        V v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = i + q * B < n ? src[i + q * B] : V{};
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if (i + q * B < n) dst[i + q * B + ((i + q * B) / NV) / E] = v[q];
    }
    __syncthreads();
}
template <typename R, int N> AX_HD size_t fs_pk_block(int E) { return (size_t)E * N + Vec16<R>::W; }  // reals per chunk block in LDS (packed form)

// the tables of the fp64 normal transform (rng.h) in the workgroup's LDS, behind the pass's coefficient rows; the barrier of fs_stage publishes them.
// fp32 draws use the hardware functions: no table, no LDS.
template <typename R> struct FsNormTabSel { using type = NormTabGlobal; static constexpr size_t BYTES = 0; };
template <> struct FsNormTabSel<double> { using type = NormTabLds; static constexpr size_t BYTES = (size_t)RNG_TAB_DOUBLES * sizeof(double); };
template <typename R> using FsNormTab = typename FsNormTabSel<R>::type;
template <typename R> __device__ __forceinline__ FsNormTab<R> fs_stage_normtab(R* behind_rows) {
    if constexpr (sizeof(R) == 8) {
        NormTabLds::stage((double*)behind_rows, false);
        return NormTabLds{(const double*)behind_rows};
    } else {
        return NormTabGlobal{};
    }
}

// the MH terms of one state v at time t = i + 1 given the state w at time t - 1 (v, w = x or x'), LogShared row i (`row`, in LDS) -- the per-state
// half of body_sweep_logpdf_shared, same operations: [q-term (concatenated likelihood + prior), target term (likelihood + prior), |v - u|^2 / delta]
template <typename R, int D, int PO>
__device__ __forceinline__ void fs_terms(const FusedArgs& a, const R* row, const R* v, const R* w, const R* u, R inv_delta, R cst, R* out3) {
    using TL = LogShared<R, D, PO>;
    R ob;
    bool badobs = false;
    {
        R q = 0;
#pragma unroll
        for (int k = 0; k < PO; ++k) {
            R z = row[TL::oYw + k];
#pragma unroll
            for (int j = 0; j < D; ++j) z -= row[TL::oWH + k * D + j] * v[j];
            badobs = badobs || !finite_(z);
            q += z * z;
        }
        ob = (R)-0.5 * q + row[TL::oCR];
        if (badobs || isnan_(ob)) ob = 0;
    }
    asm volatile("" ::: "memory");  // (the three blocks read disjoint parts of the row: keep their LDS reads apart)
    R ax, qa = 0;
    bool b = false;
    {
#pragma unroll
        for (int k = 0; k < D; ++k) {
            const R d = u[k] - v[k];
            b = b || !finite_(d);
            qa += d * d;
        }
        ax = b ? (R)0 : -qa * inv_delta + cst;
    }
    const R cc = (a.nan_policy == 0 && (b || badobs)) ? (R)0 : ax + ob;
    asm volatile("" ::: "memory");
    R pr;
    {
        R q = 0;
        bool bad = false;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            R z = -row[TL::oWb + k];
#pragma unroll
            for (int l = 0; l <= k; ++l) z += row[TL::oWQ + lidx(k, l)] * v[l];
#pragma unroll
            for (int j = 0; j < D; ++j) z -= row[TL::oWF + k * D + j] * w[j];
            bad = bad || !finite_(z);
            q += z * z;
        }
        pr = (R)-0.5 * q + row[TL::oCQ];
        if (bad || isnan_(pr)) pr = 0;
    }
    out3[0] = cc + pr;
    out3[1] = ob + pr;
    out3[2] = qa * inv_delta;
}

// The same three sums with NO per-term policy: every residual kept, nothing tested.  Returns true when the lane's result is not finite -- a non-finite
// residual, difference or row constant makes the sum of the three terms non-finite -- in which case fs_terms (the per-term NaN policy: masked rows are
// zeros, a non-finite kept residual drops its term) has to redo the step; when everything is finite the two agree term by term.  The passes branch on the
// WAVE's ballot of that flag: the policy's fourteen class tests, their boolean algebra and the selects on doubles were a tenth of pass A's instructions,
// spent on a case (a NaN in the state or the data row) that almost no wave ever sees.
template <typename R, int D, int PO>
__device__ __forceinline__ bool fs_terms_fast(const R* row, const R* v, const R* w, const R* u, R inv_delta, R cst, R* out3) {
    using TL = LogShared<R, D, PO>;
    R qo = 0;
#pragma unroll
    for (int k = 0; k < PO; ++k) {
        R z = row[TL::oYw + k];
#pragma unroll
        for (int j = 0; j < D; ++j) z -= row[TL::oWH + k * D + j] * v[j];
        qo += z * z;
    }
    const R ob = (R)-0.5 * qo + row[TL::oCR];
    asm volatile("" ::: "memory");  // (the blocks read disjoint parts of the row: keep their LDS reads apart)
    R qa = 0;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        const R d = u[k] - v[k];
        qa += d * d;
    }
    const R ax = -qa * inv_delta + cst;
    asm volatile("" ::: "memory");
    R qp = 0;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        R z = -row[TL::oWb + k];
#pragma unroll
        for (int l = 0; l <= k; ++l) z += row[TL::oWQ + lidx(k, l)] * v[l];
#pragma unroll
        for (int j = 0; j < D; ++j) z -= row[TL::oWF + k * D + j] * w[j];
        qp += z * z;
    }
    const R pr = (R)-0.5 * qp + row[TL::oCQ];
    out3[0] = (ax + ob) + pr;
    out3[1] = ob + pr;
    out3[2] = qa * inv_delta;
    return !finite_(out3[0]);
}
// fs_terms_fast for TWO states that share the row and the auxiliary variable u -- the current pair (vx, wx) and the proposed pair (vp, wp) -- with every coefficient
// read from LDS ONCE.  Per state the operations and their order are those of fs_terms_fast: the same bits.  The flags are the two calls' return values.
template <typename R, int D, int PO>
__device__ __forceinline__ void fs_terms_fast2(const R* row, const R* vx, const R* wx, const R* vp, const R* wp, const R* u, R inv_delta, R cst, R* ox3, R* op3, bool& badx,
                                               bool& badp) {
    using TL = LogShared<R, D, PO>;
    R qox = 0, qop = 0;
#pragma unroll
    for (int k = 0; k < PO; ++k) {
        R zx = row[TL::oYw + k], zp = zx;
#pragma unroll
        for (int j = 0; j < D; ++j) {
            const R cf = row[TL::oWH + k * D + j];
            zx -= cf * vx[j];
            zp -= cf * vp[j];
        }
        qox += zx * zx;
        qop += zp * zp;
    }
    const R cr = row[TL::oCR];
    const R obx = (R)-0.5 * qox + cr, obp = (R)-0.5 * qop + cr;
    asm volatile("" ::: "memory");  // (the blocks read disjoint parts of the row: keep their LDS reads apart)
    R qax = 0, qap = 0;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        const R dx = u[k] - vx[k], dp = u[k] - vp[k];
        qax += dx * dx;
        qap += dp * dp;
    }
    const R axx = -qax * inv_delta + cst, axp = -qap * inv_delta + cst;
    asm volatile("" ::: "memory");
    R qpx = 0, qpp = 0;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        R zx = -row[TL::oWb + k], zp = zx;
#pragma unroll
        for (int l = 0; l <= k; ++l) {
            const R cf = row[TL::oWQ + lidx(k, l)];
            zx += cf * vx[l];
            zp += cf * vp[l];
        }
#pragma unroll
        for (int j = 0; j < D; ++j) {
            const R cf = row[TL::oWF + k * D + j];
            zx -= cf * wx[j];
            zp -= cf * wp[j];
        }
        qpx += zx * zx;
        qpp += zp * zp;
    }
    const R cq = row[TL::oCQ];
    const R prx = (R)-0.5 * qpx + cq, prp = (R)-0.5 * qpp + cq;
    ox3[0] = (axx + obx) + prx;
    ox3[1] = obx + prx;
    ox3[2] = qax * inv_delta;
    op3[0] = (axp + obp) + prp;
    op3[1] = obp + prp;
    op3[2] = qap * inv_delta;
    badx = !finite_(ox3[0]);
    badp = !finite_(op3[0]);
}
__device__ __forceinline__ bool fs_wave_any(bool flag) { return __builtin_amdgcn_ballot_w64(flag) != 0; }

// the auxiliary variable u_t = x_t + sqrt(delta / 2) eps_aux_t, one fused multiply-add per component.  Pass AC folds it into the filter and pass E rebuilds it for
// the MH terms instead of reading it back: both call THIS, on the same x, step and draw, so the two passes hold the same bits.
template <typename R, int D> __device__ __forceinline__ void fs_aux_u(const R* x, R shd, const R* eps, R* u) {
#pragma unroll
    for (int k = 0; k < D; ++k) {
        if constexpr (sizeof(R) == 8) u[k] = __builtin_fma(shd, eps[k], x[k]);
        else u[k] = __builtin_fmaf(shd, eps[k], x[k]);
    }
}

// ---- pass AC --------------------------------------------------------------------------------------------------------------------------
constexpr int FS_WPE_A = 2;  // least waves per EU of pass AC: the compiler's own choice of registers (DESIGN.md section 4 has 3 and 4 measured against it)
// PK (few chains, one wave per workgroup): lane = sub * cp + chain walks chunk blockIdx.x * pack + sub -- the time index is per lane, everything else is the same code
template <typename R, int D, int PO, bool PK = false>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(FS_WPE_A))) k_fs_ac(FusedArgs a, const R* __restrict__ rows) {
    using F = FsRows<R, D, PO>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    R* lds = (R*)smem;
    fs_resolve(a);
    int ch, c;
    if constexpr (PK) {
        const int sub = (int)threadIdx.x / a.cp;
        c = (int)threadIdx.x - sub * a.cp;
        ch = blockIdx.x * a.pack + sub;
    } else {
        fs_block(a, ch, c);
    }
    const long long C = a.C;
    const int t0 = ch * a.E, ta = max(1, t0), tb = min(a.T, t0 + a.E);
    const FsNormTab<R> ntab = fs_stage_normtab<R>(lds + (PK ? (size_t)a.pack * fs_pk_block<R, F::NC>(a.E) : (size_t)a.E * F::NC));
    if constexpr (PK) {
        const int c0 = blockIdx.x * a.pack;
        fs_stage_pk<R, F::NC>(rows, c0 * a.E, min(a.T, (c0 + a.pack) * a.E), a.E, lds);
        lds += (size_t)(ch - c0) * fs_pk_block<R, F::NC>(a.E);   // the lane's own chunk block
        if (ch >= a.nchunk) return;
    } else {
        fs_stage<R, F::NC>(rows, t0, tb, lds);
    }
    if (c >= a.C) return;
    const R* xr = (const R*)((a.sel && a.sel[c]) ? (const void*)a.xb : a.xa) + c;
    R* ip = (R*)a.inc + c;
    R h[D], es[D];
#pragma unroll
    for (int k = 0; k < D; ++k) {
        h[k] = ch == 0 ? ((const R*)a.m0p)[k * C + c] : (R)0;  // chunk 0 folds from the true m_0; the others from zero (their first mean comes from the aggregate scan)
        es[k] = 0;
    }
    const R shd = (R)a.shd;
    R se = 0;  // sum |eps_samp|^2 over the chunk's steps: the data part of log q(x' | u)
    // one LOCAL sampler increment: inc0 = M1 h - gb + Lc eps (SampleAffOp::step without the G term, with the chunk-local mean h), stored, and folded into the chunk aggregate
    auto emit = [&](int tu, const R* row, const R* eps) {
        R inc[D];
#pragma unroll
        for (int k = 0; k < D; ++k) se += eps[k] * eps[k];
#pragma unroll
        for (int i = 0; i < D; ++i) {
            R v = -row[F::cGb + i];
#pragma unroll
            for (int k = 0; k < D; ++k) v += row[F::cM1 + i * D + k] * h[k];
#pragma unroll
            for (int k = 0; k <= i; ++k) v += row[F::cL + lidx(i, k)] * eps[k];
            inc[i] = v;
            ip[((long long)tu * D + i) * C] = v;
        }
#pragma unroll
        for (int i = 0; i < D; ++i) {
            R v = es[i];
#pragma unroll
            for (int k = 0; k < D; ++k) v += row[F::cGp + i * D + k] * inc[k];
            es[i] = v;
        }
    };
    if (ch == 0) {  // t = 0: the mean of k_filter_t0, the noise row of the fill kernel
        R eps[D];
#pragma unroll
        for (int k = 0; k < D; ++k) eps[k] = ((const R*)a.eps0s)[k * C + c];
        emit(0, lds, eps);
    }
    R xn[D];  // the next step's state, fetched one step ahead
#pragma unroll
    for (int k = 0; k < D; ++k) xn[k] = ta < tb ? xr[((long long)ta * D + k) * C] : (R)0;
#pragma unroll 1
    for (int t = ta; t < tb; ++t) {
        const int tu = PK ? t : opaque_uniform(t);
        const R* row = lds + (tu - t0) * F::NC;
        R x[D], ev[D], u[D];
#pragma unroll
        for (int k = 0; k < D; ++k) x[k] = xn[k];
        if (t + 1 < tb) {
            const int tn = PK ? t + 1 : opaque_uniform(t + 1);
#pragma unroll
            for (int k = 0; k < D; ++k) xn[k] = xr[((long long)tn * D + k) * C];
        }
        normals_cm<R, D>(a.ka0, a.ka1, (long long)tu * D * C + c, C, ev, ntab);
        fs_aux_u<R, D>(x, shd, ev, u);  // (kept in registers: pass E rebuilds it from x and the same draw)
        // the fold takes a non-finite component of u as zero (FilterMeanOp's masking).  One test per step: a non-finite component makes the sum non-finite, and
        // the rare wave that sees one masks component by component (a finite u whose sum overflows gets there too, and is left as it is).
        R um[D], us = u[0];
#pragma unroll
        for (int k = 1; k < D; ++k) us += u[k];
#pragma unroll
        for (int k = 0; k < D; ++k) um[k] = u[k];
        if (fs_wave_any(!finite_(us))) {
#pragma unroll
            for (int k = 0; k < D; ++k) um[k] = finite_(u[k]) ? u[k] : (R)0;
        }
        {  // filter fold (FilterMeanOp::fold, folded rows): h <- Mb h + kc + K[:, :D] u -- the chunk aggregate at the end, the chunk-local filtered mean on the way
            R o[D];
#pragma unroll
            for (int r = 0; r < D; ++r) {
                R v = row[F::cKc + r];
#pragma unroll
                for (int k = 0; k < D; ++k) v += row[F::cM + r * D + k] * h[k];
#pragma unroll
                for (int k = 0; k < D; ++k) v += row[F::cK + r * D + k] * um[k];
                o[r] = v;
            }
#pragma unroll
            for (int r = 0; r < D; ++r) h[r] = o[r];
        }
        asm volatile("" ::: "memory");
        R eps[D];
        normals_cm<R, D>(a.ks0, a.ks1, (long long)tu * D * C + c, C, eps, ntab);
        emit(tu, row, eps);
    }
    stv<R, D>((R*)a.agg_f + ((long long)c * a.nchunk + ch) * SampPre<R, D>::NPAD, h);
    stv<R, D>((R*)a.agg_s + ((long long)c * a.nchunk + (a.nchunk - 1 - ch)) * SampPre<R, D>::NPAD, es);
    ((R*)a.pell)[(long long)c * a.nchunk + ch] = (R)-0.5 * se;
}

// ---- pass E ---------------------------------------------------------------------------------------------------------------------------
// The unpacked form (more than 128 chains) streams arrays far larger than the caches, each touched once per sweep: a record of inc0 or u is read exactly once, here,
// and is dead afterwards; a line of x' is next touched by the following sweep's pass AC, a whole array later.  Its record loads and x' stores carry the
// non-temporal hint, and its blocks walk the chunks from the LAST one down (pass AC wrote the last chunks' records last; the pass ends on chunk 0, where the next
// pass AC starts).  Measured together: pass E 364 -> 336 us at 256 chains, T = 65536, d = 4, fp64; the sweep -3.4 % there, -3.8 % at 1024
// chains.  What did NOT move the pass is listed there too: more records in flight per lane, two chains per lane with 16-byte accesses.  Same values, same
// arithmetic: only the cache policy of the memory instructions and the order of the blocks differ from the packed form.
template <bool ONCE, typename R> __device__ __forceinline__ R fs_ld_once(const R* p) {
    if constexpr (ONCE) return __builtin_nontemporal_load(p);
    else return *p;
}
template <bool ONCE, typename R> __device__ __forceinline__ void fs_st_once(R* p, R v) {
    if constexpr (ONCE) __builtin_nontemporal_store(v, p);
    else *p = v;
}
// The pass also forms the MH terms of the CURRENT state x.  They need x and u only, and the pass has the issue slots pass AC lacks: it reads x (the bytes it used
// to read of u) from the chain's current buffer -- x' goes to the other one, so the two never alias -- rebuilds u_{t+1} = x_{t+1} + sqrt(delta / 2) eps_aux_{t+1} from the
// keyed draw with pass AC's own helper (fs_aux_u: the bits pass AC folded), and evaluates the pair (x_{t+1}, x_t) beside (x'_{t+1}, x'_t) from the same LDS row
// reads (fs_terms_fast2).  The pair (t + 1, t) is summed into the chunk of t for both states; k_fs_accept adds the chunks of a chain, whichever chunk a pair is in.
// x is loaded plainly (it is read again by the next sweep; non-temporal loads measured inside the noise: 273.5k-277.0k against 269.3k-273.8k sweeps/s at 256 chains,
// equal at 1024); inc0 is dead after its one read and stays non-temporal.
constexpr int FS_WPE_E = 2;  // two waves per EU: with two states' terms in flight the widest instantiations otherwise take a few registers more than half the file
template <typename R, int D, int PO, bool PK = false>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(FS_WPE_E))) k_fs_e(FusedArgs a, const R* __restrict__ rows) {
    using F = FsRows<R, D, PO>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    R* lds = (R*)smem;
    fs_resolve(a);
    int ch, c;
    if constexpr (PK) {
        const int sub = (int)threadIdx.x / a.cp;
        c = (int)threadIdx.x - sub * a.cp;
        ch = blockIdx.x * a.pack + sub;
    } else {
        fs_block(a, ch, c, true);
    }
    const long long C = a.C;
    const int t0 = ch * a.E, tb = min(a.T, t0 + a.E);
    const FsNormTab<R> ntab = fs_stage_normtab<R>(lds + (PK ? (size_t)a.pack * fs_pk_block<R, F::NE>(a.E) : (size_t)a.E * F::NE));
    if constexpr (PK) {
        const int c0 = blockIdx.x * a.pack;
        fs_stage_pk<R, F::NE>(rows, c0 * a.E, min(a.T, (c0 + a.pack) * a.E), a.E, lds);
        lds += (size_t)(ch - c0) * fs_pk_block<R, F::NE>(a.E);
        if (ch >= a.nchunk) return;
    } else {
        fs_stage<R, F::NE>(rows, t0, tb, lds);
    }
    if (c >= a.C) return;
    const bool sw = a.sel && a.sel[c];
    const R* xr = (const R*)(sw ? (const void*)a.xb : a.xa) + c;  // the chain's current state, as pass AC read it
    R* xw = (R*)(sw ? const_cast<void*>(a.xa) : a.xb) + c;
    const R* ip = (const R*)a.inc + c;
    R h[D], xh[D], uq[D], mst[D];  // x'_{t+1}, x_{t+1}, u_{t+1}; mst: the chunk's first filtered mean (aggregate scan of the folds): the part of the increments pass AC could not know
    if (ch > 0) {
        ldv<R, D>((const R*)a.pre_f + ((long long)c * a.nchunk + ch) * SampPre<R, D>::NPAD, mst);
    } else {
#pragma unroll
        for (int k = 0; k < D; ++k) mst[k] = 0;
    }
    if (ch == a.nchunk - 1) {
#pragma unroll
        for (int k = 0; k < D; ++k) h[k] = 0, xh[k] = 0;  // G_{T-1} = 0: the first position ignores the incoming state, and there is no pair above T - 1
    } else {
        ldv<R, D>((const R*)a.pre_s + ((long long)c * a.nchunk + (a.nchunk - 1 - ch)) * SampPre<R, D>::NPAD, h);  // x'_{tb}
#pragma unroll
        for (int k = 0; k < D; ++k) xh[k] = xr[((long long)tb * D + k) * C];  // x_{tb}: the one load of the chunk above
    }
#pragma unroll
    for (int k = 0; k < D; ++k) uq[k] = 0;
    const R shd = (R)a.shd, inv_delta = (R)1 / (R)a.delta;
    const R cst = (R)-0.5 * (R)D * log_((R)(0.5 * a.delta)) - (R)(0.5 * LOG_2PI) * (R)D;
    Acc v0 = 0, v1 = 0, v2 = 0, s0 = 0, s1 = 0, s2 = 0;  // the chunk's sums of x' (v) and of x (s)
    R incn[D], xn[D];  // the next (earlier) step's records, fetched one step ahead
#pragma unroll
    for (int k = 0; k < D; ++k) incn[k] = fs_ld_once<!PK>(ip + ((long long)(tb - 1) * D + k) * C), xn[k] = xr[((long long)(tb - 1) * D + k) * C];
#pragma unroll 1
    for (int t = tb - 1; t >= t0; --t) {
        const int tu = PK ? t : opaque_uniform(t);
        const R* row = lds + (tu - t0) * F::NE;
        R inc[D], xt[D], xp[D];
#pragma unroll
        for (int k = 0; k < D; ++k) inc[k] = incn[k], xt[k] = xn[k];
        if (t > t0) {
            const int tn = PK ? t - 1 : opaque_uniform(t - 1);
#pragma unroll
            for (int k = 0; k < D; ++k) incn[k] = fs_ld_once<!PK>(ip + ((long long)tn * D + k) * C), xn[k] = xr[((long long)tn * D + k) * C];
        }
#pragma unroll
        for (int i = 0; i < D; ++i) {
            R v = inc[i];
#pragma unroll
            for (int k = 0; k < D; ++k) v += row[F::eN + i * D + k] * mst[k];
#pragma unroll
            for (int k = 0; k < D; ++k) v += row[F::eG + i * D + k] * h[k];
            xp[i] = v;
            fs_st_once<!PK>(xw + ((long long)tu * D + i) * C, v);
        }
        asm volatile("" ::: "memory");  // (the log-density row's LDS reads stay behind the walk's: hoisted together they do not fit two waves' registers)
        if (tu + 1 < a.T) {  // (wave-uniform; per lane pair in the packed form) LogShared row tu: the states at tu + 1 given those at tu, observation and auxiliary terms at tu + 1
            R ev[D];
            normals_cm<R, D>(a.ka0, a.ka1, (long long)(tu + 1) * D * C + c, C, ev, ntab);
            fs_aux_u<R, D>(xh, shd, ev, uq);
            asm volatile("" ::: "memory");
            R wx[3], wp[3];
            bool badx, badp;
            fs_terms_fast2<R, D, PO>(row + F::eL, xh, xt, h, xp, uq, inv_delta, cst, wx, wp, badx, badp);
            // the rare wave with a non-finite value in either state redoes both under the per-term policy (finite terms come out as the fast path's, bit for
            // bit).  One branch for the two: a branch per state costs sixty registers and spills at two waves per EU.
            if (fs_wave_any(badx || badp)) {
                asm volatile("" ::: "memory");
                fs_terms<R, D, PO>(a, row + F::eL, xh, xt, uq, inv_delta, cst, wx);
                asm volatile("" ::: "memory");
                fs_terms<R, D, PO>(a, row + F::eL, h, xp, uq, inv_delta, cst, wp);
            }
            v0 += (Acc)wp[0];
            v1 += (Acc)wp[1];
            v2 += (Acc)wp[2];
            s0 += (Acc)wx[0];
            s1 += (Acc)wx[1];
            s2 += (Acc)wx[2];
        }
#pragma unroll
        for (int k = 0; k < D; ++k) h[k] = xp[k], xh[k] = xt[k];
    }
    a.pa[((long long)0 * C + c) * a.nchunk + ch] = s0;
    a.pa[((long long)1 * C + c) * a.nchunk + ch] = s1;
    a.pa[((long long)2 * C + c) * a.nchunk + ch] = s2;
    a.pe[((long long)0 * C + c) * a.nchunk + ch] = v0;
    a.pe[((long long)1 * C + c) * a.nchunk + ch] = v1;
    a.pe[((long long)2 * C + c) * a.nchunk + ch] = v2;
}

// ---- t = 0 terms (one lane per chain): body_sweep_logpdf_head on the lane's own pair of buffers -----------------------------------------------
template <typename R, int D, int PO> __global__ void __launch_bounds__(TB_ELEM) k_fs_head(SweepLogpdfArgs la, const void* xa, const void* xb, const int32_t* sel, R* __restrict__ head5) {
    resolve_step(la);
    const int c = blockIdx.x * TB_ELEM + threadIdx.x;
    if (c >= la.d.C) return;
    const bool sw = sel && sel[c];
    la.x.ptr = sw ? xb : xa;
    la.xp.ptr = sw ? xa : xb;
    R h5[5];
    body_sweep_logpdf_head<R, D, PO>(la, c, h5);
#pragma unroll
    for (int k = 0; k < 5; ++k) head5[(long long)k * la.d.C + c] = h5[k];
}

// ---- accept (generic.py:70-73, 98-106): one workgroup per chain sums its chunks' partial totals in a fixed order, forms log alpha in Acc
// exactly as k_accept does, draws the Bernoulli and -- lazy state -- flips the chain's buffer selector ------------------------------------------
// The steps the reference's nansum dropped from the concatenated likelihood of x' because an observation is missing (base.py:137-166 on ys = [u; y]): what
// the TRUE joint density of (x', u, y) holds there -- N(u_t; x'_t, delta/2 I) and the density of the finite components of y_t -- from the model's arrays.
// One workgroup per chain, its lanes over the time steps; the caller asks only when the model stage saw a non-finite log-density row (FusedArgs::nanrow) or y_0 is missing.
template <typename R, int D, int PO> __device__ __forceinline__ Acc fs_dropped_joint(const FusedArgs& a, const SweepLogpdfArgs& la, int c, const int32_t* sel) {
    Acc s = 0;
    const long long C = a.C;
    const R* xp = (const R*)((sel && sel[c]) ? a.xa : (const void*)a.xb) + c;  // the proposal: the buffer the chain does not live in
    // u is not kept: row 0 is the caller's (a.u holds that row alone); u_t, t >= 1, is rebuilt as the passes build it, from the chain's current state and the number
    // normals_cm puts at (t, k, c) -- here one whole block per number (stream_normal: the same bits), for the few steps with a missing observation
    const R* xc = (const R*)((sel && sel[c]) ? (const void*)a.xb : a.xa) + c;
    const R* u0 = (const R*)a.u + c;
    const R shd = (R)a.shd, inv_delta = (R)1 / (R)a.delta;
    const R cst = (R)-0.5 * (R)D * log_((R)(0.5 * a.delta)) - (R)(0.5 * LOG_2PI) * (R)D;
    for (int t = threadIdx.x; t < a.T; t += TB_ELEM) {
        R y[PO];
        rd<R, PO>(la.ys, c, t, 0, y);
        bool skip[PO], any = false;
#pragma unroll
        for (int k = 0; k < PO; ++k) skip[k] = !finite_(y[k]), any = any || skip[k];
        if (!any) continue;
        R H[PO * D], cv[PO], Rm[PO * PO], v[D], r[PO], q = 0;
        bool b = false;  // (a non-finite u_t - x'_t -- a NaN in the chain's state -- drops the auxiliary block, as fs_terms does; gauss_logpdf drops a non-finite kept residual)
        rd<R, PO * D>(la.Hs, c, t, 0, H);
        rd<R, PO>(la.cs, c, t, 0, cv);
        rd_upper<R, PO>(la.Rs, c, t, 0, Rm);
        R ut[D];
        if (t == 0) {
#pragma unroll
            for (int k = 0; k < D; ++k) ut[k] = u0[k * C];
        } else {
            R xt[D], ev[D];
#pragma unroll
            for (int k = 0; k < D; ++k) {
                xt[k] = xc[((long long)t * D + k) * C];
                ev[k] = stream_normal<R>(a.ka0, a.ka1, 0, (unsigned long long)(((long long)t * D + k) * C + c));
            }
            fs_aux_u<R, D>(xt, shd, ev, ut);
        }
#pragma unroll
        for (int k = 0; k < D; ++k) {
            v[k] = xp[((long long)t * D + k) * C];
            const R d = ut[k] - v[k];
            b = b || !finite_(d);
            q += d * d;
        }
#pragma unroll
        for (int k = 0; k < PO; ++k) {
            R p = cv[k];
#pragma unroll
            for (int j = 0; j < D; ++j) p += H[k * D + j] * v[j];
            r[k] = y[k] - p;
        }
        s += (Acc)(b ? (R)0 : -q * inv_delta + cst) + (Acc)gauss_logpdf<R, PO>(r, Rm, skip);
    }
    return s;
}
template <typename R, int D, int PO> __global__ void __launch_bounds__(TB_ELEM) k_fs_accept(FusedArgs a, SweepLogpdfArgs lg, const R* __restrict__ head5, const R* __restrict__ ell0,
                                                                                            const R* __restrict__ u_acc, int32_t* __restrict__ accepted, R* __restrict__ logs,
                                                                                            int32_t* __restrict__ sel) {
    __shared__ Acc sh[TB_ELEM];
    fs_resolve(a);
    const int c = blockIdx.x;
    const long long C = a.C;
    // are there dropped steps to add back?  (workgroup-uniform: the rows of t >= 1 raise the flag, row 0 has no table row; loaded here, used after the sums below)
    bool any_dropped = false;
    if (a.nan_policy == 0) {
        R y0[PO];
        rd<R, PO>(lg.ys, c, 0, 0, y0);
        any_dropped = *a.nanrow != 0;
#pragma unroll
        for (int k = 0; k < PO; ++k) any_dropped = any_dropped || !finite_(y0[k]);
    }
    Acc tot[7] = {0, 0, 0, 0, 0, 0, 0};
    const R* pl = (const R*)a.pell + (long long)c * a.nchunk;
    for (int j = threadIdx.x; j < a.nchunk; j += TB_ELEM) {  // (seven independent loads per trip)
#pragma unroll
        for (int k = 0; k < 3; ++k) tot[k] += a.pa[((long long)k * C + c) * a.nchunk + j], tot[3 + k] += a.pe[((long long)k * C + c) * a.nchunk + j];
        tot[6] += (Acc)pl[j];
    }
#pragma unroll
    for (int k = 0; k < 7; ++k) tot[k] = block_sum<Acc, TB_ELEM>(tot[k], sh);
    Acc dropped = 0;
    if (any_dropped) dropped = block_sum<Acc, TB_ELEM>(fs_dropped_joint<R, D, PO>(a, lg, c, sel), sh);
    if (threadIdx.x != 0) return;
    // The marginal log-likelihood of the auxiliary model WITHOUT walking its innovations: for any path z, ell = log p(z, u, y) - log p(z | u, y), and for the sampled
    // proposal x' both are at hand -- the joint is the sum pass E forms anyway (jp_prop), the conditional is the density of the pathwise draw,
    // log q(x' | u) = sum_t (-1/2 |eps_t|^2 - log|Lc_t| - D/2 log 2 pi) (pass C accumulates the first term, k_fs_clog the rest).  Same quantity as filtering.py:55-62
    // to rounding; log alpha does not depend on it at all (it enters lp_prop and lp_rev alike), only the reported lp_prop / lp_rev do.  Under the reference policy
    // jp_prop lacks the steps the nansum dropped for a missing observation, which log q(x' | u) holds: `dropped` completes the joint (without it lp_prop and lp_rev
    // were both off by that sum whenever data were missing).
    (void)ell0;
    const Acc jp_prop = tot[3] + (Acc)head5[0 * C + c], jp_rev = tot[0] + (Acc)head5[1 * C + c];
    const Acc ell = (jp_prop + dropped) - (tot[6] - *a.clog);
    const Acc lt_prop = tot[4] + (Acc)head5[2 * C + c], lt_rev = tot[1] + (Acc)head5[3 * C + c];
    const Acc corr = (tot[5] - tot[2]) + (Acc)head5[4 * C + c];
    const Acc lp_prop = jp_prop - ell, lp_rev = jp_rev - ell;
    Acc la = lt_prop - lt_rev;
    la += lp_rev - lp_prop;
    la -= corr;
    const Acc alpha = exp_(la != la ? la : min_(la, (Acc)0));  // jnp.minimum(0, nan) = nan (generic.py:105): a NaN ratio rejects
    const int acc = ((Acc)u_acc[c] < alpha) ? 1 : 0;  // NaN alpha -> reject, as jax.random.bernoulli(key, nan)
    accepted[c] = acc;
    if (sel) sel[c] ^= acc;
    if (logs) {
        logs[c * 5 + 0] = (R)la;
        logs[c * 5 + 1] = (R)lp_prop;
        logs[c * 5 + 2] = (R)lp_rev;
        logs[c * 5 + 3] = (R)lt_prop;
        logs[c * 5 + 4] = (R)lt_rev;
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
// few chains (<= 128): how many chunks one workgroup of up to 256 lanes walks side by side (lanes = pack x cp), 1 = the plain mapping.
// Measured at C2's sizes (profiles/r04_i_low_chain_layout.txt): 8 chains 18.2k -> 23.4k sweeps/s, 16 chains 40.7k -> 51.0k, 32 chains 78.0k -> 91.0k, 64 chains 133.7k -> 152.0k,
// 128 chains 189.4k -> 218.4k (the chunks of a workgroup share one staging of the normal tables and one barrier).
inline int fs_pack(int C, int* cp_out) {
    int cp = 2;
    while (cp < C) cp <<= 1;
    *cp_out = cp;
    constexpr int lanes = 256;   // lanes per packed workgroup (measured: 256 best from 32 chains on)
    if (cp > lanes / 2) return 1;
    const int pack = lanes / cp;
    constexpr int cap = 8;   // (LDS: pack blocks of E coefficient rows)
    return pack > cap ? cap : pack;
}
static_assert(FS_RULE_TILE == TB_CM, "fs_chunk_rule counts the chain tiles of the affine passes");
inline int fs_chunk_len(const auxssm_ctx* h, int C, int T) { return fs_chunk_rule(h->num_cu, C, T); }  // (the rule and what it was measured on: fs_chunk.h)
template <typename R, int D, int PO> size_t fused_ws(const auxssm_ctx* h, const KDims& d) {
    constexpr int P = D + PO;
    const int E = fs_chunk_len(h, d.C, d.T), nchunk = (d.T + E - 1) / E;
    size_t b = 0;
    b += (size_t)d.C * nchunk * (4 * SampPre<R, D>::NPAD * sizeof(R) + 6 * sizeof(Acc) + sizeof(R)) + 16 * 256;
    b += (size_t)d.C * (5 + 1 + D) * sizeof(R) + 4 * 256;
    // model stage (side slab when the stage overlaps, else this one): matrix filter, gain / sampler / log-density tables, chunk products
    b += filter_ws<R, D, P>(h, KDims{1, d.T, 1}, 1);
    b += (size_t)d.T * (SampShared<R, D>::NPAD + LogShared<R, D, PO>::NPAD + (size_t)D * D) * sizeof(R) + (size_t)2 * nchunk * D * D * sizeof(R) + 10 * 256 + ((size_t)d.T / 256 + 2) * sizeof(Acc);
    b += (size_t)d.T * (FsRows<R, D, PO>::NC + FsRows<R, D, PO>::NE + 2 * (size_t)D * D) * sizeof(R) + (size_t)nchunk * D * D * sizeof(R) + 8 * 256;
    b += (2 * fs_mid_ks_reals<D>() + 3 * fs_mid_ser_reals<D>(nchunk)) * sizeof(R) + 2 * 256;  // the lane-minor tables of the two aggregate scans (k_fs_gtab)
    return b;
}
template <typename R, int D, int PO> int run_fused_shared(auxssm_ctx* h, FusedHost& f) {
    constexpr int P = D + PO;
    const int C = f.fa.d.C, T = f.fa.d.T, n = T - 1;
    FusedArgs a{};
    a.C = C; a.T = T;
    a.E = fs_chunk_len(h, C, T);
    a.nchunk = (T + a.E - 1) / a.E;
    a.pack = fs_pack(C, &a.cp);
    {   // the packed workgroup stages `pack` chunk blocks of coefficient rows: keep them (and the normal tables) within 128 KB of LDS
        using FR = FsRows<R, D, PO>;
        constexpr int NMAX = FR::NC > FR::NE ? FR::NC : FR::NE;
        while (a.pack > 1 && (size_t)a.pack * fs_pk_block<R, NMAX>(a.E) * sizeof(R) + FsNormTabSel<R>::BYTES > (size_t)128 * 1024) a.pack >>= 1;
    }
    a.xa = f.xa; a.xb = f.xb; a.sel = f.sel; a.u = f.u; a.inc = f.inc;
    a.ka0 = f.keys[0]; a.ka1 = f.keys[1]; a.ks0 = f.keys[2]; a.ks1 = f.keys[3];
    a.eps0s = f.eps0s;
    a.delta = f.la.delta; a.shd = f.la.shd; a.dptr = f.la.dptr; a.nan_policy = f.la.nan_policy;
    a.memo = f.memo;
    f.fa.memo = f.sa.memo = f.la.memo = f.memo;  // the model stage below; cleared before the chain passes (k_filter_t0 serves both)
    R *cprod_f, *cprod_s, *rows_c, *rows_e, *psi, *gtab_f, *gtab_s;
    {
        // MODEL STAGE (ctx.h::SideStage when the sweep opened one): everything that reads the model and the step size only
        {
            const int rc = build_gain_table<R, D, P>(h, f.fa);
            if (rc) return rc;
        }
        SideScope side(h);
        f.sa.tab = ws_take(h, (size_t)T * SampShared<R, D>::NPAD * sizeof(R));
        f.la.tab = ws_take(h, (size_t)n * LogShared<R, D, PO>::NPAD * sizeof(R));
        R* gpre = (R*)ws_take(h, (size_t)T * D * D * sizeof(R));
        cprod_f = (R*)ws_take(h, (size_t)a.nchunk * D * D * sizeof(R));
        cprod_s = (R*)ws_take(h, (size_t)a.nchunk * D * D * sizeof(R));
        rows_c = (R*)ws_take(h, (size_t)T * FsRows<R, D, PO>::NC * sizeof(R));
        rows_e = (R*)ws_take(h, (size_t)T * FsRows<R, D, PO>::NE * sizeof(R));
        R* fpre = (R*)ws_take(h, (size_t)T * D * D * sizeof(R));
        R* ntab = (R*)ws_take(h, (size_t)T * D * D * sizeof(R));
        psi = (R*)ws_take(h, (size_t)a.nchunk * D * D * sizeof(R));
        const size_t nks = fs_mid_ks_reals<D>(), nser = fs_mid_ser_reals<D>(a.nchunk);
        gtab_f = (R*)ws_take(h, (nks + nser) * sizeof(R));
        gtab_s = (R*)ws_take(h, (nks + 2 * nser) * sizeof(R));
        const int nclb = (T + 255) / 256;
        Acc* clog = (Acc*)ws_take(h, 256 + (size_t)nclb * sizeof(Acc));  // [0] the sum, [32 ...) the partial sums
        if (!f.sa.tab || !f.la.tab || !gpre || !cprod_f || !cprod_s || !rows_c || !rows_e || !fpre || !ntab || !psi || !gtab_f || !gtab_s || !clog) return AUXSSM_ERR_NOMEM;
        a.clog = clog;
        int* nanrow = (int*)(clog + 16);  // (in the sum's 256-byte header: lives and is memoised with the tables)
        a.nanrow = nanrow;
        a.gain = f.fa.tab; a.samp = f.sa.tab; a.logt = f.la.tab; a.gpre = gpre;
        {
            ProfScope ps(h, AUXSSM_K_SAMPLE_INIT);
            hipLaunchKernelGGL((k_sample_shared_tab<R, D>), dim3((T + TB_ELEM - 1) / TB_ELEM), dim3(TB_ELEM), 0, h->stream, f.sa);
            hipLaunchKernelGGL((k_fs_clog_part<R, D>), dim3(nclb), dim3(256), 0, h->stream, T, (const R*)f.sa.tab, clog + 32, f.memo);
            hipLaunchKernelGGL((k_fs_clog_sum<D>), dim3(1), dim3(256), 0, h->stream, T, nclb, (const Acc*)(clog + 32), clog, nanrow, f.memo);
            hipLaunchKernelGGL((k_sweep_logpdf_tab<R, D, PO>), dim3((n + TB_ELEM - 1) / TB_ELEM), dim3(TB_ELEM), 0, h->stream, f.la);
            hipLaunchKernelGGL((k_fs_fprod<R, D, P>), dim3((a.nchunk + TB_CM - 1) / TB_CM), dim3(TB_CM), 0, h->stream, a, cprod_f, fpre);
            hipLaunchKernelGGL((k_fs_gpre<R, D>), dim3((a.nchunk + TB_CM - 1) / TB_CM), dim3(TB_CM), 0, h->stream, a, gpre, cprod_s);
            hipLaunchKernelGGL((k_fs_psi<R, D>), dim3((a.nchunk + TB_CM - 1) / TB_CM), dim3(TB_CM), 0, h->stream, a, (const R*)gpre, (const R*)fpre, ntab, psi);
            hipLaunchKernelGGL((k_fs_gtab<R, D>), dim3(1), dim3(TB_AGGS), 0, h->stream, a, (const R*)cprod_f, (const R*)nullptr, gtab_f, gtab_f + nks, (R*)nullptr);
            hipLaunchKernelGGL((k_fs_gtab<R, D>), dim3(1), dim3(TB_AGGS), 0, h->stream, a, (const R*)cprod_s, (const R*)psi, gtab_s, gtab_s + nks, gtab_s + nks + nser);
            {
                using F = FsRows<R, D, PO>;
                const long long nmax = (long long)T * (F::NC > F::NE ? F::NC : F::NE);
                hipLaunchKernelGGL((k_fs_rows<R, D, PO>), dim3((unsigned)((nmax + 255) / 256), 2), dim3(256), 0, h->stream, a, (const R*)ntab, rows_c, rows_e, nanrow);
            }
        }
    }
    {
        const int rc = side_close(h);
        if (rc) return rc;
    }
    a.memo = nullptr;
    f.fa.memo = f.sa.memo = f.la.memo = nullptr;  // (the chain passes are never skipped)
    const size_t npre = (size_t)C * a.nchunk * SampPre<R, D>::NPAD * sizeof(R);
    a.agg_f = ws_take(h, npre); a.pre_f = ws_take(h, npre); a.agg_s = ws_take(h, npre); a.pre_s = ws_take(h, npre);
    a.pa = (Acc*)ws_take(h, (size_t)3 * C * a.nchunk * sizeof(Acc));
    a.pe = (Acc*)ws_take(h, (size_t)3 * C * a.nchunk * sizeof(Acc));
    a.pell = ws_take(h, (size_t)C * a.nchunk * sizeof(R));
    R* head5 = (R*)ws_take(h, (size_t)5 * C * sizeof(R));
    f.fa.ell0 = ws_take(h, (size_t)C * sizeof(R));
    if (!a.agg_f || !a.pre_f || !a.agg_s || !a.pre_s || !a.pa || !a.pe || !a.pell || !head5 || !f.fa.ell0) return AUXSSM_ERR_NOMEM;
    a.m0p = f.fa.ms.ptr;
    // t = 0 update of every chain (reads the concatenated model: after the join)
    f.fa.t0_keep_ps = 1;
    hipLaunchKernelGGL((k_filter_t0<R, D, P>), dim3((C + TB_ELEM - 1) / TB_ELEM), dim3(TB_ELEM), 0, h->stream, f.fa);
    using F = FsRows<R, D, PO>;
    const int TBF = C >= 256 ? 256 : (C + 63) / 64 * 64;
    const unsigned grid = (unsigned)a.nchunk * (unsigned)((C + TBF - 1) / TBF);
    const unsigned grid_pk = (unsigned)((a.nchunk + a.pack - 1) / a.pack);
    if (a.pack > 1) {
        const size_t lds_ac = (size_t)a.pack * fs_pk_block<R, F::NC>(a.E) * sizeof(R) + FsNormTabSel<R>::BYTES;
        if (lds_ac > 64 * 1024) AX_HIP(hipFuncSetAttribute((const void*)k_fs_ac<R, D, PO, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_ac));
        ProfScope ps(h, AUXSSM_K_FILTER_SCAN);
        hipLaunchKernelGGL((k_fs_ac<R, D, PO, true>), dim3(grid_pk), dim3(a.pack * a.cp), lds_ac, h->stream, a, (const R*)rows_c);
    } else {
        const size_t lds_ac = (size_t)a.E * F::NC * sizeof(R) + FsNormTabSel<R>::BYTES;
        if (lds_ac > 64 * 1024) AX_HIP(hipFuncSetAttribute((const void*)k_fs_ac<R, D, PO>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_ac));
        ProfScope ps(h, AUXSSM_K_FILTER_SCAN);
        hipLaunchKernelGGL((k_fs_ac<R, D, PO>), dim3(grid), dim3(TBF), lds_ac, h->stream, a, (const R*)rows_c);
    }
    {
        ProfScope ps(h, AUXSSM_K_SAMPLE_SCAN);  // the two aggregate scans: first means of the chunks, then (completed by Psi m_start) the sampler's chunk starts
        hipLaunchKernelGGL((k_fs_mid<R, D>), dim3(C), dim3(TB_AGGS), 0, h->stream, a, (const R*)gtab_f, (const R*)gtab_s);
    }
    {
        ProfScope ps(h, AUXSSM_K_LOGPDF);
        if (a.pack > 1) {
            const size_t lds_e = (size_t)a.pack * fs_pk_block<R, F::NE>(a.E) * sizeof(R) + FsNormTabSel<R>::BYTES;
            if (lds_e > 64 * 1024) AX_HIP(hipFuncSetAttribute((const void*)k_fs_e<R, D, PO, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_e));
            hipLaunchKernelGGL((k_fs_e<R, D, PO, true>), dim3(grid_pk), dim3(a.pack * a.cp), lds_e, h->stream, a, (const R*)rows_e);
        } else {
            const size_t lds_e = (size_t)a.E * F::NE * sizeof(R) + FsNormTabSel<R>::BYTES;
            if (lds_e > 64 * 1024) AX_HIP(hipFuncSetAttribute((const void*)k_fs_e<R, D, PO>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_e));
            hipLaunchKernelGGL((k_fs_e<R, D, PO>), dim3(grid), dim3(TBF), lds_e, h->stream, a, (const R*)rows_e);
        }
    }
    {
        ProfScope ps(h, AUXSSM_K_SELECT);
        hipLaunchKernelGGL((k_fs_head<R, D, PO>), dim3((C + TB_ELEM - 1) / TB_ELEM), dim3(TB_ELEM), 0, h->stream, f.la, f.xa, (const void*)f.xb, (const int32_t*)f.sel, head5);
        hipLaunchKernelGGL((k_fs_accept<R, D, PO>), dim3(C), dim3(TB_ELEM), 0, h->stream, a, f.la, (const R*)head5, (const R*)f.fa.ell0, (const R*)f.u_acc, f.accepted,
                           (R*)f.logs, f.sel);
    }
    AX_HIP(hipGetLastError());
    return AUXSSM_OK;
}

