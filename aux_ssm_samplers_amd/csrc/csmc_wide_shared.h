// csmc_wide_shared.h -- the device code the two wide-state units share (4 < dx <= 32; csmc_wide.hip: the sequential sweep, pit_wide.hip: the parallel-in-time
// sweep): the model as pointers into the device block cached on the handle (FkW, cw_model), the gradient kernel of their common prologue (k_cw_grad) and the
// half-wave forms of the densities and potentials -- a particle's dx components ACROSS the 32 lanes of a half-wave, every sum in the order the sweep contract
// states (csmc_wide.hip, "Both passes").  Units including this are compiled with -ffp-contract=off.
#pragma once
#include <type_traits>
#include <utility>

#include "csmc_host.h"

namespace ax {

constexpr int CSW_MAXD = 32;

template <typename R> struct FkW {
    int proposal, potential, D;
    const R *m0, *LP0, *iLP0, *F, *b, *LQ, *iLQ;  // device arrays, matrices row-major with leading dimension D
    R c_init, c_trans, c_obs, inv_sig_y;
    int gradient;                          // AUXSSM_GRAD_*
    const R *Ft, *bt, *LQt, *ctt, *idt;    // time-varying transitions (csmc_sweep.h::FkDev: row t = transition t -> t + 1), or null
    const R* pot_mat;                      // the matrix of a coupled potential (device, leading dimension D; csmc_sweep.h::FkDev::pot_mat), or null
    R mvt_hc, mvt_inv_nu;
    AXD_HD int mat_ld() const { return D; }  // the leading dimension of the matrices
};
// the transition t -> t + 1 in global memory (gradient kernel; the sweep kernels read it from LDS)
template <typename R> struct TransW {
    const R *F, *b, *LQ;
};
// element (i, j) of chol P0 (init) or chol Q (csmc_guided.h::k_csmc_gtab)
template <typename R> __device__ __forceinline__ R gt_chol(const FkW<R>& m, bool init, int i, int j) { return (init ? m.LP0 : m.LQ)[i * m.D + j]; }
template <typename R> __device__ __forceinline__ TransW<R> trans_w(const FkW<R>& m, long long t) {
    const long long D = m.D;
    if (m.Ft) return TransW<R>{m.Ft + t * D * D, m.bt + t * D, m.LQt + t * D * D};
    return TransW<R>{m.F, m.b, m.LQ};
}

// w <- (L L^T)^-1 r (csmc_sweep.h::cho_solve_fixed, runtime dimension, leading dimension D)
template <typename R> __device__ __forceinline__ void cho_solve_w(int D, const R* L, const R* r, R* w) {
    R z[CSW_MAXD];
    for (int k = 0; k < D; ++k) {
        R acc = r[k];
        for (int j = 0; j < k; ++j) acc = fma_(-L[k * D + j], z[j], acc);
        z[k] = acc / L[k * D + k];
    }
    for (int k = D - 1; k >= 0; --k) {
        R acc = z[k];
        for (int j = k + 1; j < D; ++j) acc = fma_(-L[j * D + k], w[j], acc);
        w[k] = acc / L[k * D + k];
    }
}
// the gradient of the model's joint log-density at u (csmc_sweep.h::k_csmc_grad, same operations in the same order; one thread per (chain, time step):
// C T threads of O(dx^2) work, once per sweep -- 0.5 M multiply-adds at the SV protocol's size)
// V: a coupled potential's gradient is a compile-time variant (its z[32] would otherwise add scratch to the kernel of the other potentials); so is the
// Poisson and the logistic potentials', which are component by component like the separable kinds' (csmc_sweep.h::comp_grad_term)
template <typename R, PotV V = PotV::SEP> __global__ void k_cw_grad(CsmcArgs a, FkW<R> m) {
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (long long)a.C * a.T) return;
    const int D = m.D;
    const long long t = g % a.T;
    const R* u = (const R*)a.u + g * D;
    R gr[CSW_MAXD], r[CSW_MAXD], w[CSW_MAXD];
    const R* yv = (const R*)a.y;
    if constexpr (pot_has_matrix(V)) {
        coupled_grad<R, V, 0>(m, m.pot_mat, D, u, yv + t * D, [&](int k, R v) { gr[k] = v; });
    } else if constexpr (pot_has_size(V)) {
        for (int k = 0; k < D; ++k) gr[k] = comp_grad_term<R, V>(m.potential, m.inv_sig_y, u[k], yv[t * D + k], size_at<R>(yv, a.T, t, D, k));
    } else {
        for (int k = 0; k < D; ++k) gr[k] = comp_grad_term<R, V>(m.potential, m.inv_sig_y, u[k], yv ? yv[t * D + k] : (R)0);
    }
    if (t == 0) {
        for (int k = 0; k < D; ++k) r[k] = u[k] - m.m0[k];
        cho_solve_w<R>(D, m.LP0, r, w);
    } else {
        const TransW<R> tr = trans_w<R>(m, t - 1);
        for (int k = 0; k < D; ++k) {
            R acc = tr.b[k];
            for (int j = 0; j < D; ++j) acc = fma_(tr.F[k * D + j], u[j - D], acc);
            r[k] = u[k] - acc;
        }
        cho_solve_w<R>(D, tr.LQ, r, w);
    }
    for (int k = 0; k < D; ++k) gr[k] = gr[k] - w[k];
    if (t + 1 < a.T) {
        const TransW<R> tr = trans_w<R>(m, t);
        for (int k = 0; k < D; ++k) {
            R acc = tr.b[k];
            for (int j = 0; j < D; ++j) acc = fma_(tr.F[k * D + j], u[j], acc);
            r[k] = u[D + k] - acc;
        }
        cho_solve_w<R>(D, tr.LQ, r, w);
        for (int k = 0; k < D; ++k) {
            R acc = 0;
            for (int j = 0; j < D; ++j) acc = fma_(tr.F[j * D + k], w[j], acc);
            gr[k] = gr[k] + acc;
        }
    }
    for (int k = 0; k < D; ++k) ((R*)a.grad)[g * D + k] = gr[k];
}

// value of lane J of MY half-wave: ds_swizzle in bit mode (lane' = (lane & and) | or inside each group of 32 lanes, and = 0, or = J) -- one LDS-crossbar
// instruction, no memory, no scalar round trip (two v_readlane + two v_mov + a select before: the component loops are bound by the CU's instruction issue,
// thirteen waves of one chain walk them together)
template <typename R, int J> __device__ __forceinline__ R half_bcast(R v) {
    if constexpr (sizeof(R) == 4) {
        return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), J << 5));
    } else {
        const int lo_ = __builtin_amdgcn_ds_swizzle(__double2loint(v), J << 5), hi_ = __builtin_amdgcn_ds_swizzle(__double2hiint(v), J << 5);
        return __hiloint2double(hi_, lo_);
    }
}
template <int J, int N, typename F> __device__ __forceinline__ void static_for(F&& f) {
    if constexpr (J < N) {
        f(std::integral_constant<int, J>{});
        static_for<J + 1, N>(f);
    }
}
// sum_k ((x_k - pm_k)^2 - (x_k - u_k)^2) / (2 s^2) of the particle whose component k this lane holds (csmc_sweep.h::grad_correction: the two multiply-adds per
// component, in component order, from broadcasts of the lanes' differences; components beyond D add fma(0, 0, acc) = acc)
template <typename R> __device__ __forceinline__ R grad_corr_half(int D, int k, R xk, R uk, R pmk, R s) {
    const R d1 = k < D ? xk - uk : (R)0, d2 = k < D ? xk - pmk : (R)0;
    R acc = 0;
    static_for<0, CSW_MAXD>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        const R b2 = half_bcast<R, j>(d2), b1 = half_bcast<R, j>(d1);
        acc = fma_(b2, b2, acc);
        acc = fma_(-b1, b1, acc);
    });
    return acc * ((R)0.5 / (s * s));
}
// log N(x; mean, L L^T) of the particle whose component k this lane holds (x - mean in `acc`), column-oriented substitution; L: lane k's row pointer with
// element stride 1 (L[j] = L_kj), iLk = 1 / L_kk.  Every lane of the half-wave returns the same value.
template <typename R> __device__ __forceinline__ R gauss_half(int D, int k, bool hi, R acc, const R* Lrow, R iLk, R cst) {
    R q = 0;
    acc = k < D ? acc : (R)0;  // (components beyond D: z = 0, fma(0, 0, q) = q -- the 32 steps below are the D steps of the contract)
    R l[CSW_MAXD];
#pragma unroll
    for (int j = 0; j < CSW_MAXD; ++j) l[j] = j < D ? Lrow[j] : (R)0;
    static_for<0, CSW_MAXD>([&](auto jc) {  // (straight-line: the row of L requested up front, only the broadcast / multiply-add chain is serial)
        constexpr int j = decltype(jc)::value;
        const R zj = half_bcast<R, j>(acc * iLk);
        q = fma_(zj, zj, q);
        acc = (k > j && k < D) ? fma_(-l[j], zj, acc) : acc;
    });
    return fma_((R)-0.5, q, cst);
}
// The same density with the substitution in BLOCKS OF FOUR columns: one round of four broadcasts hands every lane the accumulators of lanes jb .. jb + 3 (final with
// respect to the columns before jb); every lane then solves the 4 x 4 triangular block for z_jb .. z_jb+3 itself -- the multiply-adds lane jb + a would apply to its own
// accumulator, in the same order, so the same bits -- and applies the four columns to its own accumulator in order.  Eight broadcast latencies per density instead of
// thirty-two (profiles/r03_d_cw2_ablation.txt: the dependent broadcast chain was half of the sweep).  blk: Cw2Lds::blk (uniform reads).
template <typename R> __device__ __forceinline__ R gauss_half_blk(int D, int k, R acc, const R* Lrow, const R* blk, R cst) {
    R q = 0;
    acc = k < D ? acc : (R)0;
    R l[CSW_MAXD];
#pragma unroll
    for (int j = 0; j < CSW_MAXD; ++j) l[j] = Lrow[j];  // (rows are zero-padded to 32 columns)
    static_for<0, CSW_MAXD / 4>([&](auto bc) {
        constexpr int jb = 4 * decltype(bc)::value;
        const R* e = blk + 12 * decltype(bc)::value;
        R a0 = half_bcast<R, jb>(acc), a1 = half_bcast<R, jb + 1>(acc), a2 = half_bcast<R, jb + 2>(acc), a3 = half_bcast<R, jb + 3>(acc);
        const R z0 = a0 * e[6];
        a1 = fma_(-e[0], z0, a1);
        const R z1 = a1 * e[7];
        a2 = fma_(-e[1], z0, a2);
        a2 = fma_(-e[2], z1, a2);
        const R z2 = a2 * e[8];
        a3 = fma_(-e[3], z0, a3);
        a3 = fma_(-e[4], z1, a3);
        a3 = fma_(-e[5], z2, a3);
        const R z3 = a3 * e[9];
        q = fma_(z0, z0, q);
        q = fma_(z1, z1, q);
        q = fma_(z2, z2, q);
        q = fma_(z3, z3, q);
        acc = (k > jb && k < D) ? fma_(-l[jb], z0, acc) : acc;
        acc = (k > jb + 1 && k < D) ? fma_(-l[jb + 1], z1, acc) : acc;
        acc = (k > jb + 2 && k < D) ? fma_(-l[jb + 2], z2, acc) : acc;
        acc = (k > jb + 3 && k < D) ? fma_(-l[jb + 3], z3, acc) : acc;
    });
    return fma_((R)-0.5, q, cst);
}
// a coupled potential of that particle (csmc_sweep.h::coupled_resid / coupled_value, same operations in the same order): with v = r = x - y (MVT) or v = x (LIN) in
// the lane that owns the component, a_k = row k of the potential's matrix (Mrow: this lane's zero-padded LDS row) times v from half-wave broadcasts of v_j, j ascending;
// z_k = a_k (MVT) or yw_k - a_k (LIN); q accumulated in component order by every lane alike from broadcasts of z_k and r_k (MVT) or of z_k alone (LIN).  Columns /
// components beyond D contribute fma(0, 0, acc) = acc.
template <typename R, PotV V> __device__ __forceinline__ R coupled_half(const FkW<R>& m, int k, R xk, R yk, const R* Mrow) {
    constexpr bool MVT = V == PotV::MVT;
    const int D = m.D;
    const R v = k < D ? (MVT ? xk - yk : xk) : (R)0;
    R p[CSW_MAXD];
#pragma unroll
    for (int j = 0; j < CSW_MAXD; ++j) p[j] = Mrow[j];
    R a = 0;
    static_for<0, CSW_MAXD>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        a = fma_(p[j], half_bcast<R, j>(v), a);
    });
    const R z = k < D ? (MVT ? a : yk - a) : (R)0;
    R q = 0;
    static_for<0, CSW_MAXD>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        const R zj = half_bcast<R, j>(z);
        q = fma_(zj, MVT ? half_bcast<R, j>(v) : zj, q);
    });
    if constexpr (MVT) return mvt_value<R>(m.mvt_hc, (R)1 + q * m.mvt_inv_nu);
    else return lin_value<R>(m.c_obs, q);
}
// The logistic potential of that particle (PotV::LOGI), the Poisson shape: the term of this lane's component with its size m_{t,k} -- plane 1 of y,
// csmc_sweep.h::size_at -- then the half-wave broadcast sum in component order.  A function of its own, called under `if constexpr (V == PotV::LOGI)`: the
// call sites of the other variants stay token for token what they were, and so do their kernels' registers.
template <typename R> __device__ __forceinline__ R logistic_half(int D, int k, R xk, R yk, const void* y, int T, long long t) {
    const R v = k < D ? logi_term<R>(xk, yk, size_at<R>((const R*)y, T, t, D, k)) : (R)0;
    R acc = 0;
    static_for<0, CSW_MAXD>([&](auto jc) { acc += half_bcast<R, decltype(jc)::value>(v); });
    return acc;
}
// g_t(x) of that particle, the potential's variant V chosen at compile time.  Separable and Poisson: per-component terms in the lanes, summed in component order
// (csmc_sweep.h::potential with a runtime dimension, same operations; components beyond D add + 0)
template <typename R, PotV V> __device__ __forceinline__ R potential_half(const FkW<R>& m, int k, bool hi, R xk, R yk, const R* Mrow) {
    static_assert(!pot_has_size(V), "the logistic potential reads a size beside yk: logistic_half");
    if constexpr (pot_has_matrix(V)) return coupled_half<R, V>(m, k, xk, yk, Mrow);
    const int D = m.D;
    if constexpr (V == PotV::POIS) {  // SV's shape: the term of this lane's component, then the half-wave broadcast sum in component order
        const R v = k < D ? pois_term<R>(xk, yk) : (R)0;
        R acc = 0;
        static_for<0, CSW_MAXD>([&](auto jc) { acc += half_bcast<R, decltype(jc)::value>(v); });
        return acc;
    }
    if (m.potential == 0) return (R)0;
    if (m.potential == 1 || m.potential == 3) {
        const bool obs = m.potential == 1 || (yk - yk == 0);
        const R z = (k < D && obs) ? (yk - xk) * m.inv_sig_y : (R)0;
        R q = 0;
        static_for<0, CSW_MAXD>([&](auto jc) {
            const R zj = half_bcast<R, decltype(jc)::value>(z);
            q = fma_(zj, zj, q);  // (a missing component, or one beyond D, contributes fma(0, 0, q) = q: the reference skips it)
        });
        if (m.potential == 1) return fma_((R)-0.5, q, m.c_obs);
        const unsigned long long bal = __ballot(k < D && obs);
        const int nobs = __popc((unsigned int)(hi ? bal >> 32 : bal & 0xffffffffull));
        return fma_((R)-0.5, q, (R)nobs * m.c_obs);
    }
    const R e = det_exp(-xk);
    const R sv = fma_(yk * yk, e, xk);
    R v = fma_((R)-0.5, sv, m.c_obs);
    v = (k < D && v == v) ? v : (R)0;
    R acc = 0;
    static_for<0, CSW_MAXD>([&](auto jc) { acc += half_bcast<R, decltype(jc)::value>(v); });
    return acc;
}

// the gradient launch of the wide-state prologue (csmc_host.h::csmc_prologue's grad()): one thread per (chain, time step)
template <typename R> static void cw_grad_launch(auxssm_ctx* h, const CsmcArgs& a, const FkW<R>& m) {
    const dim3 grid((unsigned)(((long long)a.C * a.T + 63) / 64));
    with_pot(m.potential, [&](auto pv) { hipLaunchKernelGGL((k_cw_grad<R, decltype(pv)::value>), grid, dim3(64), 0, h->stream, a, m); });
}
// m <- the model of fk in precision R, its arrays in the handle's device block [m0 | LP0 | iLP0 | F | b | LQ | iLQ | the matrix of a coupled potential]: a new
// upload only when the content differs from the last one.  Defined and explicitly instantiated for float and double in csmc_wide.hip, which owns the handle's
// block: pit_wide.o resolves it against csmc_wide.o when the library is linked
template <typename R> int cw_model(auxssm_ctx* h, const auxssm_fk_model* fk, FkW<R>& m);

}  // namespace ax
