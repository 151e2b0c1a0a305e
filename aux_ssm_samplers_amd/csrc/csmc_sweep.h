// csmc_sweep.h -- the device side of the sequential conditional-SMC sweep (k_csmc_fwd / k_csmc_bwd of csmc.hip) and what the cSMC units share
// with it: the device-side Feynman-Kac model, its densities in fixed operation order, the workgroup reductions whose orders the C oracle
// (oracle/csmc_ref.c) restates, and the forward / backward pass bodies.  Self-contained device code: it compiles under hipcc (through csmc_host.h)
// AND under hipRTC (fk_program.hip: a user-defined model compiled at get_kernel time; rtc_compat.h), so nothing here may include host C++ or ctx.h.
// Units including this are compiled with -ffp-contract=off (hipRTC programs too).
#pragma once
#include "rtc_compat.h"
#include "det_math.h"
#include "rng.h"

namespace ax {

constexpr int CS_MAXD = 4;

template <typename R> struct FkDev {
    int proposal, potential, D, transition;  // transition: 0 = linear-Gaussian (F, b); 1 = Lorenz-63 Euler-Maruyama (theta = F[0][0..2], dt = b[0])
    R m0[CS_MAXD], LP0[CS_MAXD * CS_MAXD], F[CS_MAXD * CS_MAXD], b[CS_MAXD], LQ[CS_MAXD * CS_MAXD];
    R c_init, c_trans, c_obs, inv_sig_y;  // additive constants: -sum log L_kk - D/2 log 2pi, etc.
    R iLP0[CS_MAXD], iLQ[CS_MAXD];        // reciprocal diagonals of LP0 / LQ: the log-densities multiply by them (sweep contract v3)
    // time-varying linear transitions (device arrays, row t = transition t -> t+1; null: the invariant F / b / LQ above); under a ChainDyn policy (below) the
    // same five pointers hold PER-CHAIN rows instead, row c = chain c's time-invariant transition: (C, D, D), (C, D), (C, D, D), (C), (C, D)
    const R* Ft;   // (T-1, D, D)
    const R* bt;   // (T-1, D)
    const R* LQt;  // (T-1, D, D) lower
    const R* ctt;  // (T-1) additive constants of the transition densities (k_csmc_ctrans)
    const R* idt;  // (T-1, D) reciprocal diagonals of LQt (k_csmc_ctrans)
    int gradient;  // AUXSSM_GRAD_*
    // the matrix of a coupled potential (leading dimension CS_MAXD; one potential is live per model) -- AUXSSM_POT_MVT: the precision matrix, with the two constants
    // (nu + D) / 2 and 1 / nu below, formed on the host in R; AUXSSM_POT_LIN_GAUSS: the whitened observation matrix Hw (rows beyond dy zero), with c_lin in c_obs
    R pot_mat[CS_MAXD * CS_MAXD];
    R mvt_hc, mvt_inv_nu;
    AXD_HD constexpr int mat_ld() const { return CS_MAXD; }  // the leading dimension of the struct's matrices
};
// the transition t -> t+1 of the model: matrices through pointers (wave-uniform loads when time-varying)
template <typename R> struct TransT {
    const R* F;
    const R* b;
    const R* LQ;
    int ld;  // leading dimension of F / LQ: CS_MAXD for the struct arrays, D for the device rows
    R c_trans;
    const R* iL;  // reciprocal diagonal of LQ
};
template <typename R, int D> __device__ __forceinline__ TransT<R> trans_at(const FkDev<R>& m, long long t) {
    if (m.Ft) return TransT<R>{m.Ft + t * D * D, m.bt + t * D, m.LQt + t * D * D, D, m.ctt[t], m.idt + t * D};
    return TransT<R>{m.F, m.b, m.LQ, CS_MAXD, m.c_trans, m.iLQ};
}
// the same with the choice made at compile time (the persistent sweep kernels: no branch on the model kind inside the time loop)
template <typename R, int D, bool TV> __device__ __forceinline__ TransT<R> trans_at_c(const FkDev<R>& m, long long t) {
    if constexpr (TV) return TransT<R>{m.Ft + t * D * D, m.bt + t * D, m.LQt + t * D * D, D, m.ctt[t], m.idt + t * D};
    else return TransT<R>{m.F, m.b, m.LQ, CS_MAXD, m.c_trans, m.iLQ};
}
// ---- per-chain, time-invariant transitions (auxssm_csmc_sweep_chain_dynamics: particle Gibbs over (x, F, b, Q)) ----------------------------------------------
// The third source of a TransT: row c of PER-CHAIN device arrays, c the GLOBAL chain.  The model's five pointers then hold F (C, D, D), b (C, D), chol_Q (C, D, D)
// lower, the constants (C) and the reciprocal diagonals (C, D) -- the layout of the time-varying rows with the chain in the place of the time step (the constants
// come from the same k_csmc_ctrans, run over C rows), so that FkDev and every kernel argument keep their layout.  The mode belongs to the model POLICY of a kernel
// (ChainDyn<P>::value, a compile-time constant: FkBuiltinChain below, the built-in family only), never to a run-time test: the kernels of every other policy keep
// their code.  A one-thread-per-(chain, step) kernel reads its row through pointers (trans_chain); a persistent sweep kernel, whose chain is its workgroup, copies
// the row ONCE, before its time loop, into scalar registers (TransC::load: every load is wave-uniform and independent of t), and hands the loop a TransT of that
// copy -- the loop then costs what the shared-parameter kernels' does, not a row of loads per step.
template <typename P> struct ChainDyn { static constexpr bool value = false; };
template <typename R, int D> __device__ __forceinline__ TransT<R> trans_chain(const FkDev<R>& m, long long c) {
    return TransT<R>{m.Ft + c * D * D, m.bt + c * D, m.LQt + c * D * D, D, m.ctt[c], m.idt + c * D};
}
// v, which the caller knows to be the same in every lane, as a scalar-register value
__device__ __forceinline__ float uniform_(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
__device__ __forceinline__ double uniform_(double v) {
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
}
template <typename R, int D> struct TransC {
    R F[D * D], b[D], LQ[D * D], iL[D], c_trans;  // (leading dimension D; the strict upper triangle of LQ is never read and stays unset)
    __device__ __forceinline__ void load(const FkDev<R>& m, long long c) {
        const TransT<R> g = trans_chain<R, D>(m, c);
#pragma unroll
        for (int k = 0; k < D; ++k) {
            b[k] = uniform_(g.b[k]);
            iL[k] = uniform_(g.iL[k]);
#pragma unroll
            for (int j = 0; j < D; ++j) {
                F[k * D + j] = uniform_(g.F[k * D + j]);
                if (j <= k) LQ[k * D + j] = uniform_(g.LQ[k * D + j]);
            }
        }
        c_trans = uniform_(g.c_trans);
    }
    __device__ __forceinline__ TransT<R> trans() const { return TransT<R>{F, b, LQ, D, c_trans, iL}; }
};

struct CsmcArgs {
    int C, T, N, backward;
    const void* y;       // (T, D) shared by chains (may be null for the flat potential)
    const void* shd;     // (T) sqrt(delta_t / 2), AUX proposal only
    void* x;             // (C, T, D) reference trajectory in, new trajectory out
    void* u;             // (C, T, D) auxiliary variables (workspace), AUX only
    void* grad;          // (C, T, D) gradient of the model's joint log-density at u (workspace), gradient proposals only
    void* xs;            // (C, T, N, D)
    void* lws;           // (C, T, N)
    int32_t* As;         // (C, T-1, N) or null
    void* wT;            // (C, N)
    void* fmax;          // (C, T) the shift the forward pass used for the weights of step t (an upper bound of max_i log_ws[t][i], or that maximum;
                         // non-finite -> 0): the backward pass builds its own bound from it (sweep contract)
    const void* gb;      // (T) upper bound of the potential G_t over x (a function of y_t only; +inf where there is none); null: exact maxima only
    int32_t* anc;        // (C, T)
    int noise_mode;      // 0 explicit arrays, 1 Threefry
    int pregen = 0;      // Threefry mode with the forward pass's draws generated into eps_prop / u_res BEFORE the pass (k_csmc_pregen: a sweep with fewer chains than
                         // CUs leaves most of the chip idle while every step of its few workgroups waits for a Threefry block and a Box-Muller pair)
    uint32_t key0, key1;
    const void* eps_aux;   // (C, T, D)
    const void* eps_prop;  // (C, T, N, D)
    const void* u_res;     // (C, T-1, N)
    const void* u_bwd;     // (C, T); with in-kernel draws the sweep fills its own array first (k_csmc_ubwd): the backward kernels always read it
    // chain batching (csmc.hip::auxssm_csmc_sweep): the particle system of one chain is T N (D + 1) reals -- 537 MB at C3 -- so a sweep over more chains
    // than the device holds runs the forward + backward pair batch by batch, [c0, c0 + C) per launch.  Every array above is indexed by the GLOBAL
    // chain c0 + blockIdx.x (so are the random streams: a batched sweep is bit for bit the unbatched one); the workspace-owned xs / lws / As of a
    // batch are passed with their base moved back by c0 records.
    int c0 = 0;
    int cb = 0;                               // host side: chains per batch
    size_t xs_rec = 0, lws_rec = 0, As_rec = 0;  // host side: bytes per chain of the workspace-owned arrays (0: caller-owned, indexed globally anyway)
    const void* gtab = nullptr;  // guided proposals only: the tables of the T steps (GuidedT; csmc_guided.h::k_csmc_gtab); `grad` then holds the shifted u
};

enum { STREAM_EPS_AUX = 1, STREAM_EPS_PROP = 2, STREAM_U_RES = 3, STREAM_U_BWD = 4 };

template <typename R> __device__ __forceinline__ R noise_normal(const CsmcArgs& a, const void* arr, uint32_t stream, long long idx) {
    if (a.noise_mode == 0) return ((const R*)arr)[idx];
    return stream_normal<R>(a.key0, a.key1, stream, (unsigned long long)idx);
}
template <typename R> __device__ __forceinline__ R noise_uniform(const CsmcArgs& a, const void* arr, uint32_t stream, long long idx) {
    if (a.noise_mode == 0) return ((const R*)arr)[idx];
    return stream_uniform<R>(a.key0, a.key1, stream, (unsigned long long)idx);
}

AXD_HD float fma_(float a, float b, float c) { return fmaf(a, b, c); }
AXD_HD double fma_(double a, double b, double c) { return fma(a, b, c); }

// log N(x; mean, L L^T) = cst - 0.5 |L^-1 (x - mean)|^2, forward substitution in a fixed order; iL = the reciprocal diagonal of L, computed once
// per factor (sweep contract v3: a multiplication instead of an IEEE division -- ten instructions -- per particle, component and step)
template <typename R, int D> AXD_HD R gauss_chol_logpdf(const R* x, const R* mean, const R* L, const R* iL, R cst, int ld = CS_MAXD) {
    R z[D];
    R q = 0;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        R acc = x[k] - mean[k];
#pragma unroll
        for (int j = 0; j < k; ++j) acc = fma_(-L[k * ld + j], z[j], acc);
        z[k] = acc * iL[k];
        q = fma_(z[k], z[k], q);
    }
    return fma_((R)-0.5, q, cst);
}
// ---- guided proposals (AUXSSM_PROP_AUX_GUIDED) ------------------------------------------------------------------------------------------------------
// x_t ~ N(mu_t, Lambda_t), mu_t = pred + K_t (u~_t - pred), K_t = P (P + s_t^2 I)^-1, Lambda_t = P - K_t P with pred / P = m0 / P0 at t = 0, the parent's transition
// mean / Q after; weight log g_t(x) + log N(x; pred, P) + sum_k log N(x_k; u_k, s_t^2) - log N(x; mu_t, Lambda_t).  Row t of the table k_csmc_gtab builds per sweep:
template <typename R> struct GuidedT {
    const R *K, *L, *iL;   // K_t (D x D), chol Lambda_t (D x D lower) and its reciprocal diagonal, leading dimension D
    R c_lam, c_u, inv_s;   // the additive constants of N(.; ., Lambda_t) and of sum_k N(.; u_k, s_t^2); 1 / s_t
};
template <typename R> __device__ __forceinline__ GuidedT<R> guided_at(const void* tab, int D, long long t) {
    const R* p = (const R*)tab + t * (2 * D * D + D + 4);
    const R* c = p + 2 * D * D + D;
    return GuidedT<R>{p, p + D * D, p + 2 * D * D, c[0], c[1], c[2]};
}
// mu = pred + K (ut - pred), x = mu + L eps (rows in component order, explicit fma)
template <typename R, int D> __device__ __forceinline__ void guided_propose(const GuidedT<R>& g, const R* pred, const R* ut, const R* eps, R* mu, R* x) {
    R dv[D];
#pragma unroll
    for (int k = 0; k < D; ++k) dv[k] = ut[k] - pred[k];
#pragma unroll
    for (int k = 0; k < D; ++k) {
        R acc = pred[k];
#pragma unroll
        for (int j = 0; j < D; ++j) acc = fma_(g.K[k * D + j], dv[j], acc);
        mu[k] = acc;
    }
#pragma unroll
    for (int k = 0; k < D; ++k) {
        R acc = mu[k];
#pragma unroll
        for (int j = 0; j <= k; ++j) acc = fma_(g.L[k * D + j], eps[j], acc);
        x[k] = acc;
    }
}
// lw + sum_k log N(x_k; u_k, s^2) - log N(x; mu, Lambda)   (lw = log g + log N(x; pred, P))
template <typename R, int D> __device__ __forceinline__ R guided_weight(const GuidedT<R>& g, R lw, const R* x, const R* u, const R* mu) {
    R q = 0;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        const R z = (x[k] - u[k]) * g.inv_s;
        q = fma_(z, z, q);
    }
    lw = lw + fma_((R)-0.5, q, g.c_u);
    return lw - gauss_chol_logpdf<R, D>(x, mu, g.L, g.iL, g.c_lam, D);
}

template <typename R, int D> AXD_HD void trans_mean(const FkDev<R>& m, const R* xp, R* mu);
// mean of the transition tr applied to xp (linear, or the Lorenz-63 Euler-Maruyama step of the invariant model)
template <typename R, int D> __device__ __forceinline__ void trans_mean_t(const FkDev<R>& m, const TransT<R>& tr, const R* xp, R* mu) {
    if (m.transition == 1) {
        trans_mean<R, D>(m, xp, mu);
        return;
    }
#pragma unroll
    for (int k = 0; k < D; ++k) {
        R acc = tr.b[k];
#pragma unroll
        for (int j = 0; j < D; ++j) acc = fma_(tr.F[k * tr.ld + j], xp[j], acc);
        mu[k] = acc;
    }
}
template <typename R, int D> AXD_HD void trans_mean(const FkDev<R>& m, const R* xp, R* mu) {
    if constexpr (D == 3) {
        if (m.transition == 1) {  // x + dt (phi_0(x) + theta * phi(x)), examples/lorenz/model.py:10-25; fixed operation order
            const R th1 = m.F[0], th2 = m.F[1], th3 = m.F[2], dt = m.b[0];
            const R f1 = th1 * (xp[1] - xp[0]);
            const R f2 = fma_(-xp[0], xp[2], fma_(th2, xp[0], -xp[1]));
            const R f3 = fma_(xp[0], xp[1], -(th3 * xp[2]));
            mu[0] = fma_(dt, f1, xp[0]);
            mu[1] = fma_(dt, f2, xp[1]);
            mu[2] = fma_(dt, f3, xp[2]);
            return;
        }
    }
#pragma unroll
    for (int k = 0; k < D; ++k) {
        R acc = m.b[k];
#pragma unroll
        for (int j = 0; j < D; ++j) acc = fma_(m.F[k * CS_MAXD + j], xp[j], acc);
        mu[k] = acc;
    }
}
// ---- the built-in potentials ----------------------------------------------------------------------------------------------------------------------
// The kinds (the values of AUXSSM_POT_* of include/auxssm.h, which hipRTC cannot include: csmc_host.h asserts that they agree) and their compile-time VARIANT:
// the separable kinds share one code path and are told apart at run time inside it; a potential that couples the components through a dx x dx matrix
// (FkDev::pot_mat) is a variant of its own, so that the instantiations of the other potentials hold none of its code -- as a fifth run-time branch the
// multivariate-t potential cost every forward instantiation twelve registers in fp64 and a wave of occupancy.  The Poisson count potential is
// separable like kinds 0 - 3 but a variant of its own for the same reason: the instantiations of the other potentials stay as they were.  So is the logistic
// potential (binomial / negative-binomial counts), the one kind with a second per-observation number, the size m_{t,k}: for it CsmcArgs::y is (2, T, D),
// plane 0 the data and plane 1 the sizes, and the kernels read plane 1 at y[(T + t) D + k] under `V == PotV::LOGI` alone (size_at below).  Kind 7 is unassigned.
enum { POT_FLAT = 0, POT_GAUSS_OBS = 1, POT_SV = 2, POT_GAUSS_OBS_MASKED = 3, POT_MVT = 4, POT_LIN_GAUSS = 5, POT_POISSON = 6, POT_LOGISTIC = 8 };
// separable (kinds 0 - 3) | multivariate Student-t | linear-Gaussian observation | Poisson counts | logistic (binomial / negative-binomial) counts
enum class PotV { SEP, MVT, LIN, POIS, LOGI };
template <PotV V> struct PotC { static constexpr PotV value = V; };
AXD_HD constexpr PotV pot_variant(int kind) {
    return kind == POT_MVT ? PotV::MVT : (kind == POT_LIN_GAUSS ? PotV::LIN : (kind == POT_POISSON ? PotV::POIS : (kind == POT_LOGISTIC ? PotV::LOGI : PotV::SEP)));
}
// whether the variant reads a size beside every observation (plane 1 of y)
AXD_HD constexpr bool pot_has_size(PotV v) { return v == PotV::LOGI; }
// the size m_{t,k} of the logistic potential: plane 1 of the (2, T, D) array y
template <typename R> AXD_HD R size_at(const R* y, long long T, long long t, int D, int k) { return y[(T + t) * D + k]; }
// whether the variant carries a dx x dx matrix (FkDev / FkW::pot_mat; the wide kernels stage it in LDS): the coupled potentials
AXD_HD constexpr bool pot_has_matrix(PotV v) { return v == PotV::MVT || v == PotV::LIN; }
// f(PotC<V>{}) for the variant V of a run-time kind: the ONE place a kind becomes a template argument (host: the kernel choices; device: potential_rt)
template <typename F> AXD_HD auto with_pot(int kind, F&& f) {
    if (pot_variant(kind) == PotV::MVT) return f(PotC<PotV::MVT>{});
    if (pot_variant(kind) == PotV::LIN) return f(PotC<PotV::LIN>{});
    if (pot_variant(kind) == PotV::POIS) return f(PotC<PotV::POIS>{});
    if (pot_variant(kind) == PotV::LOGI) return f(PotC<PotV::LOGI>{});
    return f(PotC<PotV::SEP>{});
}

constexpr int CS_MAXD_RT = 32;  // the widest state of a caller with a run-time dimension (csmc_wide.hip, csmc_guided.h)
// f(k) for k = 0 .. D - 1, D = DC when the dimension is a compile-time constant (DC > 0: the register kernels, fully unrolled) and d otherwise
template <int DC, typename F> AXD_HD void for_dim(int d, F&& f) {
    if constexpr (DC > 0) {
#pragma unroll
        for (int k = 0; k < DC; ++k) f(k);
    } else {
        for (int k = 0; k < d; ++k) f(k);
    }
}
// The coupled potentials, the ONE definition of their arithmetic: every kernel family calls it (the register kernels with DC = D, the wide-state gradient and the
// guided shift with DC = 0 and the run-time dimension m.D; the half-wave form of csmc_wide.hip::coupled_half lays the same operations across lanes).  A: the
// potential's matrix, leading dimension ld (CS_MAXD for FkDev, D for csmc_wide.hip's FkW); m: the model, for the constants.  The order is include/auxssm.h's:
//   MVT (examples/spatial/t_distribution.py:98-104 with model.py:121-124; A = the precision matrix):  r = x - y;  z = A r (row k: fma over j ascending from 0);
//       q = sum_k fma(z_k, r_k, .) (k ascending from 0);  s = 1 + q / nu.  Value -((nu + D) / 2) det_log(s) with NaN -> 0; gradient component k = c z_k with
//       c = -(hc + hc) inv_nu / s = -(nu + D) / (nu + q), every component 0 where s is NaN (a missing observation: the step is flat).
//   LIN (log N(y_t; H x + c, R) whitened on the host into c_lin - |yw_t - Hw x|^2 / 2; A = Hw, dx x dx with zero rows beyond dy, yw zero beyond dy: those
//       components add fma(0, 0, .)):  a_k = row k of A times x (fma over j ascending from 0);  z_k = yw_k - a_k;  q = sum_k fma(z_k, z_k, .) (k ascending from 0).
//       Value c_lin - q / 2 with NaN -> 0 (a missing observation row is all NaN); gradient A^T z (component j: fma over k ascending from 0), every component 0
//       where the value is NaN.
// coupled_resid leaves z and returns s (MVT) or q (LIN).
template <typename R, PotV V, int DC> AXD_HD R coupled_resid(int d, const R* A, int ld, R inv_nu, const R* x, const R* y, R* z) {
    R q = 0;
    if constexpr (V == PotV::MVT) {
        R r[DC > 0 ? DC : CS_MAXD_RT];
        for_dim<DC>(d, [&](int k) { r[k] = x[k] - y[k]; });
        for_dim<DC>(d, [&](int k) {
            R acc = 0;
            for_dim<DC>(d, [&](int j) { acc = fma_(A[k * ld + j], r[j], acc); });
            z[k] = acc;
        });
        for_dim<DC>(d, [&](int k) { q = fma_(z[k], r[k], q); });
        return (R)1 + q * inv_nu;
    } else {
        for_dim<DC>(d, [&](int k) {
            R acc = 0;
            for_dim<DC>(d, [&](int j) { acc = fma_(A[k * ld + j], x[j], acc); });
            z[k] = y[k] - acc;
        });
        for_dim<DC>(d, [&](int k) { q = fma_(z[k], z[k], q); });
        return q;
    }
}
template <typename R> AXD_HD R mvt_value(R hc, R s) {
    const R v = -hc * det_log(s);
    return (v == v) ? v : (R)0;
}
template <typename R> AXD_HD R lin_raw(R c_lin, R q) { return fma_((R)-0.5, q, c_lin); }  // (q / 2 is exact: this is c_lin - q / 2 rounded once)
template <typename R> AXD_HD R lin_value(R c_lin, R q) {
    const R v = lin_raw<R>(c_lin, q);
    return (v == v) ? v : (R)0;
}
template <typename R, PotV V, int DC, typename M> AXD_HD R coupled_value(const M& m, const R* A, int ld, const R* x, const R* y) {
    R z[DC > 0 ? DC : CS_MAXD_RT];
    if constexpr (V == PotV::MVT) return mvt_value<R>(m.mvt_hc, coupled_resid<R, V, DC>(m.D, A, ld, m.mvt_inv_nu, x, y, z));
    else return lin_value<R>(m.c_obs, coupled_resid<R, V, DC>(m.D, A, ld, m.mvt_inv_nu, x, y, z));
}
// the gradient at x, component by component: out(k, d log g / d x_k)
template <typename R, PotV V, int DC, typename M, typename O> AXD_HD void coupled_grad(const M& m, const R* A, int ld, const R* x, const R* y, O&& out) {
    R z[DC > 0 ? DC : CS_MAXD_RT];
    const R sq = coupled_resid<R, V, DC>(m.D, A, ld, m.mvt_inv_nu, x, y, z);
    if constexpr (V == PotV::MVT) {
        const R c = -((m.mvt_hc + m.mvt_hc) * m.mvt_inv_nu) / sq;
        for_dim<DC>(m.D, [&](int k) { out(k, (sq == sq) ? c * z[k] : (R)0); });
    } else {
        const R v = lin_raw<R>(m.c_obs, sq);
        for_dim<DC>(m.D, [&](int j) {
            R acc = 0;
            for_dim<DC>(m.D, [&](int k) { acc = fma_(A[k * ld + j], z[k], acc); });
            out(j, (v == v) ? acc : (R)0);
        });
    }
}
// d / dx_k of a separable potential (kinds 0 - 3: sums over the components): the ONE definition (potential_grad, csmc_wide.hip::k_cw_grad, csmc_guided.h::k_csmc_gshift)
template <typename R> AXD_HD R sep_grad_term(int kind, R inv_sig_y, R xk, R yk) {
    R v = 0;
    if (kind == POT_GAUSS_OBS || (kind == POT_GAUSS_OBS_MASKED && yk - yk == 0)) v = ((yk - xk) * inv_sig_y) * inv_sig_y;
    else if (kind == POT_SV) {
        const R e = det_exp(-xk);
        v = (R)0.5 * fma_(yk * yk, e, (R)-1);
        v = (v == v) ? v : (R)0;
    }
    return v;
}
// The Poisson count potential y_k ~ Poisson(exp(x_k)), the ONE definition of its per-component arithmetic (include/auxssm.h: the order; the -log y_k! constant is
// left out): the term y_k x_k - e^{x_k} and its derivative y_k - e^{x_k}, both 0 for a missing (non-finite) y_k.  Every kernel family sums the terms over k
// ascending from 0 (the wide kernels from half-wave broadcasts: csmc_wide_shared.h::potential_half).
template <typename R> AXD_HD R pois_term(R xk, R yk) {
    const R e = det_exp(xk);
    const R v = fma_(yk, xk, -e);
    return (yk - yk == 0) ? v : (R)0;
}
template <typename R> AXD_HD R pois_grad_term(R xk, R yk) { return (yk - yk == 0) ? yk - det_exp(xk) : (R)0; }
// The logistic potential (binomial counts with m_k trials, y_k ~ Bin(m_k, sigma(x_k)); negative-binomial counts y_k ~ NB(r, p = sigma(x_k)) with m_k = y_k + r),
// the ONE definition of its per-component arithmetic (include/auxssm.h: the order; the combinatorial constant is left out): the term y_k x_k - m_k softplus(x_k)
// and its derivative y_k - m_k sigma(x_k), both 0 for a missing (non-finite) y_k whatever m_k is.  e = det_exp(-|x_k|) <= 1, so nothing overflows at any x_k.
// There is no det_log1p: det_log(1 + e) rounds 1 + e first, an ABSOLUTE error of at most half an ulp of 1 in softplus (2^-24 in fp32, 2^-53 in fp64), i.e. of
// m_k ulp / 2 in a log-weight (DESIGN 4q holds the measurement against logaddexp).
template <typename R> AXD_HD R logi_term(R xk, R yk, R mk) {
    const R e = det_exp(-(xk < (R)0 ? -xk : xk));
    const R l = det_log((R)1 + e);
    const R sp = (xk > (R)0 ? xk : (R)0) + l;
    const R v = fma_(yk, xk, -(mk * sp));
    return (yk - yk == 0) ? v : (R)0;
}
template <typename R> AXD_HD R logi_grad_term(R xk, R yk, R mk) {
    const R e = det_exp(-(xk < (R)0 ? -xk : xk));
    const R r = (R)1 / ((R)1 + e);
    const R s = xk >= (R)0 ? r : e * r;
    return (yk - yk == 0) ? fma_(-mk, s, yk) : (R)0;
}
// d / dx_k of a potential that is a sum over the components, by variant (SEP: the run-time kind of sep_grad_term; POIS; LOGI, the one that reads the size mk):
// k_cw_grad, k_csmc_gshift_pois / _logi
template <typename R, PotV V> AXD_HD R comp_grad_term(int kind, R inv_sig_y, R xk, R yk, R mk = (R)0) {
    static_assert(!pot_has_matrix(V), "a coupled potential's gradient is not component by component (coupled_grad)");
    if constexpr (V == PotV::POIS) return pois_grad_term<R>(xk, yk);
    else if constexpr (V == PotV::LOGI) return logi_grad_term<R>(xk, yk, mk);
    else return sep_grad_term<R>(kind, inv_sig_y, xk, yk);
}
// potential g_t(x_t) (csmc test fixtures test_csmc/common.py:52-75; SV examples/stochastic_volatility/auxiliary_csmc.py:40-46) of the variant V, chosen at
// COMPILE time; potential_rt below is the run-time choice for the callers that are not register-bound.  sz: the D sizes of row t, read by the logistic variant alone
template <typename R, int D, PotV V = PotV::SEP> AXD_HD R potential(const FkDev<R>& m, const R* x, const R* y, const R* sz = nullptr) {
    if constexpr (pot_has_matrix(V)) return coupled_value<R, V, D>(m, m.pot_mat, CS_MAXD, x, y);
    if constexpr (V == PotV::LOGI) {
        R acc = 0;
#pragma unroll
        for (int k = 0; k < D; ++k) acc += logi_term<R>(x[k], y[k], sz[k]);
        return acc;
    }
    if constexpr (V == PotV::POIS) {
        R acc = 0;
#pragma unroll
        for (int k = 0; k < D; ++k) acc += pois_term<R>(x[k], y[k]);
        return acc;
    }
    if (m.potential == POT_FLAT) return (R)0;
    if (m.potential == POT_GAUSS_OBS) {  // y ~ N(x, sig_y^2 I)
        R q = 0;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            const R z = (y[k] - x[k]) * m.inv_sig_y;
            q = fma_(z, z, q);
        }
        return fma_((R)-0.5, q, m.c_obs);
    }
    if (m.potential == POT_GAUSS_OBS_MASKED) {  // y_k ~ N(x_k, sig_y^2) for the finite y_k only (missing components / whole missing steps are skipped)
        R q = 0;
        int nobs = 0;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            if (y[k] - y[k] == 0) {
                const R z = (y[k] - x[k]) * m.inv_sig_y;
                q = fma_(z, z, q);
                ++nobs;
            }
        }
        return fma_((R)-0.5, q, (R)nobs * m.c_obs);
    }
    // stochastic volatility: y_k ~ N(0, exp(x_k)):  -0.5 (y^2 e^{-x} + x) - 0.5 log 2pi, NaN terms -> 0
    R acc = 0;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        const R e = det_exp(-x[k]);
        const R s = fma_(y[k] * y[k], e, x[k]);
        const R v = fma_((R)-0.5, s, m.c_obs);
        acc += (v == v) ? v : (R)0;
    }
    return acc;
}
// gx = d potential / dx at x (the closed family's potentials do not read x_{t-1}); y = the D reals of row t, or nullptr; sz = the D sizes of row t (logistic only)
template <typename R, int D, PotV V = PotV::SEP>
__device__ __forceinline__ void potential_grad(const FkDev<R>& m, const R* x, const R* y, R* gx, const R* sz = nullptr) {
    if constexpr (pot_has_matrix(V)) {
        coupled_grad<R, V, D>(m, m.pot_mat, CS_MAXD, x, y, [&](int k, R v) { gx[k] = v; });
    } else if constexpr (V == PotV::LOGI) {
#pragma unroll
        for (int k = 0; k < D; ++k) gx[k] = logi_grad_term<R>(x[k], y[k], sz[k]);
    } else {
#pragma unroll
        for (int k = 0; k < D; ++k) gx[k] = comp_grad_term<R, V>(m.potential, m.inv_sig_y, x[k], y ? y[k] : (R)0);
    }
}
// the potential kind of m at run time, the coupled variants included (the parallel-in-time kernels, a user program that keeps the built-in potential)
template <typename R, int D> __device__ __forceinline__ R potential_rt(const FkDev<R>& m, const R* x, const R* y, const R* sz) {
    return with_pot(m.potential, [&](auto pv) { return potential<R, D, decltype(pv)::value>(m, x, y, sz); });
}
template <typename R, int D> __device__ __forceinline__ void potential_grad_rt(const FkDev<R>& m, const R* x, const R* y, R* gx, const R* sz) {
    with_pot(m.potential, [&](auto pv) { potential_grad<R, D, decltype(pv)::value>(m, x, y, gx, sz); });
}
// sz <- the D sizes of step t when the model's potential is the logistic one (the callers whose kind is a run-time value), zeros otherwise
template <typename R, int D> __device__ __forceinline__ void size_row_rt(const FkDev<R>& m, const R* y, long long T, long long t, R* sz) {
#pragma unroll
    for (int k = 0; k < D; ++k) sz[k] = m.potential == POT_LOGISTIC ? size_at<R>(y, T, t, D, k) : (R)0;
}
// out = J^T v, J = d mean / d xp of the transition tr (trans_mean_t): F^T, or the Lorenz-63 step's I + dt dphi/dx (examples/lorenz/model.py:10-25)
template <typename R, int D> __device__ __forceinline__ void trans_mean_vjp_t(const FkDev<R>& m, const TransT<R>& tr, const R* xp, const R* v, R* out) {
    if constexpr (D == 3) {
        if (m.transition == 1) {
            const R th1 = m.F[0], th2 = m.F[1], th3 = m.F[2], dt = m.b[0];
            const R J[9] = {-th1, th1, (R)0, th2 - xp[2], (R)-1, -xp[0], xp[1], xp[0], -th3};
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                R acc = 0;
#pragma unroll
                for (int j = 0; j < 3; ++j) acc = fma_(J[j * 3 + k], v[j], acc);
                out[k] = fma_(dt, acc, v[k]);
            }
            return;
        }
    }
#pragma unroll
    for (int k = 0; k < D; ++k) {
        R acc = 0;
#pragma unroll
        for (int j = 0; j < D; ++j) acc = fma_(tr.F[j * tr.ld + k], v[j], acc);
        out[k] = acc;
    }
}
// w <- (L L^T)^-1 r, L lower with leading dimension ld; fixed operation order (restated by oracle/csmc_ref.c::cho_solve_)
template <typename R, int D> __device__ __forceinline__ void cho_solve_fixed(const R* L, int ld, const R* r, R* w) {
    R z[D];
#pragma unroll
    for (int k = 0; k < D; ++k) {
        R acc = r[k];
#pragma unroll
        for (int j = 0; j < k; ++j) acc = fma_(-L[k * ld + j], z[j], acc);
        z[k] = acc / L[k * ld + k];
    }
#pragma unroll
    for (int k = D - 1; k >= 0; --k) {
        R acc = z[k];
#pragma unroll
        for (int j = k + 1; j < D; ++j) acc = fma_(-L[j * ld + k], w[j], acc);
        w[k] = acc / L[k * ld + k];
    }
}

// ---- block primitives (TB threads = NW waves) ---------------------------------------------------------------------
template <typename R> __device__ __forceinline__ R wave_max(R v) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const R o = __shfl_xor(v, off, 64);
        v = v > o ? v : o;  // NaN-agnostic: weights are never NaN for valid models
    }
    return v;
}
template <typename R> __device__ __forceinline__ R wave_sum_tree(R v) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off, 64);
    return v;
}
template <typename R> __device__ __forceinline__ R wave_scan_ks(R v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const R o = __shfl_up(v, off, 64);
        if (lane >= off) v += o;
    }
    return v;
}

// the up-to-16 per-wave partials of a block reduction, fetched with wide LDS reads into registers (same values, same
// left-to-right combination order as a scalar loop over red[]; only the dependent LDS round trips disappear)
template <typename R> __device__ __forceinline__ void load16(const R* red, R* t) {
#pragma unroll
    for (int k = 0; k < 16; ++k) t[k] = red[k];
}

// normalize (math/utils.py:23-39): w = exp(lw - logsumexp(lw)); logsumexp = log(sum(exp(lw - max))) + max
// red: 48 slots (max in [0,16), sum in [16,32), scan totals in [32,48)); slots of unused waves are never read.
template <typename R> __device__ __forceinline__ R block_normalize(R lw, R* red, int tid, int nw) {
    const int lane = tid & 63, wv = tid >> 6;
    R m = wave_max(lw);
    if (lane == 0) red[wv] = m;
    __syncthreads();
    R t[16];
    load16<R>(red, t);
    m = t[0];
    if (nw == 16) {  // full workgroup: no per-slot masks
#pragma unroll
        for (int k = 1; k < 16; ++k) m = t[k] > m ? t[k] : m;
    } else {
#pragma unroll
        for (int k = 1; k < 16; ++k) m = (k < nw && t[k] > m) ? t[k] : m;
    }
    if (!(m - m == 0)) m = 0;  // non-finite max -> 0 (jax logsumexp)
    const R e = det_exp(lw - m);
    R s = wave_sum_tree(e);
    if (lane == 0) red[16 + wv] = s;
    __syncthreads();
    load16<R>(red + 16, t);
    s = t[0];
    if (nw == 16) {
#pragma unroll
        for (int k = 1; k < 16; ++k) s = s + t[k];
    } else {
#pragma unroll
        for (int k = 1; k < 16; ++k) s = k < nw ? s + t[k] : s;
    }
    const R lse = det_log(s) + m;
    return det_exp(lw - lse);
}

// inclusive cumsum of w into c[] (slots [32,48) of red hold the wave totals); c[] valid after the trailing barrier
template <typename R> __device__ __forceinline__ void block_cumsum(R w, R* c, R* red, int tid, int nw) {
    const int lane = tid & 63, wv = tid >> 6;
    const R v = wave_scan_ks(w, lane);
    if (lane == 63) red[32 + wv] = v;
    __syncthreads();
    R t[16];
    load16<R>(red + 32, t);
    R pre = t[0];
#pragma unroll
    for (int k = 1; k < 16; ++k) pre = k < wv ? pre + t[k] : pre;
    c[tid] = wv > 0 ? pre + v : v;
    __syncthreads();
}

// first index j in [0, n) with c[j] >= r  (jnp.searchsorted side='left'); n if none
template <typename R> __device__ __forceinline__ int lower_bound(const R* c, int n, R r) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (c[mid] < r) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// ---- sweep contract (k_csmc_fwd / k_csmc_bwd of csmc.hip; restated by oracle/csmc_ref.c::csmc_ref_sweep) ---------------------------
// The sequential sweep carries UNNORMALISED weights e_i = exp(lw_i - max lw): conditional multinomial resampling only ever uses
// searchsorted(cumsum(w), c[-1] (1 - u)) (resamplings.py:35-36 -> jax.random.choice), which is invariant to the scale of w, so the
// normaliser of normalize() (math/utils.py:38-39: one block sum, one log and one more exp per particle and step) is never formed.
//   cumsum : inside each group of 64 consecutive particles the DPP scan of the hardware -- Kogge-Stone with offsets 1, 2, 4, 8 inside
//            every row of 16 lanes, then row 1 += last of row 0 and row 3 += last of row 2, then rows 2 and 3 += last of row 1; the (up to 16)
//            group totals, padded with +0, prefix-summed by the same Kogge-Stone network on one row of 16 lanes (v3): c_i = P[g - 1] + local_i.
//   search : branch-free lower bound by descent over the whole array (v3): pos = 0; for s = S0, S0 / 2, ..., 1 (S0 the largest power of two
//            below N): if (pos + s - 1 < N and c[pos + s - 1] < r) pos += s; clipped to N - 1.  On a non-decreasing c this IS
//            searchsorted(c, r, side='left').
//   densities : Gaussian log-densities multiply by the reciprocal diagonal of the Cholesky factor, computed once per factor (v3).
//   single draw (backward pass): B = 64 g + #{l < 64 : c_{64 g + l} < r}, g = #{k < ng - 1 : P[k] < r}, clipped to N - 1 (v3; again searchsorted
//            on a non-decreasing c): every wave finds g and counts inside the group by ballot -- one barrier per backward step.
//   shifts   : the weights of a step are e_i = exp(lw_i - M) with M an upper bound of max_i lw_i that needs NO reduction where one exists, the
//            exact maximum otherwise, and the exact maximum after all whenever every e_i underflowed (cumulative total not > 0: detected where
//            the total is formed -- one step later in the forward pass, in the same step in the backward pass).  Scale-invariant as above.
//            Forward, 1 <= t < T - 1, not the exact-gradient proposals: M_t = gb_t (+ c_t for the auxiliary proposals), gb_t = sup_x G_t(x)
//            (csmc_host.h::k_csmc_potbound: 0 | c_obs | nobs c_obs | sum_k max(0, c_obs - (1 + log y_k^2) / 2); +inf -> no bound), c_t the log-normaliser
//            of the transition density; t = 0 and t = T - 1 use the exact maximum.  fmax[t] = the shift finally used.
//            Backward: lw_i = log_ws[t][i] + log p(x_{t+1} | x_t^i) <= M := fmax[t] + c_t.
//   max    : exact, any order.
template <int CTRL, int ROW_MASK> __device__ __forceinline__ float dpp_mov(float old, float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(v), CTRL, ROW_MASK, 0xf, false));
}
template <int CTRL, int ROW_MASK> __device__ __forceinline__ double dpp_mov(double old, double v) {
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(old), __double2loint(v), CTRL, ROW_MASK, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(old), __double2hiint(v), CTRL, ROW_MASK, 0xf, false);
    return __hiloint2double(hi, lo);
}
constexpr int DPP_ROW_SHR1 = 0x111, DPP_ROW_SHR2 = 0x112, DPP_ROW_SHR4 = 0x114, DPP_ROW_SHR8 = 0x118, DPP_ROW_BCAST15 = 0x142, DPP_ROW_BCAST31 = 0x143;
// inclusive scan of the wave in the order stated above (lanes without a source add +0)
template <typename R> __device__ __forceinline__ R wave_scan_dpp(R v) {
    v = v + dpp_mov<DPP_ROW_SHR1, 0xf>((R)0, v);
    v = v + dpp_mov<DPP_ROW_SHR2, 0xf>((R)0, v);
    v = v + dpp_mov<DPP_ROW_SHR4, 0xf>((R)0, v);
    v = v + dpp_mov<DPP_ROW_SHR8, 0xf>((R)0, v);
    v = v + dpp_mov<DPP_ROW_BCAST15, 0xa>((R)0, v);
    v = v + dpp_mov<DPP_ROW_BCAST31, 0xc>((R)0, v);
    return v;
}
// max of the wave, in every lane (exact: the order is immaterial)
template <typename R> __device__ __forceinline__ R wave_max_dpp(R v) {
    R o;
    o = dpp_mov<DPP_ROW_SHR1, 0xf>(v, v); v = v > o ? v : o;
    o = dpp_mov<DPP_ROW_SHR2, 0xf>(v, v); v = v > o ? v : o;
    o = dpp_mov<DPP_ROW_SHR4, 0xf>(v, v); v = v > o ? v : o;
    o = dpp_mov<DPP_ROW_SHR8, 0xf>(v, v); v = v > o ? v : o;
    o = dpp_mov<DPP_ROW_BCAST15, 0xa>(v, v); v = v > o ? v : o;
    o = dpp_mov<DPP_ROW_BCAST31, 0xc>(v, v); v = v > o ? v : o;
    return __shfl(v, 63, 64);  // lane 63 holds the maximum of the wave
}
// e_i = exp(lw_i - max lw) (non-finite max -> 0, as jax's logsumexp); red slots [0, 16).
// NW = 8 / 16: the workgroup is exactly NW full waves (N = 64 NW particles) -- no per-group bounds selects, the NW wave maxima are reduced by
// one more DPP pass instead of fifteen compare / select pairs per lane.
template <typename R, int NW = 0> __device__ __forceinline__ R block_expmax(R lw, R* red, int tid, int nw, R* m_out = nullptr) {
    const int lane = tid & 63, wv = tid >> 6;
    R m = wave_max_dpp(lw);
    if constexpr (NW > 0) {
        if (lane == 0) red[wv] = m;
        __syncthreads();
        m = wave_max_dpp(red[lane & (NW - 1)]);
    } else if (nw > 1) {
        if (lane == 0) red[wv] = m;
        __syncthreads();
        R t[16];
        load16<R>(red, t);
        m = t[0];
#pragma unroll
        for (int k = 1; k < 16; ++k) m = (k < nw && t[k] > m) ? t[k] : m;
    }
    if (!(m - m == 0)) m = 0;
    if (m_out) *m_out = m;
    return det_exp(lw - m);
}
// lane `l` (wave-uniform) of v
__device__ __forceinline__ float readlane_(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }
__device__ __forceinline__ double readlane_(double v, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}
// Sweep contract v3 (round 3), the prefix over the (up to 16) group totals: every wave reads the totals into lanes 0..15 (all four rows alike; slots of
// absent groups hold +0 -- the kernels zero red[32 .. 48) once) and scans them with the Kogge-Stone network of one DPP row (offsets 1, 2, 4, 8).  Lane k then
// holds P[k]; a wave's own base is ONE readlane -- no dependent left-to-right adds, no branch on the wave id (31 branches per wave and step before).
//   base = P[wv - 1] (0 for the first wave);   tot = P[last - 1] + t[last] = c[N - 1] bit for bit (the last live particle's cumulative weight)
template <typename R> __device__ __forceinline__ void totals_prefix(const R* red, int lane, int wv, int last, R& pre, R& tot, R* Pv = nullptr) {
    const R tv = red[32 + (lane & 15)];
    R v = tv;
    v = v + dpp_mov<DPP_ROW_SHR1, 0xf>((R)0, v);
    v = v + dpp_mov<DPP_ROW_SHR2, 0xf>((R)0, v);
    v = v + dpp_mov<DPP_ROW_SHR4, 0xf>((R)0, v);
    v = v + dpp_mov<DPP_ROW_SHR8, 0xf>((R)0, v);
    const int wvu = __builtin_amdgcn_readfirstlane(wv);
    pre = wvu > 0 ? readlane_(v, wvu > 0 ? wvu - 1 : 0) : (R)0;
    tot = last > 0 ? readlane_(v, last > 0 ? last - 1 : 0) + readlane_(tv, last) : readlane_(tv, 0);
    if (Pv) *Pv = v;
}
// The single draw of the backward pass (sweep contract v3): B = 64 g + #{l < 64 : c_{64 g + l} < r}, g = #{k < ng - 1 : P[k] < r} -- on a non-decreasing c
// exactly #{j : c_j < r} = searchsorted(c, r).  Every wave finds g from the totals' prefix it holds in lanes 0..15 (one ballot) and counts inside group g from
// the group's LOCAL scan values, which each wave left in LDS before the one barrier of the step: no second barrier, no exchange of per-wave counts.
//   vloc: this step's image of the local scan values (64 per group); Pv: totals_prefix's lane vector; ng groups; returns B clipped to N - 1
template <typename R> __device__ __forceinline__ int draw_two_level(const R* vloc, R Pv, int lane, int ng, int N, R r) {
    const unsigned long long below = __ballot(Pv < r);
    const unsigned long long mask = ng > 1 ? ((1ull << (ng - 1)) - 1ull) : 0ull;
    const int g = __popcll(below & mask);  // (wave-uniform)
    const int gu = __builtin_amdgcn_readfirstlane(g);
    const R base = gu > 0 ? readlane_(Pv, gu > 0 ? gu - 1 : 0) : (R)0;
    const int j = 64 * gu + lane;
    const R vl = vloc[j];
    const R cg = gu > 0 ? base + vl : vl;
    const int cntg = __popcll(__ballot(j < N && cg < r));
    const int B = 64 * gu + cntg;
    return B < N - 1 ? B : N - 1;
}
// inclusive cumsum of w into c[] in the sweep contract's order; tot = c[N - 1]; c[] valid after the trailing barrier.  red slots [32, 48).
// PAD: c[] is stored with one spare slot per 32 entries (index cpad(i) = i + (i >> 5)): the probes of the search below sit at strides of 512 .. 1
// entries, which without the padding fall into one or two LDS banks (a 16- to 32-way conflict on the later probes of every lane).
__host__ __device__ __forceinline__ constexpr int cpad(int i) { return i + (i >> 5); }
template <typename R, int NW = 0, bool PAD = false> __device__ __forceinline__ void block_cumsum_dpp(R w, R* c, R* red, int tid, int nw, R& tot) {
    const int lane = tid & 63, wv = tid >> 6;
    const R v = wave_scan_dpp(w);
    if (lane == 63) red[32 + wv] = v;
    __syncthreads();
    R pre;
    totals_prefix<R>(red, lane, wv, (NW > 0 ? NW : nw) - 1, pre, tot);
    c[PAD ? cpad(tid) : tid] = wv > 0 ? pre + v : v;
    __syncthreads();
}
// the ancestor search of the sweep contract (v3): branch-free lower bound by descent over the whole cumulative-weight array.  On the padded image of a full
// workgroup every probe is one LDS read at (running padded position + constant): while pos stays a multiple of 2 s, cpad(pos + s - 1) =
// cpad(pos) + (s - 1) + ((s - 1) >> 5), and taking the step adds s + (s >> 5).
template <typename R, int NW = 0, bool PAD = false> __device__ __forceinline__ int search2(const R* c, int N, R r) {
    if constexpr (NW > 0 && PAD) {
        // TWO levels of the descent per LDS round trip: the probe of step s and BOTH candidate probes of step s / 2 (after a step not taken / taken) are three
        // reads at constant offsets from the same position, issued together; the comparisons are exactly those of the one-level descent, in its order
        // (ten dependent LDS latencies per search were the longest chain of the forward step)
        int ppos = 0;
        constexpr int S0 = NW * 32;
        static_assert((S0 & (S0 - 1)) == 0, "the two-level descent needs a power-of-two particle count");
        constexpr int LEVELS = 32 - __builtin_clz((unsigned)S0);  // steps S0, S0 / 2, ..., 1
        constexpr bool ODD = (LEVELS & 1) != 0;  // an odd number of levels (9 at N = 512, 7 at N = 128): the first one alone, the rest in pairs
        if constexpr (ODD) ppos += c[ppos + (S0 - 1) + ((S0 - 1) >> 5)] < r ? S0 + (S0 >> 5) : 0;
#pragma unroll
        for (int s = ODD ? S0 / 2 : S0; s >= 2; s >>= 2) {
            const int h = s >> 1;
            const int ks = (s - 1) + ((s - 1) >> 5), kh = (h - 1) + ((h - 1) >> 5), ps = s + (s >> 5), ph = h + (h >> 5);
            const R A = c[ppos + ks], B0 = c[ppos + kh], B1 = c[ppos + ps + kh];
            const bool a = A < r;
            const bool b = (a ? B1 : B0) < r;
            ppos += (a ? ps : 0) + (b ? ph : 0);
        }
        const int pos = ppos - ((ppos * 1986) >> 16);  // ppos = 33 (pos >> 5) + (pos & 31)
        return pos < N - 1 ? pos : N - 1;
    } else {
        int s0 = 1;
        while (s0 * 2 < N) s0 *= 2;
        int pos = 0;
        for (int s = s0; s > 0; s >>= 1) {
            const int q = pos + s - 1;
            pos += (q < N && c[PAD ? cpad(q < N ? q : N - 1) : (q < N ? q : N - 1)] < r) ? s : 0;
        }
        return pos < N - 1 ? pos : N - 1;
    }
}

// ---- kernels both sweeps launch (csmc.hip: sequential; pit.hip: parallel in time) ------------------------------------------------------------
// the backward pass's uniforms, one per (chain, time step), drawn ONCE into an array (uniform c T + t of stream 4): inside the pass a single lane
// needed a single number per step, and the whole wave ran a Threefry block for it -- three quarters of the pass's vector instructions
template <typename R> __global__ void k_csmc_ubwd(long long n, uint32_t key0, uint32_t key1, R* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (2 * i >= n) return;
    R u0, u1;
    stream_uniform2<R>(key0, key1, STREAM_U_BWD, (unsigned long long)i, u0, u1);
    out[2 * i] = u0;
    if (2 * i + 1 < n) out[2 * i + 1] = u1;
}
// The forward pass's in-kernel draws (csmc.hip::k_csmc_fwd: one Threefry block serves two consecutive time steps of a particle), written out as the explicit
// arrays the same kernel reads in explicit-noise mode -- value for value what it would have drawn itself:
//   eps_prop[ch][t][n][k] = normal  2 (((ch T2 + (t >> 1)) N + n) D + k) + (t & 1) of stream 2,   u_res[ch][s][n] = uniform 2 ((ch T2 + (s >> 1)) N + n) + (s & 1) of stream 3
// grid (C T2, ceil(N D / 256)): blockIdx.x = ch T2 + h is the pair of time steps (2 h, 2 h + 1) of chain ch -- no 64-bit division per thread
template <typename R> __global__ void __launch_bounds__(256) k_csmc_pregen(int T, int N, int D, uint32_t key0, uint32_t key1, R* __restrict__ eps, R* __restrict__ ures) {
    const int T2 = (T + 1) >> 1, row = blockIdx.x, ch = row / T2, h = row - ch * T2;
    const int j = blockIdx.y * 256 + threadIdx.x, ND = N * D;
    if (j < ND) {
        R z0, z1;
        stream_normal2<R>(key0, key1, STREAM_EPS_PROP, (unsigned long long)row * ND + j, z0, z1);
        R* e = eps + ((long long)ch * T + 2 * h) * ND + j;
        e[0] = z0;
        if (2 * h + 1 < T) e[ND] = z1;
    }
    if (j < N) {
        R u0, u1;
        stream_uniform2<R>(key0, key1, STREAM_U_RES, (unsigned long long)row * N + j, u0, u1);
        R* u = ures + ((long long)ch * (T - 1) + 2 * h) * N + j;
        if (2 * h < T - 1) u[0] = u0;
        if (2 * h + 1 < T - 1) u[N] = u1;
    }
}
// ---- prologue: u = x + sqrt(delta_t/2) eps   (csmc/generic.py:67) ------------------------------------------------------
template <typename R> __global__ void k_csmc_aux(CsmcArgs a, int D) {
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long total = (long long)a.C * a.T * D;
    if (g >= total) return;
    const long long t = (g / D) % a.T;
    const R e = noise_normal<R>(a, a.eps_aux, STREAM_EPS_AUX, g);
    ((R*)a.u)[g] = fma_(((const R*)a.shd)[t], e, ((const R*)a.x)[g]);
}

// sum_k [log N(x_k; u_k, s) - log N(x_k; pm_k, s)] = sum_k ((x_k - pm_k)^2 - (x_k - u_k)^2) / (2 s^2)   (independent.py:184-189)
template <typename R, int D> __device__ __forceinline__ R grad_correction(const R* x, const R* u, const R* pm, R s) {
    R acc = 0;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        const R d1 = x[k] - u[k], d2 = x[k] - pm[k];
        acc = fma_(d2, d2, acc);
        acc = fma_(-d1, d1, acc);
    }
    return acc * ((R)0.5 / (s * s));
}

// the kernel argument of a user-model policy (fk_user.h::FkUserPolicy), also filled by the host (csmc.hip::run_csmc_program): the user potential's observations (T, p) and the two parameter vectors (device arrays of R, any may be null)
template <typename R> struct FkUser {
    const R* y;
    const R* theta_g;
    const R* theta_m;
    int p;
};

// ---- the model policy of the sweep bodies (compile time) ------------------------------------------------------------------------------------------
// The bodies below ask a policy object for the two model functions of a step:
//   pol.log_g(m, t, x, xprev, y, sz) log G_t(x_t) (xprev = x_{t-1}, nullptr at t = 0; y = the D reals of row t of CsmcArgs::y; sz = the D sizes of row t, plane 1
//                                    of y, filled by pol.size_row when P::size_row says that the policy may read them and nullptr otherwise)
//   pol.mean(m, tr, t, xprev, mu)    the mean of x_t | x_{t-1} = xprev under the transition tr (t = the index of x_t)
// and the gradient kernel (k_csmc_grad) for their derivatives:
//   pol.grad_log_g(m, t, x, xprev, y, gx, gxprev, sz)   gx = d log G_t / dx, gxprev = d log G_t / dxprev (nullptr at t = 0); both zero-filled by the caller
//   pol.mean_vjp(m, tr, t, xprev, v, out)           out = J^T v, J = d pol.mean(m, tr, t, xprev) / d xprev
//   P::grad_xprev                                   whether log G_t may depend on xprev (false: k_csmc_grad adds no d / dxprev term)
// FkBuiltin is the closed family of include/auxssm.h, dispatched on the integers of FkDev (the kernels of csmc.hip), FkBuiltin<R, D, V> the same with a coupled
// potential fixed at compile time (potential<R, D, V> above); fk_user.h's FkUserPolicy calls device functions of a user's source (fk_program.hip).  The backward
// pass evaluates the Gaussian transition density around pol.mean.
template <typename R, int D, PotV V = PotV::SEP> struct FkBuiltin {
    static constexpr bool grad_xprev = false;
    static constexpr bool size_row = pot_has_size(V);
    __device__ __forceinline__ void load_sizes(const FkDev<R>&, const R* y, long long T, long long t, R* sz) const {
#pragma unroll
        for (int k = 0; k < D; ++k) sz[k] = size_at<R>(y, T, t, D, k);
    }
    __device__ __forceinline__ R log_g(const FkDev<R>& m, int, const R* x, const R*, const R* y, const R* sz = nullptr) const { return potential<R, D, V>(m, x, y, sz); }
    __device__ __forceinline__ void mean(const FkDev<R>& m, const TransT<R>& tr, int, const R* xp, R* mu) const { trans_mean_t<R, D>(m, tr, xp, mu); }
    __device__ __forceinline__ void grad_log_g(const FkDev<R>& m, int, const R* x, const R*, const R* y, R* gx, R*, const R* sz = nullptr) const {
        potential_grad<R, D, V>(m, x, y, gx, sz);
    }
    __device__ __forceinline__ void mean_vjp(const FkDev<R>& m, const TransT<R>& tr, int, const R* xp, const R* v, R* out) const {
        trans_mean_vjp_t<R, D>(m, tr, xp, v, out);
    }
};
// the built-in family on per-chain transitions (ChainDyn above): the same two model functions, the transition record from row `chain` of the per-chain arrays
template <typename R, int D, PotV V = PotV::SEP> struct FkBuiltinChain : FkBuiltin<R, D, V> {};
template <typename R, int D, PotV V> struct ChainDyn<FkBuiltinChain<R, D, V>> { static constexpr bool value = true; };

// gradient at u of  log M0(u_0) + G0(u_0) + sum_t [log Mt(u_{t+1} | u_t) + Gt(u_{t+1}, u_t)]  (csmc/independent.py:121-134, jax.grad there), one thread per
// (chain, time step):  d_x log G_t(u_t, u_{t-1}) [+ d_xprev log G_{t+1}(u_{t+1}, u_t)] - Q^-1 (u_t - mean_t(u_{t-1})) + J_{t+1}(u_t)^T Q^-1 (u_{t+1} - mean_{t+1}(u_t))
// (t = 0: the prior term -P0^-1 (u_0 - m0); t = T - 1: no t + 1 terms).  The d_xprev term only exists for a policy whose potential may read xprev, and is
// added to the d_x term before anything else: a potential that leaves it at zero gives the built-in gradient bit for bit.
template <typename R, int D, typename P = FkBuiltin<R, D>, typename... PA> __global__ void k_csmc_grad(CsmcArgs a, FkDev<R> m, PA... pa) {
    const P pol{pa...};
    constexpr bool PC = ChainDyn<P>::value;  // per-chain transitions: this thread's chain is g / T (a.C counts all chains here: the gradient is not batched)
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (long long)a.C * a.T) return;
    const long long t = g % a.T;
    const R* u = (const R*)a.u + g * D;
    R ut[D], gr[D], r[D], w[D], mu[D];
#pragma unroll
    for (int k = 0; k < D; ++k) ut[k] = u[k];
    const R* yv = (const R*)a.y;
    // potential
    {
        R gp[D];
#pragma unroll
        for (int k = 0; k < D; ++k) gr[k] = gp[k] = (R)0;
        if constexpr (P::size_row) {
            R sz[D];
            pol.load_sizes(m, yv, a.T, t, sz);
            pol.grad_log_g(m, (int)t, ut, t > 0 ? u - D : nullptr, yv ? yv + t * D : nullptr, gr, t > 0 ? gp : nullptr, sz);
        } else {
            pol.grad_log_g(m, (int)t, ut, t > 0 ? u - D : nullptr, yv ? yv + t * D : nullptr, gr, t > 0 ? gp : nullptr);
        }
        if constexpr (P::grad_xprev) {
            if (t + 1 < a.T) {  // log G_{t+1}(u_{t+1}, u_t) as a function of u_t
                R gn[D], gq[D];
#pragma unroll
                for (int k = 0; k < D; ++k) gn[k] = gq[k] = (R)0;
                pol.grad_log_g(m, (int)t + 1, u + D, ut, yv ? yv + (t + 1) * D : nullptr, gn, gq);
#pragma unroll
                for (int k = 0; k < D; ++k) gr[k] = gr[k] + gq[k];
            }
        }
    }
    // density of u_t given the past
    if (t == 0) {
#pragma unroll
        for (int k = 0; k < D; ++k) r[k] = ut[k] - m.m0[k];
        cho_solve_fixed<R, D>(m.LP0, CS_MAXD, r, w);
    } else {
        const TransT<R> tr = PC ? trans_chain<R, D>(m, g / a.T) : trans_at<R, D>(m, t - 1);
        pol.mean(m, tr, (int)t, u - D, mu);
#pragma unroll
        for (int k = 0; k < D; ++k) r[k] = ut[k] - mu[k];
        cho_solve_fixed<R, D>(tr.LQ, tr.ld, r, w);
    }
#pragma unroll
    for (int k = 0; k < D; ++k) gr[k] = gr[k] - w[k];
    // density of u_{t+1} given u_t:  J(u_t)^T Q^-1 (u_{t+1} - mean(u_t))
    if (t + 1 < a.T) {
        const TransT<R> tr = PC ? trans_chain<R, D>(m, g / a.T) : trans_at<R, D>(m, t);
        pol.mean(m, tr, (int)t + 1, ut, mu);
#pragma unroll
        for (int k = 0; k < D; ++k) r[k] = u[D + k] - mu[k];
        cho_solve_fixed<R, D>(tr.LQ, tr.ld, r, w);
        pol.mean_vjp(m, tr, (int)t + 1, ut, w, mu);  // (mu: J^T w)
#pragma unroll
        for (int k = 0; k < D; ++k) gr[k] = gr[k] + mu[k];
    }
#pragma unroll
    for (int k = 0; k < D; ++k) ((R*)a.grad)[g * D + k] = gr[k];
}

// ---- forward pass (_csmc, csmc.py:69-107) -------------------------------------------------------------------------------
// NW = 8 / 16: exactly NW full waves (N = blockDim = 64 NW: the C4 / C3 shapes): no liveness / group-bound selects (block_expmax); NW = 0: any N
// SP = 1: the instantiation of config C3's shape -- auxiliary independent proposals, the stochastic-volatility potential, a time-invariant linear transition, draws
// generated in the kernel, no ancestor trace (backward sampling): the run-time switches on the model kind are folded at compile time (they are wave-uniform
// branches, two dozen per time step); same operations on the same operands, bit for bit (tests/test_gpu_csmc.py runs both instantiations on C3's model)
// SP = 2: the guided proposals (GuidedT above; time-invariant transitions, GRAD = the proposal mean reads the shifted u of CsmcArgs::grad): a compile-time variant, so
// that the instantiations of the other proposals hold none of its code; its weights have no reduction-free bound (CsmcArgs::gb is null: exact maxima)
// P: the model policy (above); PA: its kernel arguments (none for the built-in family, so the built-in kernels take exactly (CsmcArgs, FkDev) as before)
// ChainDyn<P>: per-chain transitions (FkBuiltinChain; csmc_chain.hip) -- TV = false, SP = 0 or 1: the chain's row is copied into scalar registers before the loop
// and every step reads that copy; the backward pass and k_csmc_grad (one thread per (chain, step): its row through pointers) follow the same switch
template <typename R, int D, bool TV, bool GRAD, int NW, int SP = 0, typename P = FkBuiltin<R, D>, typename... PA>
__global__ void __launch_bounds__(1024) k_csmc_fwd(CsmcArgs a, FkDev<R> m, PA... pa) {
    const P pol{pa...};
    if constexpr (SP == 1) {
        m.proposal = 1;
        m.potential = 2;
        m.transition = 0;
        a.As = nullptr;
        a.noise_mode = 1;
        a.pregen = 0;
    }
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int TB = blockDim.x, nw = TB >> 6, tid = threadIdx.x, N = a.N, T = a.T;
    // two images of (c, xprev), alternated by time-step parity: readers of step t never race writers of step t+1,
    // which removes the end-of-step barrier (4 barriers per step: max, sum, wave totals, publish)
    const int CP = cpad(TB);            // the cumsum image is padded against LDS bank conflicts of the search (cpad)
    R* cbuf = (R*)smem;                 // [2][CP]
    R* xbuf = cbuf + 2 * CP;            // [2][TB][D]
    R* red = xbuf + 2 * TB * D;         // [48]
    const int ch = a.c0 + blockIdx.x;
    constexpr bool PC = ChainDyn<P>::value;  // per-chain transitions: the chain's row, read once into scalar registers (TransC); untouched otherwise
    static_assert(!(PC && TV) && !(PC && SP == 2), "per-chain transitions are time-invariant and have no guided tables");
    TransC<R, D> trc;
    if constexpr (PC) trc.load(m, ch);
    const bool live = NW > 0 ? true : tid < N;
    if (tid < 16) red[32 + tid] = 0;  // totals of absent groups: +0 (totals_prefix reads all 16 slots; ordered by the first barrier below)
    const R* xstar = (const R*)a.x + (long long)ch * T * D;
    const R* uaux = (const R*)a.u + (long long)ch * T * D;
    const R* gaux = GRAD ? (const R*)a.grad + (long long)ch * T * D : uaux;
    const R* yv = (const R*)a.y;
    R* xs = (R*)a.xs + (long long)ch * T * N * D;
    R* lws = (R*)a.lws + (long long)ch * T * N;
    int32_t* As = a.As ? a.As + (long long)ch * (T - 1) * N : nullptr;
    const long long eps_base = (long long)ch * T * N * D;
    const long long ures_base = (long long)ch * (T - 1) * N;
    const R ninf = -INFINITY;

    // t = 0  (csmc.py:74-80)
    // In-kernel draws (THREEFRY): one Threefry block serves TWO consecutive time steps of a particle, so each step pays for
    // one block (normals on even t, uniforms on odd t) instead of two.  With T2 = ceil(T/2):
    //   eps_prop[ch][t][n][k] = normal  2 * (((ch T2 + (t >> 1)) N + n) D + k) + (t & 1)  of stream 2
    //   u_res[ch][s][n]       = uniform 2 * ((ch T2 + (s >> 1)) N + n) + (s & 1)          of stream 3
    // (flat auxssm_rng_* indices; csmc/_device.py::key_noise builds the equivalent explicit arrays).
    const bool gen = a.noise_mode != 0 && !a.pregen;
    const long long T2 = (T + 1) >> 1;
    R x[D], eps[D], eps_nx[D], ycur[D], pm[D], un_nx = 0;
    R szcur[P::size_row ? D : 1];  // the sizes of the step (the logistic potential); unused otherwise
    const R* szp = P::size_row ? szcur : nullptr;
    if constexpr (P::size_row) pol.load_sizes(m, yv, T, 0, szcur);
#pragma unroll
    for (int k = 0; k < D; ++k) {
        eps_nx[k] = 0;
        if (gen) {
            R z0, z1;
            stream_normal2<R>(a.key0, a.key1, STREAM_EPS_PROP, (unsigned long long)(((long long)ch * T2 * N + tid) * D + k), z0, z1);
            eps[k] = live ? z0 : (R)0;
            eps_nx[k] = live ? z1 : (R)0;
        } else {
            eps[k] = live ? ((const R*)a.eps_prop)[eps_base + (long long)tid * D + k] : (R)0;
        }
        ycur[k] = yv ? yv[k] : (R)0;
    }
    if constexpr (SP == 2) {  // guided: pred = m0, P = P0
        R ut[D];
#pragma unroll
        for (int k = 0; k < D; ++k) ut[k] = gaux[k];
        guided_propose<R, D>(guided_at<R>(a.gtab, D, 0), m.m0, ut, eps, pm, x);
    } else if (m.proposal == 0) {  // M0 = N(m0, P0)
#pragma unroll
        for (int k = 0; k < D; ++k) {
            R acc = m.m0[k];
#pragma unroll
            for (int j = 0; j <= k; ++j) acc = fma_(m.LP0[k * CS_MAXD + j], eps[j], acc);
            x[k] = acc;
        }
    } else {  // AuxiliaryM0: N(u_0 [+ delta_0/2 grad_0], delta_0/2 I)  (independent.py:143-158)
        const R s0 = ((const R*)a.shd)[0];
#pragma unroll
        for (int k = 0; k < D; ++k) {
            pm[k] = GRAD ? fma_(s0 * s0, gaux[k], uaux[k]) : uaux[k];
            x[k] = fma_(s0, eps[k], pm[k]);
        }
    }
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < D; ++k) x[k] = xstar[k];
    }
    R lw;
    {
        R g = pol.log_g(m, 0, x, nullptr, ycur, szp);
        if constexpr (SP == 2) {
            g = g + gauss_chol_logpdf<R, D>(x, m.m0, m.LP0, m.iLP0, m.c_init);
            g = guided_weight<R, D>(guided_at<R>(a.gtab, D, 0), g, x, uaux, pm);
        } else if (m.proposal == 1) {
            g = g + gauss_chol_logpdf<R, D>(x, m.m0, m.LP0, m.iLP0, m.c_init);  // AuxiliaryG0 (independent.py:163-169)
            if constexpr (GRAD) g = g + grad_correction<R, D>(x, uaux, pm, ((const R*)a.shd)[0]);  // GradientAuxiliaryG0 (:173-190)
        }
        lw = live ? g : ninf;
    }
    if (live) {
#pragma unroll
        for (int k = 0; k < D; ++k) xs[(long long)tid * D + k] = x[k];
        lws[tid] = lw;
    }
    R* fmax = a.fmax ? (R*)a.fmax + (long long)ch * T : nullptr;
    R mstep;
    R w = block_expmax<R, NW>(lw, red, tid, nw, &mstep);
    if (fmax && tid == 0) fmax[0] = mstep;
    const R* gbp = (const R*)a.gb;
    const bool bmode = gbp != nullptr && !(GRAD && m.gradient == 2);  // (the exact-gradient correction is unbounded in x)
    bool used_bound = false;

    for (int t = 1; t < T; ++t) {
        // issue this step's independent loads first
        R un = 0;
        const R gbt = bmode ? gbp[t] : (R)0;
#pragma unroll
        for (int k = 0; k < D; ++k) ycur[k] = yv ? yv[(long long)t * D + k] : (R)0;
        if constexpr (P::size_row) pol.load_sizes(m, yv, T, t, szcur);
        if (!gen) {
#pragma unroll
            for (int k = 0; k < D; ++k) eps[k] = live ? ((const R*)a.eps_prop)[eps_base + ((long long)t * N + tid) * D + k] : (R)0;
            if (live) un = ((const R*)a.u_res)[ures_base + (long long)(t - 1) * N + tid];
        } else if (t & 1) {  // normals cached by step t - 1; uniforms of steps t and t + 1
#pragma unroll
            for (int k = 0; k < D; ++k) eps[k] = eps_nx[k];
            stream_uniform2<R>(a.key0, a.key1, STREAM_U_RES, (unsigned long long)(((long long)ch * T2 + ((t - 1) >> 1)) * N + tid), un, un_nx);
        } else {  // uniform cached by step t - 1; normals of steps t and t + 1
            un = un_nx;
#pragma unroll
            for (int k = 0; k < D; ++k) {
                R z0, z1;
                stream_normal2<R>(a.key0, a.key1, STREAM_EPS_PROP, (unsigned long long)((((long long)ch * T2 + (t >> 1)) * N + tid) * D + k), z0, z1);
                eps[k] = live ? z0 : (R)0;
                eps_nx[k] = live ? z1 : (R)0;
            }
        }
        // conditional multinomial resampling (resamplings.py:14-37 -> jax.random.choice: cumsum, r = c[-1] (1-u), searchsorted)
        R* c = cbuf + (t & 1) * CP;
        R* xprev = xbuf + (t & 1) * TB * D;
#pragma unroll
        for (int k = 0; k < D; ++k) xprev[tid * D + k] = x[k];
        R tot;
        block_cumsum_dpp<R, NW, true>(w, c, red, tid, nw, tot);  // trailing barrier also publishes xprev; tot = c[N - 1]
        if (used_bound && !(tot > (R)0)) {  // every weight of step t - 1 underflowed under its bound: the exact maximum after all (uniform)
            __syncthreads();                // (every lane is past its reads of the step's images before they are rewritten)
            w = block_expmax<R, NW>(lw, red, tid, nw, &mstep);
            if (fmax && tid == 0) fmax[t - 1] = mstep;
            block_cumsum_dpp<R, NW, true>(w, c, red, tid, nw, tot);
        }
        int idx = 0;
        if (live && tid > 0) idx = search2<R, NW, true>(c, N, tot * ((R)1 - un));
        R xp[D];
#pragma unroll
        for (int k = 0; k < D; ++k) xp[k] = xprev[idx * D + k];
        // propagate (csmc.py:91-92); the transition t - 1 -> t (time-varying: row t - 1 of the device arrays)
        const TransT<R> tr = PC ? trc.trans() : trans_at_c<R, D, TV>(m, t - 1);
        if constexpr (SP == 2) {  // guided: pred = the parent's transition mean, P = Q
            R mu[D], ut[D];
            pol.mean(m, tr, t, xp, mu);
#pragma unroll
            for (int k = 0; k < D; ++k) ut[k] = gaux[(long long)t * D + k];
            guided_propose<R, D>(guided_at<R>(a.gtab, D, t), mu, ut, eps, pm, x);
        } else if (m.proposal == 0) {
            R mu[D];
            pol.mean(m, tr, t, xp, mu);
#pragma unroll
            for (int k = 0; k < D; ++k) {
                R acc = mu[k];
#pragma unroll
                for (int j = 0; j <= k; ++j) acc = fma_(tr.LQ[k * tr.ld + j], eps[j], acc);
                x[k] = acc;
            }
        } else {  // AuxiliaryMtDynamics: N(u_t [+ delta_t/2 grad_t], delta_t/2 I), independent of the parent (independent.py:192-198)
            const R st = ((const R*)a.shd)[t];
#pragma unroll
            for (int k = 0; k < D; ++k) {
                pm[k] = GRAD ? fma_(st * st, gaux[(long long)t * D + k], uaux[(long long)t * D + k]) : uaux[(long long)t * D + k];
                x[k] = fma_(st, eps[k], pm[k]);
            }
        }
        if (tid == 0) {
#pragma unroll
            for (int k = 0; k < D; ++k) x[k] = xstar[(long long)t * D + k];
        }
        // weights (csmc.py:95-96)
        R g = pol.log_g(m, t, x, xp, ycur, szp);
        if constexpr (SP == 2) {
            R mu[D];
            pol.mean(m, tr, t, xp, mu);
            g = g + gauss_chol_logpdf<R, D>(x, mu, tr.LQ, tr.iL, tr.c_trans, tr.ld);
            g = guided_weight<R, D>(guided_at<R>(a.gtab, D, t), g, x, uaux + (long long)t * D, pm);
        } else if (m.proposal == 1) {  // AuxiliaryGt = Mt.logpdf + Gt (independent.py:238-248)
            R mu[D];
            pol.mean(m, tr, t, xp, mu);
            g = gauss_chol_logpdf<R, D>(x, mu, tr.LQ, tr.iL, tr.c_trans, tr.ld) + g;
            // GradientAuxiliaryGt (:252-268): in the reference the correction is summed over all particles, i.e. a constant of the
            // step (AUXSSM_GRAD_REFERENCE: nothing to add); AUXSSM_GRAD_EXACT applies it per particle
            if constexpr (GRAD) {
                if (m.gradient == 2) g = g + grad_correction<R, D>(x, uaux + (long long)t * D, pm, ((const R*)a.shd)[t]);
            }
        }
        lw = live ? g : ninf;
        if (live) {
            const long long o = (long long)t * N + tid;
#pragma unroll
            for (int k = 0; k < D; ++k) xs[o * D + k] = x[k];
            lws[o] = lw;
            if (As) As[(long long)(t - 1) * N + tid] = idx;
        }
        // the shift of this step's weights (sweep contract): a reduction-free bound where there is one, else the block maximum
        R Mb = gbt + (m.proposal == 1 ? tr.c_trans : (R)0);
        used_bound = bmode && t < T - 1 && (Mb - Mb == 0);
        if (used_bound) {
            w = det_exp(lw - Mb);
            mstep = Mb;
        } else {
            w = block_expmax<R, NW>(lw, red, tid, nw, &mstep);
        }
        if (fmax && tid == 0) fmax[t] = mstep;
    }
    if (live) ((R*)a.wT)[(long long)ch * N + tid] = w;
}

// ---- backward passes (csmc.py:110-149) ------------------------------------------------------------------------------------
// One draw per step: B = #{j : c_j < r} by ballot + per-wave counts (no serial search), the candidate particles of the step are
// published to LDS before the first barrier so that x_t^B is an LDS read, and the next step's rows (xs, log_ws) and uniform are
// fetched one step ahead: no global-memory latency on the dependent chain.  4 barriers per step (max, wave totals, publish, counts).
template <typename R, int D, bool TV, int NW, typename P = FkBuiltin<R, D>, typename... PA>
__global__ void __launch_bounds__(1024) k_csmc_bwd(CsmcArgs a, FkDev<R> m, PA... pa) {
    const P pol{pa...};
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int TB = blockDim.x, nw = TB >> 6, tid = threadIdx.x, N = a.N, T = a.T;
    R* c = (R*)smem;                 // [2][TB] the step's cumulative weights (generic) / local scan values (full workgroups), by step parity
    R* red = c + 2 * TB;             // [48] + [16]: a second set of wave totals (slots [48, 64)) for the odd steps of the one-barrier loop
    R* xpub = red + 64;              // [2][TB][D] candidate particles of the step, by step parity
    R* ubuf = xpub + 2 * TB * D;     // [2] the step's uniform, by step parity
    const int ch = a.c0 + blockIdx.x;
    constexpr bool PC = ChainDyn<P>::value;  // per-chain transitions, as in the forward pass
    static_assert(!(PC && TV), "per-chain transitions are time-invariant");
    TransC<R, D> trc;
    if constexpr (PC) trc.load(m, ch);
    const bool live = NW > 0 ? true : tid < N;
    if (tid < 16) red[32 + tid] = 0, red[48 + tid] = 0;  // totals of absent groups: +0 (totals_prefix)
    const R* xs = (const R*)a.xs + (long long)ch * T * N * D;
    const R* lws = (const R*)a.lws + (long long)ch * T * N;
    const int32_t* As = a.As ? a.As + (long long)ch * (T - 1) * N : nullptr;
    R* xout = (R*)a.x + (long long)ch * T * D;
    int32_t* anc = a.anc + (long long)ch * T;
    const long long ub_base = (long long)ch * T;
    const R ninf = -INFINITY;

    // B_T ~ choice(w_T)   (csmc.py:111 / :131); w_T are the forward pass's unnormalised weights
    R w = live ? ((const R*)a.wT)[(long long)ch * N + tid] : (R)0;
    if (tid == 0) ubuf[1] = ((const R*)a.u_bwd)[ub_base + (T - 1)];
    {
        R xi[D];
#pragma unroll
        for (int k = 0; k < D; ++k) xi[k] = live ? xs[((long long)(T - 1) * N + tid) * D + k] : (R)0;
#pragma unroll
        for (int k = 0; k < D; ++k) xpub[(TB + tid) * D + k] = xi[k];
    }
    R tot;
    int B;
    {   // (sweep contract: the two-level single draw; the generic cumsum image c[] holds base + local, so the local values are recovered per group)
        const int lane = tid & 63, wv = tid >> 6;
        const R v = wave_scan_dpp(w);
        c[TB + tid] = v;
        if (lane == 63) red[32 + wv] = v;
        __syncthreads();
        R pre, Pv;
        totals_prefix<R>(red, lane, wv, nw - 1, pre, tot, &Pv);
        B = draw_two_level<R>(c + TB, Pv, lane, nw, N, tot * ((R)1 - ubuf[1]));
    }
    R xn[D];
#pragma unroll
    for (int k = 0; k < D; ++k) xn[k] = xpub[(TB + B) * D + k];
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < D; ++k) xout[(long long)(T - 1) * D + k] = xn[k];
        anc[T - 1] = B;
    }
    if (!a.backward) {
        // ancestor tracing: B_{t-1} = A_t[B_t]  (csmc.py:114-121); a dependent pointer chase, one lane
        if (tid == 0) {
            for (int t = T - 1; t >= 1; --t) {
                B = As[(long long)(t - 1) * N + B];
#pragma unroll
                for (int k = 0; k < D; ++k) xout[(long long)(t - 1) * D + k] = xs[((long long)(t - 1) * N + B) * D + k];
                anc[t - 1] = B;
            }
        }
        return;
    }
    // backward sampling (Whiteley), csmc.py:134-146
    __syncthreads();  // the parity-1 slots of the first draw are free again
    R xi_nx[D], lw_nx = ninf, un_nx = 0, fm_nx = 0;
    const R* fmax = (const R*)a.fmax + (long long)ch * T;
    if (T >= 2) {
#pragma unroll
        for (int k = 0; k < D; ++k) xi_nx[k] = live ? xs[((long long)(T - 2) * N + tid) * D + k] : (R)0;
        lw_nx = live ? lws[(long long)(T - 2) * N + tid] : ninf;
        fm_nx = fmax[T - 2];
        if (tid == 0) un_nx = ((const R*)a.u_bwd)[ub_base + (T - 2)];
    }
    for (int t = T - 2; t >= 0; --t) {
        const int par = t & 1;
        R xi[D];
#pragma unroll
        for (int k = 0; k < D; ++k) xi[k] = xi_nx[k];
        const R lwi = lw_nx, un_t = un_nx, fm_t = fm_nx;
        if (t > 0) {  // the rows of step t - 1: independent of this step's draw
#pragma unroll
            for (int k = 0; k < D; ++k) xi_nx[k] = live ? xs[((long long)(t - 1) * N + tid) * D + k] : (R)0;
            lw_nx = live ? lws[(long long)(t - 1) * N + tid] : ninf;
            fm_nx = fmax[t - 1];
            if (tid == 0) un_nx = ((const R*)a.u_bwd)[ub_base + (t - 1)];
        }
        R lw = ninf;
        const TransT<R> tr = PC ? trc.trans() : trans_at_c<R, D, TV>(m, t);  // Pt.logpdf(x_{t+1}, xs_t, params_t) (csmc.py:136)
        if (live) {
            R mu[D];
            pol.mean(m, tr, t + 1, xi, mu);
            lw = gauss_chol_logpdf<R, D>(xn, mu, tr.LQ, tr.iL, tr.c_trans, tr.ld) + lwi;
        }
#pragma unroll
        for (int k = 0; k < D; ++k) xpub[(par * TB + tid) * D + k] = xi[k];
        if (tid == 0) ubuf[par] = un_t;
        // weights shifted by a bound of their maximum that needs no reduction (sweep contract): the forward pass's block maximum of
        // log_ws[t] plus the transition's log-normaliser; the exact maximum only if everything underflowed
        R Mb = fm_t + tr.c_trans;
        if (!(Mb - Mb == 0)) Mb = 0;
        w = det_exp(lw - Mb);
        {   // ONE barrier per step: local scan values and wave totals of this parity are published together with xpub / ubuf; every wave then finds the
            // group and counts inside it on its own (draw_two_level)
            const int lane = tid & 63, wv = tid >> 6;
            R* vloc = c + par * TB;
            R* tl = red + 32 + par * 16;
            R v = wave_scan_dpp(w);
            vloc[tid] = v;
            if (lane == 63) tl[wv] = v;
            __syncthreads();
            R pre, Pv;
            totals_prefix<R>(tl - 32, lane, wv, nw - 1, pre, tot, &Pv);
            if (!(tot > (R)0)) {  // (uniform) every weight underflowed under its bound: the exact maximum after all
                __syncthreads();  // (every wave has read this parity's totals before they are rewritten)
                w = block_expmax<R, NW>(lw, red, tid, nw);
                v = wave_scan_dpp(w);
                vloc[tid] = v;
                if (lane == 63) tl[wv] = v;
                __syncthreads();
                totals_prefix<R>(tl - 32, lane, wv, nw - 1, pre, tot, &Pv);
            }
            B = draw_two_level<R>(vloc, Pv, lane, nw, N, tot * ((R)1 - ubuf[par]));
        }
#pragma unroll
        for (int k = 0; k < D; ++k) xn[k] = xpub[(par * TB + B) * D + k];
        if (tid == 0) {
#pragma unroll
            for (int k = 0; k < D; ++k) xout[(long long)t * D + k] = xn[k];
            anc[t] = B;
        }
    }
}

}  // namespace ax
