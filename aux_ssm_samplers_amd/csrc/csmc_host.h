// csmc_host.h -- the host side the conditional-SMC drivers share (csmc.hip: the sequential sweep, built-in and user-defined models; csmc_wide.hip: the
// wide-state sweep; pit.hip: the parallel-in-time sweep): the model checks of both entry points, the model in precision R, the one kernel launch helper
// (launch), the per-sweep prologue (csmc_prologue: transition constants, potential bound, auxiliary variables, gradient or guided tables), chain batching and
// the dtype x dx dispatch.  (The workspace plan the drivers fill, WsPlan, is ctx.h's.)  hipcc only (the device side, csmc_sweep.h, also compiles under
// hipRTC).  Units including this are compiled with -ffp-contract=off.
#pragma once
#include <cstring>
#include <type_traits>
#include <utility>

#include "ctx.h"
#include "csmc_sweep.h"
#include "csmc_guided.h"

namespace ax {

// What a built-in potential kind needs, in ONE place, indexed by AUXSSM_POT_* (its compile-time variant: csmc_sweep.h::pot_variant, shared with the device code).
// A new kind adds its row here.
struct PotKind {
    bool needs_y;                               // reads the observations y
    const double* auxssm_fk_model::*matrix;     // the ABI field of the dx x dx matrix a coupled potential carries (FkDev / FkW::pot_mat), or null
    const char* matrix_missing;                 // check_fk_model's message when that field is NULL
    bool wide_no_bound;                         // the wide-state sweep drops the bound array and shifts every step by its exact maximum (csmc.hip::csmc_sweep_impl)
    bool unassigned = false;                    // a number no kind has: check_fk_model refuses it as it refuses one beyond the table
};
static const PotKind POT_KINDS[] = {
    /* AUXSSM_POT_FLAT */ {false, nullptr, nullptr, false},
    /* AUXSSM_POT_GAUSS_OBS */ {true, nullptr, nullptr, false},
    /* AUXSSM_POT_SV */ {true, nullptr, nullptr, false},
    /* AUXSSM_POT_GAUSS_OBS_MASKED */ {true, nullptr, nullptr, false},
    /* AUXSSM_POT_MVT */ {true, &auxssm_fk_model::prec, "the multivariate-t potential needs its precision matrix prec (host, dx x dx)", true},
    /* AUXSSM_POT_LIN_GAUSS */
    {true, &auxssm_fk_model::obs_H, "the linear-Gaussian observation potential needs its whitened observation matrix obs_H (host, dx x dx)", true},
    /* AUXSSM_POT_POISSON */ {true, nullptr, nullptr, true},
    /* 7: unassigned */ {false, nullptr, nullptr, false, true},
    /* AUXSSM_POT_LOGISTIC: y is (2, T, dx), the sizes in plane 1 */ {true, nullptr, nullptr, true},
};
constexpr int POT_NKINDS = sizeof(POT_KINDS) / sizeof(POT_KINDS[0]);
static_assert(POT_FLAT == AUXSSM_POT_FLAT && POT_GAUSS_OBS == AUXSSM_POT_GAUSS_OBS && POT_SV == AUXSSM_POT_SV && POT_GAUSS_OBS_MASKED == AUXSSM_POT_GAUSS_OBS_MASKED &&
                  POT_MVT == AUXSSM_POT_MVT && POT_LIN_GAUSS == AUXSSM_POT_LIN_GAUSS && POT_POISSON == AUXSSM_POT_POISSON && POT_LOGISTIC == AUXSSM_POT_LOGISTIC &&
                  POT_NKINDS == 9 && POT_NKINDS == AUXSSM_POT_LOGISTIC + 1,
              "csmc_sweep.h restates the potential kinds of include/auxssm.h");
static const PotKind& pot_kind(int kind) { return POT_KINDS[kind]; }  // (kind checked by check_fk_model)
// the matrix of fk's potential (host, dx x dx), or null for a potential without one
static const double* pot_matrix(const auxssm_fk_model* fk) { return pot_kind(fk->potential).matrix ? fk->*pot_kind(fk->potential).matrix : nullptr; }

// The one kernel launch of the cSMC drivers: kern<<<grid, block, lds, h->stream>>>(args...), the kernel's dynamic LDS limit raised first when the launch asks
// for more than the 48 KB every kernel is granted.  (Functions of a hipRTC module have no such attribute: csmc.hip::fk_launch.)
template <typename... P, typename... A> static int launch(auxssm_ctx* h, void (*kern)(P...), dim3 grid, dim3 block, size_t lds, A&&... args) {
    if (lds > 48 * 1024) AX_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, grid, block, lds, h->stream, std::forward<A>(args)...);
    return AUXSSM_OK;
}

// the model checks auxssm_csmc_sweep(_program) and auxssm_csmc_pit_sweep share; each entry point adds its own (proposals, dimensions, the explicit noise
// arrays it reads).  user_potential: the potential is a program's, which brings its own observations
static int check_fk_model(const auxssm_fk_model* fk, const auxssm_csmc_noise* noise, bool user_potential) {
    if (fk->potential < 0 || fk->potential >= POT_NKINDS || POT_KINDS[fk->potential].unassigned) {
        set_error("unknown potential kind %d", fk->potential);
        return AUXSSM_ERR_ARG;
    }
    if (!fk->m0 || !fk->chol_P0 || !fk->F || !fk->b || !fk->chol_Q) {
        set_error("model has a NULL m0/chol_P0/F/b/chol_Q host pointer");
        return AUXSSM_ERR_ARG;
    }
    const PotKind& pk = pot_kind(fk->potential);
    if (!user_potential && pk.needs_y && !fk->y) {
        set_error("potential needs observations y");
        return AUXSSM_ERR_ARG;
    }
    if (fk->potential == AUXSSM_POT_GAUSS_OBS && !(fk->sig_y > 0)) {
        set_error("sig_y must be > 0");
        return AUXSSM_ERR_ARG;
    }
    if (!user_potential && pk.matrix && !pot_matrix(fk)) {
        set_error("%s", pk.matrix_missing);
        return AUXSSM_ERR_ARG;
    }
    if (fk->potential == AUXSSM_POT_MVT && !user_potential && !(fk->nu > 0)) {
        set_error("the multivariate-t potential needs nu > 0");
        return AUXSSM_ERR_ARG;
    }
    const int ntv = (fk->F_t != nullptr) + (fk->b_t != nullptr) + (fk->chol_Q_t != nullptr);
    if (ntv != 0 && ntv != 3) {
        set_error("time-varying transitions need F_t, b_t and chol_Q_t together (device arrays with T - 1 rows)");
        return AUXSSM_ERR_ARG;
    }
    if (ntv && fk->transition != AUXSSM_TRANS_LINEAR) {
        set_error("time-varying parameters are for the linear transition only");
        return AUXSSM_ERR_ARG;
    }
    if (fk->gradient != AUXSSM_GRAD_NONE && fk->gradient != AUXSSM_GRAD_REFERENCE && fk->gradient != AUXSSM_GRAD_EXACT) {
        set_error("unknown gradient mode %d", fk->gradient);
        return AUXSSM_ERR_ARG;
    }
    if (noise->mode != AUXSSM_NOISE_EXPLICIT && noise->mode != AUXSSM_NOISE_THREEFRY) {
        set_error("unknown noise mode %d", noise->mode);
        return AUXSSM_ERR_ARG;
    }
    return AUXSSM_OK;
}

// The model of fk in precision R, as both kernel families read it: the parameters into m0 | LP0 | F | b | LQ (matrices row-major, leading dimension ld), the
// reciprocal Cholesky diagonals into iLP0 / iLQ, the kinds, the gradient mode and the additive constants into m (FkDev<R>, or csmc_wide.hip's FkW<R>).  The
// constants are computed once, here, in precision R: they enter both the GPU and the oracle as data.  pot_mat: where the matrix of a coupled potential goes
// (pot_matrix: the precision matrix of AUXSSM_POT_MVT, the whitened observation matrix of AUXSSM_POT_LIN_GAUSS, whose c_lin goes into c_obs).
template <typename R, typename M>
static void fk_model(const auxssm_fk_model* fk, M& m, int ld, R* m0, R* LP0, R* iLP0, R* F, R* b, R* LQ, R* iLQ, R* pot_mat) {
    const int D = fk->dx;
    m.proposal = fk->proposal;
    m.potential = fk->potential;
    m.D = D;
    m.gradient = fk->gradient;
    for (int k = 0; k < D; ++k) m0[k] = (R)fk->m0[k], b[k] = (R)fk->b[k];
    for (int i = 0; i < D; ++i)
        for (int j = 0; j < D; ++j) {
            LP0[i * ld + j] = (R)fk->chol_P0[i * D + j];
            F[i * ld + j] = (R)fk->F[i * D + j];
            LQ[i * ld + j] = (R)fk->chol_Q[i * D + j];
        }
    R ci = 0, ct = 0;
    for (int k = 0; k < D; ++k) {
        ci -= det_log(LP0[k * ld + k]);
        ct -= det_log(LQ[k * ld + k]);
        iLP0[k] = (R)1 / LP0[k * ld + k];
        iLQ[k] = (R)1 / LQ[k * ld + k];
    }
    const R half_log_2pi = (R)0.91893853320467274178;
    m.c_init = ci - (R)D * half_log_2pi;
    m.c_trans = ct - (R)D * half_log_2pi;
    if (fk->potential == AUXSSM_POT_GAUSS_OBS) {
        m.inv_sig_y = (R)1 / (R)fk->sig_y;
        m.c_obs = -(R)D * det_log((R)fk->sig_y) - (R)D * half_log_2pi;
    } else if (fk->potential == AUXSSM_POT_GAUSS_OBS_MASKED) {  // per observed component
        m.inv_sig_y = (R)1 / (R)fk->sig_y;
        m.c_obs = -det_log((R)fk->sig_y) - half_log_2pi;
    } else if (fk->potential == AUXSSM_POT_LIN_GAUSS) {  // c_lin, formed on the host in double with the whitening
        m.inv_sig_y = 0;
        m.c_obs = (R)fk->obs_const;
    } else {
        m.inv_sig_y = 0;
        m.c_obs = -half_log_2pi;
    }
    m.mvt_hc = 0, m.mvt_inv_nu = 0;
    if (fk->potential == AUXSSM_POT_MVT) {  // (nu + D) / 2 and 1 / nu, formed here once in precision R
        m.mvt_hc = ((R)fk->nu + (R)D) / (R)2;
        m.mvt_inv_nu = (R)1 / (R)fk->nu;
    }
    if (const double* A = pot_matrix(fk))
        for (int i = 0; i < D; ++i)
            for (int j = 0; j < D; ++j) pot_mat[i * ld + j] = (R)A[i * D + j];
}
// the register kernels' model (the time-varying arrays null: fk_time_varying sets them)
template <typename R> static FkDev<R> fk_dev(const auxssm_fk_model* fk) {
    FkDev<R> m;
    memset(&m, 0, sizeof(m));
    m.transition = fk->transition;
    fk_model<R>(fk, m, CS_MAXD, m.m0, m.LP0, m.iLP0, m.F, m.b, m.LQ, m.iLQ, m.pot_mat);
    return m;
}

// additive constants ct[t] = -sum_k log LQ_t[k][k] - D/2 log 2 pi and reciprocal diagonals of the time-varying transition densities, one thread per transition
template <typename R> __global__ void k_csmc_ctrans(int n, int D, const R* __restrict__ LQt, R* __restrict__ ct, R* __restrict__ idt) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    R c = 0;
    for (int k = 0; k < D; ++k) {
        const R l = LQt[((long long)t * D + k) * D + k];
        c -= det_log(l);
        idt[(long long)t * D + k] = (R)1 / l;  // reciprocal diagonal (sweep contract v3)
    }
    ct[t] = c - (R)D * (R)0.91893853320467274178;
}
// time-varying transitions (fk's device rows F_t, b_t, chol_Q_t of the T - 1 transitions): m reads them, and ctt -- (T - 1) (1 + D) reals of workspace --
// receives their constants and reciprocal diagonals.  Nothing to do for a time-invariant model.
template <typename R, typename M> static void fk_time_varying(auxssm_ctx* h, const auxssm_fk_model* fk, int T, void* ctt, M& m) {
    if (!fk->F_t || T < 2) return;
    m.Ft = (const R*)fk->F_t;
    m.bt = (const R*)fk->b_t;
    m.LQt = (const R*)fk->chol_Q_t;
    m.ctt = (const R*)ctt;
    m.idt = (const R*)ctt + (T - 1);
    hipLaunchKernelGGL((k_csmc_ctrans<R>), dim3((T - 1 + 255) / 256), dim3(256), 0, h->stream, T - 1, fk->dx, m.LQt, (R*)ctt, (R*)ctt + (T - 1));
}

// gb[t] = sup_x G_t(x): the reduction-free part of the forward weights' shift (sweep contract, csmc_sweep.h); +inf where the potential is unbounded
template <typename R> __global__ void k_csmc_potbound(int T, int D, int potential, R c_obs, const R* __restrict__ y, R* __restrict__ gb) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    R b = 0;  // (FLAT, and the multivariate-t potential: sup_x log g = 0 for a positive definite precision)
    if (potential == AUXSSM_POT_GAUSS_OBS) b = c_obs;
    else if (potential == AUXSSM_POT_GAUSS_OBS_MASKED) {
        int nobs = 0;
        for (int k = 0; k < D; ++k) nobs += (y[(long long)t * D + k] - y[(long long)t * D + k] == 0) ? 1 : 0;
        b = (R)nobs * c_obs;
    } else if (potential == AUXSSM_POT_LIN_GAUSS) {  // c_lin - |yw - Hw x|^2 / 2 <= c_lin; a missing row (all NaN) makes the step flat
        bool obs = true;
        for (int k = 0; k < D; ++k) obs = obs && (y[(long long)t * D + k] - y[(long long)t * D + k] == 0);
        b = obs ? c_obs : (R)0;
    } else if (potential == AUXSSM_POT_SV) {  // sum_k [c_obs - (x + y^2 e^-x) / 2] <= sum_k max(0, c_obs - (1 + log y^2) / 2)  (a NaN term counts 0)
        for (int k = 0; k < D; ++k) {
            const R yk = y[(long long)t * D + k], y2 = yk * yk;
            R v = (R)0;
            if (y2 - y2 == 0) v = y2 > (R)0 ? fma_((R)-0.5, (R)1 + det_log(y2), c_obs) : (R)INFINITY;
            b += v > (R)0 ? v : (R)0;
        }
    } else if (potential == AUXSSM_POT_POISSON) {  // sum_k [y x - e^x] <= sum_k y (log y - 1), attained at x_k = log y_k; y_k = 0 and a missing y_k add 0: always finite
        for (int k = 0; k < D; ++k) {
            const R yk = y[(long long)t * D + k];
            b += yk > (R)0 ? yk * (det_log(yk) - (R)1) : (R)0;
        }
    } else if (potential == AUXSSM_POT_LOGISTIC) {
        // sum_k [y x - m softplus(x)] <= the binomial log-likelihood at p = y / m, y log(y / m) + (m - y) log((m - y) / m), without cancellation; <= 0, always
        // finite; 0 at y = 0 and y = m (approached, not attained) and for a missing y_k
        for (int k = 0; k < D; ++k) {
            const R yk = y[(long long)t * D + k], mk = y[((long long)T + t) * D + k], nk = mk - yk;
            const R v = (yk > (R)0 ? yk * det_log(yk / mk) : (R)0) + (nk > (R)0 ? nk * det_log(nk / mk) : (R)0);
            b += (yk - yk == 0) ? v : (R)0;
        }
    }
    gb[t] = b;
}
template <typename R, typename M> static void fk_potbound(auxssm_ctx* h, const CsmcArgs& a, const M& m) {
    hipLaunchKernelGGL((k_csmc_potbound<R>), dim3((a.T + 255) / 256), dim3(256), 0, h->stream, a.T, m.D, m.potential, m.c_obs, (const R*)a.y, (R*)a.gb);
}

// guided proposals (AUXSSM_PROP_AUX_GUIDED), after k_csmc_aux has formed u: the shifted auxiliary variables of the gradient variant into a.grad and the tables
// of the T steps into a.gtab ((2 D D + D + 4) reals per step: guided_tab_reals).  Rebuilt at every sweep: delta may change between sweeps.
static size_t guided_tab_reals(int T, int D) { return (size_t)T * ((size_t)2 * D * D + D + 4); }
template <typename R, typename M> static void fk_guided(auxssm_ctx* h, const CsmcArgs& a, const M& m) {
    if (m.gradient)
        with_pot(m.potential, [&](auto pv) {
            constexpr PotV V = decltype(pv)::value;
            const long long total = (long long)a.C * a.T;
            if constexpr (pot_has_matrix(V)) hipLaunchKernelGGL((k_csmc_gshift_coupled<R, M, V>), dim3((unsigned)((total + 63) / 64)), dim3(64), 0, h->stream, a, m);
            else if constexpr (V == PotV::POIS) hipLaunchKernelGGL((k_csmc_gshift_pois<R>), dim3((unsigned)((total * m.D + 255) / 256)), dim3(256), 0, h->stream, a, m.D);
            else if constexpr (V == PotV::LOGI) hipLaunchKernelGGL((k_csmc_gshift_logi<R>), dim3((unsigned)((total * m.D + 255) / 256)), dim3(256), 0, h->stream, a, m.D);
            else hipLaunchKernelGGL((k_csmc_gshift<R>), dim3((unsigned)((total * m.D + 255) / 256)), dim3(256), 0, h->stream, a, m.D, m.potential, m.inv_sig_y);
        });
    hipLaunchKernelGGL((k_csmc_gtab<R, M>), dim3(a.T), dim3(64), 0, h->stream, a.T, m, (const R*)a.shd, (R*)a.gtab);
}

// the gradient launch of the built-in family on the register kernels (csmc.hip::run_csmc, pit.hip::run_pit)
template <typename R, int D> static int builtin_grad(auxssm_ctx* h, const CsmcArgs& a, const FkDev<R>& m) {
    const dim3 grid((unsigned)(((long long)a.C * a.T + 255) / 256));
    with_pot(m.potential, [&](auto pv) { hipLaunchKernelGGL((k_csmc_grad<R, D, FkBuiltin<R, D, decltype(pv)::value>>), grid, dim3(256), 0, h->stream, a, m); });
    return AUXSSM_OK;
}

// What a sweep enqueues before its passes, in this order: the constants of time-varying transitions (m then reads them), the built-in potential's bound into
// a.gb (user_bound: the program has launched its own), the auxiliary variables u = x + sqrt(delta / 2) eps of the auxiliary proposals (a.u null: the caller's
// kernels form them themselves -- pit.hip without gradients), then the gradient at u for gradient-informed independent proposals -- grad(), the one launch the
// drivers differ in: it returns an AUXSSM_* code -- or the guided proposals' shift and tables.  SEQ = false: the parallel-in-time sweep, which has neither a
// bound array nor guided proposals (its unit then holds none of their kernels).
template <typename R, bool SEQ = true, typename M, typename G>
static int csmc_prologue(auxssm_ctx* h, const auxssm_fk_model* fk, const CsmcArgs& a, void* ctt, M& m, bool user_bound, G&& grad) {
    fk_time_varying<R>(h, fk, a.T, ctt, m);
    if constexpr (SEQ) {
        if (a.gb && !user_bound) fk_potbound<R>(h, a, m);
    }
    if (m.proposal == AUXSSM_PROP_BOOTSTRAP_LG || !a.u) return AUXSSM_OK;
    const long long total = (long long)a.C * a.T * m.D;
    hipLaunchKernelGGL((k_csmc_aux<R>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, a, m.D);
    if constexpr (SEQ) {
        if (m.proposal == AUXSSM_PROP_AUX_GUIDED) {
            fk_guided<R>(h, a, m);
            return AUXSSM_OK;
        }
    }
    return m.gradient ? grad() : AUXSSM_OK;
}

// ---- what the launchers of the sequential passes share (csmc.hip::run_csmc / run_csmc_program, csmc_chain.hip::run_csmc_chain) ----
// dynamic LDS of the forward / backward pass (csmc_sweep.h: k_csmc_fwd, k_csmc_bwd) for TB lanes
static size_t fwd_lds(int TB, int D, size_t sR) { return (size_t)2 * (cpad(TB) + TB * D) * sR + 48 * sR + 64; }
static size_t bwd_lds(int TB, int D, size_t sR) { return (size_t)2 * TB * sR + 64 * sR + (size_t)2 * TB * D * sR + 2 * sR + 64; }

// the workgroup shapes with instantiations of their own (NW of k_csmc_fwd / k_csmc_bwd): sixteen full waves, eight full waves, 0 = any N
static int nw_class(int N) { return N == 1024 ? 16 : (N == 512 ? 8 : 0); }
// f(std::true_type / std::false_type) for b; f(std::integral_constant<int, nw>) for an nw_class
template <typename F> static auto with_bool(bool b, F&& f) { return b ? f(std::true_type{}) : f(std::false_type{}); }
template <typename F> static auto with_nw(int nw, F&& f) {
    return nw == 16 ? f(std::integral_constant<int, 16>{}) : (nw == 8 ? f(std::integral_constant<int, 8>{}) : f(std::integral_constant<int, 0>{}));
}

// a pass of the built-in family, as run_csmc launches it
template <typename R> using SweepKernel = void (*)(CsmcArgs, FkDev<R>);

// the arguments of the batch [c0, c0 + cb) of chains (CsmcArgs::c0)
static CsmcArgs csmc_batch(const CsmcArgs& a, int c0, int cb) {
    CsmcArgs ab = a;
    ab.c0 = c0;
    ab.C = a.C - c0 < cb ? a.C - c0 : cb;
    ab.xs = (char*)a.xs - (size_t)c0 * a.xs_rec;
    ab.lws = (char*)a.lws - (size_t)c0 * a.lws_rec;
    if (a.As) ab.As = (int32_t*)((char*)a.As - (size_t)c0 * a.As_rec);
    return ab;
}

// f(R(), std::integral_constant<int, D>()) for the sweep's dtype and dx: the register kernels' instantiations, 1 <= dx <= CS_MAXD
template <typename F> static int csmc_dispatch(int dtype, int D, F&& f) {
    auto dx = [&](auto r) {
        switch (D) {
            case 1: return f(r, std::integral_constant<int, 1>{});
            case 2: return f(r, std::integral_constant<int, 2>{});
            case 3: return f(r, std::integral_constant<int, 3>{});
            default: return f(r, std::integral_constant<int, 4>{});
        }
    };
    return dtype == AUXSSM_F32 ? dx(0.0f) : dx(0.0);
}

}  // namespace ax
