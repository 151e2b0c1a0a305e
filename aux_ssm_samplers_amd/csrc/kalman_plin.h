// kalman_plin.h -- Poisson counts through a loading matrix under the auxiliary Kalman sampler (AUXSSM_KMODEL_POISSON_LIN_FIRST / _SECOND):
//
//     y_{t,j} ~ Poisson(exp(h_j' x_t + c_j)),  j = 1..dy,      log g_t = sum_j y_j eta_j - e_j,  grad_t = H' (y - e),  Lam_t = H' diag(e) H = -hess
//
// with eta = H x + c, e = exp(eta), every term of a missing (NaN) count dropped -- and its twin under the logit link (AUXSSM_KMODEL_LOGISTIC_LIN_FIRST / _SECOND:
// binomial and negative-binomial channels, plin_accum_logistic below), which shares everything but the channel body.  The first half of this header is the per-step arithmetic as AX_HD functions:
// the kernels of kalman_plin.hip and the CPU harness of tests/hostsim_plin compile the same text.  The second half (HIP builds only) is what api.hip hands to
// kalman_plin.hip.
#pragma once
#include "smallmat.h"

namespace ax {

constexpr int PLIN_JB = 64;        // channels per column block: the y tile of a block is staged through LDS, and a step's potential value is summed per block
constexpr int PLIN_MAX_DY = 1024;  // (include/auxssm.h; a limit of the interface: the column-block loop itself takes any dy)

// what one (chain, step) accumulates over the channels: 1 + D + D (D + 1) / 2 numbers (15 at D = 4)
template <typename R, int D> struct PlinAcc {
    Acc val;               // log g_t: each column block's part summed in R, the blocks in Acc
    R g[D];                // H' (y - e)
    R lam[symsize(D)];     // upper triangle of H' diag(e) H
};
template <typename R, int D> AX_HD void plin_zero(PlinAcc<R, D>& a) {
    a.val = 0;
#pragma unroll
    for (int k = 0; k < D; ++k) a.g[k] = 0;
#pragma unroll
    for (int k = 0; k < symsize(D); ++k) a.lam[k] = 0;
}
// n <= PLIN_JB channels of one column block, ascending: y (n, element stride 1) the step's counts, Hb (n, D) row-major and cb (n) the block's rows of H and c.
// One exponential per channel.  A count that is not finite is missing: it takes part in nothing.
template <typename R, int D> AX_HD void plin_accum(PlinAcc<R, D>& a, const R* x, const R* y, const R* Hb, const R* cb, int n) {
    R v = 0;
    for (int j = 0; j < n; ++j) {
        R h[D];
        R eta = cb[j];
#pragma unroll
        for (int k = 0; k < D; ++k) {
            h[k] = Hb[j * D + k];
            eta += h[k] * x[k];
        }
        const R yj = y[j];
        const bool on = finite_(yj);
        const R e = on ? exp_(eta) : (R)0;
        const R yy = on ? yj : (R)0;
        v += yy * eta - e;
        const R r = yy - e;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            a.g[k] += h[k] * r;
            const R eh = e * h[k];
#pragma unroll
            for (int l = k; l < D; ++l) a.lam[sidx_u(D, k, l)] += eh * h[l];
        }
    }
    a.val += (Acc)v;
}
// The same block under the logit link (AUXSSM_KMODEL_LOGISTIC_LIN_*): channel j has the size m = sb[j] + wb[j] yy (binomial: sb = trials, wb = 0; negative
// binomial: sb = r, wb = 1 -- no branch), and with e = exp(-|eta|) <= 1, r = 1 / (1 + e):  sigma = eta >= 0 ? r : e r,  sigma (1 - sigma) = (e r) r on either
// side (never a subtraction),  softplus = max(eta, 0) + log1p(e):
//     log g += yy eta - m softplus,      g += h (yy - m sigma),      lam += (m sigma (1 - sigma)) h h'
// One exponential, one reciprocal and one logarithm per channel; nothing overflows at any eta.  A missing channel has yy = m = 0 by selection: its size (which may
// be anything, NaN included) is never part of a sum.
template <typename R, int D> AX_HD void plin_accum_logistic(PlinAcc<R, D>& a, const R* x, const R* y, const R* Hb, const R* cb, const R* sb, const R* wb, int n) {
    R v = 0;
    for (int j = 0; j < n; ++j) {
        R h[D];
        R eta = cb[j];
#pragma unroll
        for (int k = 0; k < D; ++k) {
            h[k] = Hb[j * D + k];
            eta += h[k] * x[k];
        }
        const R yj = y[j];
        const bool on = finite_(yj);
        const R yy = on ? yj : (R)0;
        const R m = on ? sb[j] + wb[j] * yy : (R)0;
        const R e = exp_(-abs_(eta));
        const R u = (R)1 + e, r = (R)1 / u, er = e * r;
        // log1p(e) = log(u) + log(1 + (e - (u - 1)) / u): u - 1 is exact (u in (1, 2]), so e - (u - 1) is what rounding u lost, and its first-order term restores
        // it -- accurate to an ulp however small e is, on the reciprocal the body has anyway (the library's log1pf alone is about 100 instructions)
        const R l1p = log_(u) + (e - (u - (R)1)) * r;
        v += yy * eta - m * (max_(eta, (R)0) + l1p);
        const R res = yy - m * (eta >= (R)0 ? r : er);
        const R w = m * (er * r);
#pragma unroll
        for (int k = 0; k < D; ++k) {
            a.g[k] += h[k] * res;
            const R wh = w * h[k];
#pragma unroll
            for (int l = k; l < D; ++l) a.lam[sidx_u(D, k, l)] += wh * h[l];
        }
    }
    a.val += (Acc)v;
}
// the auxiliary observation of the step from its sums: order 1  ys = u + delta/2 grad;  order 2  Om = sym((Lam + 2/delta I)^-1) by Cholesky (Lam is PSD: the
// matrix is positive definite), ys = Om (2u/delta + grad + Lam x); Om: upper triangle, packed (written for order 2 only)
template <typename R, int D> AX_HD void plin_finish(const PlinAcc<R, D>& a, const R* x, const R* u, R delta, int order, R* ys, R* Om) {
    if (order == 1) {
#pragma unroll
        for (int k = 0; k < D; ++k) ys[k] = u[k] + (R)0.5 * delta * a.g[k];
        return;
    }
    const R td = (R)2 / delta;
    R A[symsize(D)], L[symsize(D)], invd[D], X[D * D], rhs[D];
#pragma unroll
    for (int k = 0; k < D; ++k)
#pragma unroll
        for (int l = k; l < D; ++l) A[sidx_u(D, k, l)] = a.lam[sidx_u(D, k, l)] + (k == l ? td : (R)0);
    chol_packed<R, D>(A, L, invd, nullptr);
#pragma unroll
    for (int col = 0; col < D; ++col) {  // column col of the inverse
        R b[D];
#pragma unroll
        for (int k = 0; k < D; ++k) b[k] = k == col ? (R)1 : (R)0;
        cho_solve<R, D>(L, invd, b);
#pragma unroll
        for (int k = 0; k < D; ++k) X[k * D + col] = b[k];
    }
#pragma unroll
    for (int k = 0; k < D; ++k)
#pragma unroll
        for (int l = k; l < D; ++l) Om[sidx_u(D, k, l)] = (R)0.5 * (X[k * D + l] + X[l * D + k]);  // symmetrised where it is formed
#pragma unroll
    for (int k = 0; k < D; ++k) {
        R s = td * u[k] + a.g[k];
#pragma unroll
        for (int l = 0; l < D; ++l) s += a.lam[sidx(D, k, l)] * x[l];
        rhs[k] = s;
    }
#pragma unroll
    for (int k = 0; k < D; ++k) {
        R s = 0;
#pragma unroll
        for (int l = 0; l < D; ++l) s += Om[sidx(D, k, l)] * rhs[l];
        ys[k] = s;
    }
}
// One step from x_t, u_t, y_t (dy), H (dy, D) row-major, c (dy): value = log g_t(x_t), ys (D) and -- order 2 -- Om (upper triangle, packed).  The channels go
// through in column blocks of PLIN_JB, as the kernel takes them.
template <typename R, int D> AX_HD void plin_step(const R* x, const R* u, const R* y, const R* H, const R* c, int dy, R delta, int order, Acc& value, R* ys, R* Om) {
    PlinAcc<R, D> a;
    plin_zero(a);
    for (int j0 = 0; j0 < dy; j0 += PLIN_JB) plin_accum<R, D>(a, x, y + j0, H + (long long)j0 * D, c + j0, dy - j0 < PLIN_JB ? dy - j0 : PLIN_JB);
    value = a.val;
    plin_finish<R, D>(a, x, u, delta, order, ys, Om);
}
// The same step under the logit link: csw (3, dy) = [c; s; w], the array the model's cs slot carries (include/auxssm.h, LOGISTIC_LIN_*)
template <typename R, int D>
AX_HD void plin_step_logistic(const R* x, const R* u, const R* y, const R* H, const R* csw, int dy, R delta, int order, Acc& value, R* ys, R* Om) {
    PlinAcc<R, D> a;
    plin_zero(a);
    for (int j0 = 0; j0 < dy; j0 += PLIN_JB)
        plin_accum_logistic<R, D>(a, x, y + j0, H + (long long)j0 * D, csw + j0, csw + dy + j0, csw + 2 * (long long)dy + j0, dy - j0 < PLIN_JB ? dy - j0 : PLIN_JB);
    value = a.val;
    plin_finish<R, D>(a, x, u, delta, order, ys, Om);
}
// log N(y; x, Om) with Om dense symmetric (upper triangle, packed), by Cholesky in registers; NaN when the factorisation fails
template <typename R, int D> AX_HD R plin_norm_logpdf(const R* y, const R* x, const R* Om) {
    R L[symsize(D)], invd[D], z[D];
    const bool ok = chol_packed<R, D>(Om, L, invd, nullptr);
    R ld = 0, q = 0;
#pragma unroll
    for (int k = 0; k < D; ++k) z[k] = y[k] - x[k];
    lsolve<R, D>(L, invd, z);
#pragma unroll
    for (int k = 0; k < D; ++k) {
        q += z[k] * z[k];
        ld += log_(L[lidx(k, k)]);
    }
    return ok ? (R)-0.5 * q - ld - (R)(0.5 * LOG_2PI) * (R)D : r_nan<R>();
}

}  // namespace ax

#if defined(__HIPCC__) && !defined(__HIPCC_RTC__)
#include "ctx.h"

namespace ax {

// The factory launch at one linearisation point, everything per-chain dense (C, T, D).  eps != null (pass 1): u = xlin + sqrt(delta/2) eps is formed and
// written; eps == null (pass 2): u is read.  Writes ys (C, T, D), for order 2 the full dense Rs (C, T, D, D), and pot (C, T): log g_t(xlin_t) in Acc.
enum PlinLink : int { PLIN_POISSON = 0, PLIN_LOGISTIC = 1 };  // the channel body: plin_accum | plin_accum_logistic (then c is [c; s; w] (3, dy))
struct PlinObsArgs {
    int link;
    int C, T, D, dy, order;
    double delta;        // host step size (a placeholder when dptr is set)
    const double* dptr;  // device-resident {delta, sqrt(delta / 2)}, or null
    const void *H, *c;   // (dy, D) row-major, (dy) -- PLIN_LOGISTIC: (3, dy)
    const void* yobs;    // (T, dy), time stride y_st elements
    long long y_st;
    const void *xlin, *eps;
    void *u, *ys, *Rs;
    Acc* pot;
};
int run_plin_obs(auxssm_ctx* h, int dtype, const PlinObsArgs& a);
// The five totals k_sv_accept takes, [5][C] in the sweep's dtype: pot(x'), pot(x) (the sums of pot2 / pot1 as the two factory launches left them: no
// exponential here), la1 = sum_t log N(ys1_t; x'_t, R1_t), la2 = sum_t log N(ys2_t; x_t, R2_t) (R1 / R2 null: delta/2 I), corr.
struct PlinTermsArgs {
    int C, T, D;
    double delta;
    const double* dptr;
    const void *x, *xp, *u, *ys1, *ys2, *R1, *R2;
    const Acc *pot1, *pot2;
    Acc* part;  // scratch of plin_terms_part_bytes(C, T): the per-segment sums
    void* out;
};
size_t plin_terms_part_bytes(int C, int T);
int run_plin_terms(auxssm_ctx* h, int dtype, const PlinTermsArgs& a);

}  // namespace ax
#endif
