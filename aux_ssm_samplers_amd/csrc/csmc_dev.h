// csmc_dev.h -- what the conditional-SMC units share (csmc.hip: the sequential sweep; pit.hip: the parallel-in-time sweep): the
// device-side Feynman-Kac model, its densities in fixed operation order, and the workgroup reductions whose orders the C oracle
// (oracle/csmc_ref.c) restates.  Units including this are compiled with -ffp-contract=off.
#pragma once
#include <cstring>
#include "ctx.h"
#include "csmc_sweep.h"

namespace ax {

// additive constants of time-varying transition densities: ct[t] = -sum_k log LQ_t[k][k] - D/2 log 2 pi
template <typename R, int D> __global__ void k_csmc_ctrans(int n, const R* __restrict__ LQt, R* __restrict__ ct, R* __restrict__ idt) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    R c = 0;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        const R l = LQt[((long long)t * D + k) * D + k];
        c -= det_log(l);
        idt[(long long)t * D + k] = (R)1 / l;  // reciprocal diagonal (sweep contract v3)
    }
    ct[t] = c - (R)D * (R)0.91893853320467274178;
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
// gradient at u of  log M0(u_0) + G0(u_0) + sum_t [log Mt(u_{t+1} | u_t) + Gt(u_{t+1})]  (csmc/independent.py:121-134, jax.grad there),
// closed form for the model family: one thread per (chain, time step)
template <typename R, int D> __global__ void k_csmc_grad(CsmcArgs a, FkDev<R> m) {
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (long long)a.C * a.T) return;
    const long long t = g % a.T;
    const R* u = (const R*)a.u + g * D;
    R ut[D], gr[D], r[D], w[D], mu[D];
#pragma unroll
    for (int k = 0; k < D; ++k) ut[k] = u[k];
    const R* yv = (const R*)a.y;
    // potential
#pragma unroll
    for (int k = 0; k < D; ++k) {
        const R y = yv ? yv[t * D + k] : (R)0;
        R v = 0;
        if (m.potential == 1 || (m.potential == 3 && y - y == 0)) v = ((y - ut[k]) * m.inv_sig_y) * m.inv_sig_y;
        else if (m.potential == 2) {
            const R e = det_exp(-ut[k]);
            v = (R)0.5 * fma_(y * y, e, (R)-1);
            v = (v == v) ? v : (R)0;
        }
        gr[k] = v;
    }
    // density of u_t given the past
    if (t == 0) {
#pragma unroll
        for (int k = 0; k < D; ++k) r[k] = ut[k] - m.m0[k];
        cho_solve_fixed<R, D>(m.LP0, CS_MAXD, r, w);
    } else {
        const TransT<R> tr = trans_at<R, D>(m, t - 1);
        trans_mean_t<R, D>(m, tr, u - D, mu);
#pragma unroll
        for (int k = 0; k < D; ++k) r[k] = ut[k] - mu[k];
        cho_solve_fixed<R, D>(tr.LQ, tr.ld, r, w);
    }
#pragma unroll
    for (int k = 0; k < D; ++k) gr[k] = gr[k] - w[k];
    // density of u_{t+1} given u_t:  J(u_t)^T Q^-1 (u_{t+1} - mean(u_t))
    if (t + 1 < a.T) {
        const TransT<R> tr = trans_at<R, D>(m, t);
        trans_mean_t<R, D>(m, tr, ut, mu);
#pragma unroll
        for (int k = 0; k < D; ++k) r[k] = u[D + k] - mu[k];
        cho_solve_fixed<R, D>(tr.LQ, tr.ld, r, w);
        if constexpr (D == 3) {
            if (m.transition == 1) {  // Lorenz-63: J = I + dt dphi/dx (examples/lorenz/model.py:10-25)
                const R th1 = m.F[0], th2 = m.F[1], th3 = m.F[2], dt = m.b[0];
                const R J[9] = {-th1, th1, (R)0, th2 - ut[2], (R)-1, -ut[0], ut[1], ut[0], -th3};
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    R acc = 0;
#pragma unroll
                    for (int j = 0; j < 3; ++j) acc = fma_(J[j * 3 + k], w[j], acc);
                    gr[k] = gr[k] + fma_(dt, acc, w[k]);
                }
                goto done;
            }
        }
#pragma unroll
        for (int k = 0; k < D; ++k) {
            R acc = 0;
#pragma unroll
            for (int j = 0; j < D; ++j) acc = fma_(tr.F[j * tr.ld + k], w[j], acc);
            gr[k] = gr[k] + acc;
        }
    }
done:
#pragma unroll
    for (int k = 0; k < D; ++k) ((R*)a.grad)[g * D + k] = gr[k];
}

template <typename R> static void fill_model(FkDev<R>& m, const auxssm_fk_model* fk, const double* host) {
    // host = [m0 (D) | chol_P0 (D*D) | F (D*D) | b (D) | chol_Q (D*D)] as doubles
    const int D = fk->dx;
    memset(&m, 0, sizeof(m));  // (also: no time-varying arrays, no gradient; the sweep entry point sets them)
    m.proposal = fk->proposal;
    m.potential = fk->potential;
    m.D = D;
    m.transition = fk->transition;
    const double* p = host;
    for (int k = 0; k < D; ++k) m.m0[k] = (R)p[k];
    p += D;
    for (int i = 0; i < D; ++i)
        for (int j = 0; j < D; ++j) m.LP0[i * CS_MAXD + j] = (R)p[i * D + j];
    p += D * D;
    for (int i = 0; i < D; ++i)
        for (int j = 0; j < D; ++j) m.F[i * CS_MAXD + j] = (R)p[i * D + j];
    p += D * D;
    for (int k = 0; k < D; ++k) m.b[k] = (R)p[k];
    p += D;
    for (int i = 0; i < D; ++i)
        for (int j = 0; j < D; ++j) m.LQ[i * CS_MAXD + j] = (R)p[i * D + j];
    // additive constants, computed once on the host in precision R (they enter both the GPU and the oracle as data)
    R ci = 0, ct = 0;
    for (int k = 0; k < D; ++k) {
        ci -= det_log(m.LP0[k * CS_MAXD + k]);
        ct -= det_log(m.LQ[k * CS_MAXD + k]);
    }
    for (int k = 0; k < D; ++k) {
        m.iLP0[k] = (R)1 / m.LP0[k * CS_MAXD + k];
        m.iLQ[k] = (R)1 / m.LQ[k * CS_MAXD + k];
    }
    const R half_log_2pi = (R)0.91893853320467274178;
    m.c_init = ci - (R)D * half_log_2pi;
    m.c_trans = ct - (R)D * half_log_2pi;
    if (fk->potential == 1) {
        m.inv_sig_y = (R)1 / (R)fk->sig_y;
        m.c_obs = -(R)D * det_log((R)fk->sig_y) - (R)D * half_log_2pi;
    } else if (fk->potential == 3) {  // per observed component
        m.inv_sig_y = (R)1 / (R)fk->sig_y;
        m.c_obs = -det_log((R)fk->sig_y) - half_log_2pi;
    } else {
        m.inv_sig_y = 0;
        m.c_obs = -half_log_2pi;
    }
}

}  // namespace ax
