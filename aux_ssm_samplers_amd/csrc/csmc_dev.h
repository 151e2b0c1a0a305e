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
