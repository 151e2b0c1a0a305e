// csmc_guided.h -- the per-sweep prologue of the guided proposals (AUXSSM_PROP_AUX_GUIDED; csmc_sweep.h::GuidedT holds the layout the sweep kernels read):
// the tables K_t, chol Lambda_t of every time step, built on the device from the model's Cholesky factors and the sqrt(delta_t / 2) array, and the shifted
// auxiliary variables of the gradient variant.  hipcc only (included by csmc_host.h).  Units including this are compiled with -ffp-contract=off.
#pragma once
#include "csmc_sweep.h"

namespace ax {

// element (i, j) of chol P0 (init) or chol Q of a model; csmc_wide.hip adds the overload of its FkW
template <typename R> __device__ __forceinline__ R gt_chol(const FkDev<R>& m, bool init, int i, int j) { return (init ? m.LP0 : m.LQ)[i * CS_MAXD + j]; }
constexpr int GT_MAXD = CS_MAXD_RT;  // the widest state of either kernel family

constexpr int GT_S = 33;  // row stride of the 32 x 32 work matrices in LDS (odd: a column walk touches every bank)

// in-place lower Cholesky factor of the symmetric A (D x D in LDS, row stride GT_S; the lower triangle is read), one lane per row, column by column: lane i >= j
// forms A_ij - sum_{k < j} L_ik L_jk in k order and the pivot L_jj the same way (every lane its own copy: no broadcast).  A failed pivot leaves NaNs behind.
template <typename R> __device__ __forceinline__ void gt_cholesky(R* A, int D, int i) {
    for (int j = 0; j < D; ++j) {
        R val = 0;
        const bool mine = i >= j && i < D;
        if (mine) {
            R acc = A[i * GT_S + j], dj = A[j * GT_S + j];
            for (int k = 0; k < j; ++k) {
                acc = fma_(-A[i * GT_S + k], A[j * GT_S + k], acc);
                dj = fma_(-A[j * GT_S + k], A[j * GT_S + k], dj);
            }
            dj = sqrt(dj);
            val = i == j ? dj : acc / dj;
        }
        __syncthreads();  // (column j and the pivot have been read by every lane before they are overwritten)
        if (mine) A[i * GT_S + j] = val;
        __syncthreads();
    }
}

// The tables of step t = blockIdx.x (one wave per step, lane i = row i; D <= 32), with P = P0 at t = 0, Q after, s = sqrt(delta_t / 2):
//   K = solve(P + s^2 I, P)^T by the Cholesky factor of P + s^2 I (lane c solves column c, which is row c of K);  Lambda = P - K P;
//   L = cholesky((Lambda + Lambda^T) / 2); a factorisation that fails (a non-finite entry) is replaced by s I, as the reference's where(isfinite) does with
//   the all-NaN factor its cholesky returns on failure.
// Row t of tab (GuidedT): K (D x D) | L (D x D, zeros above the diagonal) | 1 / L_kk (D) | c_lam | c_u | 1 / s | 0.
template <typename R, typename M> __global__ void __launch_bounds__(64) k_csmc_gtab(int T, M m, const R* __restrict__ shd, R* __restrict__ tab) {
    __shared__ R Pm[32 * GT_S], A[32 * GT_S], X[32 * GT_S];
    const int t = blockIdx.x, i = threadIdx.x, D = m.D;
    const bool row = i < D, init = t == 0;
    const R s = shd[t], s2 = s * s;
    R* out = tab + (long long)t * (2 * D * D + D + 4);
    if (row) {
        for (int j = 0; j < D; ++j) {
            R acc = 0;
            const int n = i < j ? i : j;
            for (int k = 0; k <= n; ++k) acc = fma_(gt_chol(m, init, i, k), gt_chol(m, init, j, k), acc);
            Pm[i * GT_S + j] = acc;
            A[i * GT_S + j] = i == j ? acc + s2 : acc;
        }
    }
    __syncthreads();
    gt_cholesky<R>(A, D, i);
    if (row) {  // column i of (P + s^2 I)^-1 P: forward, then backward substitution, in place in column i of X
        for (int k = 0; k < D; ++k) {
            R acc = Pm[k * GT_S + i];
            for (int j = 0; j < k; ++j) acc = fma_(-A[k * GT_S + j], X[j * GT_S + i], acc);
            X[k * GT_S + i] = acc / A[k * GT_S + k];
        }
        for (int k = D - 1; k >= 0; --k) {
            R acc = X[k * GT_S + i];
            for (int j = k + 1; j < D; ++j) acc = fma_(-A[j * GT_S + k], X[j * GT_S + i], acc);
            X[k * GT_S + i] = acc / A[k * GT_S + k];
        }
    }
    __syncthreads();
    if (row) {  // K_ik = X_ki;  Lambda_ij = P_ij - sum_k K_ik P_kj  (into A: its factor is no longer needed)
        for (int j = 0; j < D; ++j) {
            R acc = Pm[i * GT_S + j];
            for (int k = 0; k < D; ++k) acc = fma_(-X[k * GT_S + i], Pm[k * GT_S + j], acc);
            A[i * GT_S + j] = acc;
            out[i * D + j] = X[j * GT_S + i];
        }
    }
    __syncthreads();
    if (row)
        for (int j = 0; j <= i; ++j) X[i * GT_S + j] = (R)0.5 * (A[i * GT_S + j] + A[j * GT_S + i]);
    __syncthreads();
    gt_cholesky<R>(X, D, i);
    bool ok = true;
    if (row)
        for (int j = 0; j <= i; ++j) ok = ok && (X[i * GT_S + j] - X[i * GT_S + j] == 0);
    const bool failed = __ballot(!ok) != 0ull;
    R* Lo = out + D * D;
    if (row) {
        for (int j = 0; j < D; ++j) {
            const R v = failed ? (i == j ? s : (R)0) : (j <= i ? X[i * GT_S + j] : (R)0);
            Lo[i * D + j] = v;
            if (i == j) X[i * GT_S + i] = v, out[2 * D * D + i] = (R)1 / v;
        }
    }
    __syncthreads();
    if (i == 0) {
        const R half_log_2pi = (R)0.91893853320467274178;
        R c = 0;
        for (int k = 0; k < D; ++k) c -= det_log(X[k * GT_S + k]);
        R* cs = out + 2 * D * D + D;
        cs[0] = c - (R)D * half_log_2pi;                  // log N(.; ., Lambda_t) = c_lam - |L^-1 (x - mu)|^2 / 2
        cs[1] = -(R)D * det_log(s) - (R)D * half_log_2pi;  // sum_k log N(x_k; u_k, s^2) = c_u - sum_k ((x_k - u_k) / s)^2 / 2
        cs[2] = (R)1 / s;
        cs[3] = 0;
    }
}

// gradient variant: u~ = u + s_t^2 grad_x log g_t(u_t) into a.grad, once per (chain, t, component) -- the separable potentials are sums over components, so
// the gradient is component by component (csmc_sweep.h::sep_grad_term)
template <typename R> __global__ void k_csmc_gshift(CsmcArgs a, int D, int potential, R inv_sig_y) {
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (long long)a.C * a.T * D) return;
    const long long t = (g / D) % a.T;
    const int k = (int)(g % D);
    const R u = ((const R*)a.u)[g], s = ((const R*)a.shd)[t];
    const R yk = a.y ? ((const R*)a.y)[t * D + k] : (R)0;
    ((R*)a.grad)[g] = fma_(s * s, sep_grad_term<R>(potential, inv_sig_y, u, yk), u);
}

// the same for the Poisson count potential (csmc_sweep.h::pois_grad_term), a kernel of its own: k_csmc_gshift stays as it was
template <typename R> __global__ void k_csmc_gshift_pois(CsmcArgs a, int D) {
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (long long)a.C * a.T * D) return;
    const long long t = (g / D) % a.T;
    const int k = (int)(g % D);
    const R u = ((const R*)a.u)[g], s = ((const R*)a.shd)[t];
    ((R*)a.grad)[g] = fma_(s * s, pois_grad_term<R>(u, ((const R*)a.y)[t * D + k]), u);
}

// the same for the logistic potential (csmc_sweep.h::logi_grad_term; the size of (t, k) is plane 1 of y), again a kernel of its own
template <typename R> __global__ void k_csmc_gshift_logi(CsmcArgs a, int D) {
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (long long)a.C * a.T * D) return;
    const long long t = (g / D) % a.T;
    const int k = (int)(g % D);
    const R u = ((const R*)a.u)[g], s = ((const R*)a.shd)[t];
    ((R*)a.grad)[g] = fma_(s * s, logi_grad_term<R>(u, ((const R*)a.y)[t * D + k], size_at<R>((const R*)a.y, a.T, t, D, k)), u);
}

// the same for a coupled potential (variant V: csmc_sweep.h::coupled_grad with the run-time dimension m.D), whose gradient is not component by component: one
// thread per (chain, t).  M: FkDev or csmc_wide.hip's FkW
template <typename R, typename M, PotV V> __global__ void k_csmc_gshift_coupled(CsmcArgs a, M m) {
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (long long)a.C * a.T) return;
    const int D = m.D;
    const long long t = g % a.T;
    const R* u = (const R*)a.u + g * D;
    const R s = ((const R*)a.shd)[t];
    coupled_grad<R, V, 0>(m, m.pot_mat, m.mat_ld(), u, (const R*)a.y + t * D, [&](int k, R v) { ((R*)a.grad)[g * D + k] = fma_(s * s, v, u[k]); });
}

}  // namespace ax
