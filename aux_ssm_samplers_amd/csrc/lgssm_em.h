// lgssm_em.h -- the arithmetic of EM for a time-invariant linear-Gaussian state-space model (csrc/lgssm_em.hip): the lag-one smoothing covariance of one step,
// the expected sufficient statistics of one step, and the closed-form M-steps of the three parameter blocks.  AX_HD functions only: the kernels compile this text
// for gfx950 and tests/hostsim_lgssm_em compiles it with g++ (tests/lgssm_em_np.py is its literal NumPy restatement).  Everything here is in double, whatever the
// moments' type; units that include it are built with -ffp-contract=off.
//
// Model: x_0 ~ N(m0, P0), x_{t+1} = F x_t + b + N(0, Q), y_t = H x_t + c + N(0, R).  With the filtered moments (m_t, P_t), the smoothed moments (sm_t, sP_t),
// z_t = [x_t; 1] (n = D + 1) and E[.] = E[. | y_{0:T-1}]:
//   lag one      S_t = sym(F P_t F^T + Q),  G_t = P_t F^T S_t^-1 (Cholesky + two triangular solves),  X_t = Cov[x_{t+1}, x_t | y] = sP_{t+1} G_t^T      t = 0 .. T - 2
//   dynamics     S_zz = sum_{t < T-1} E[z_t z_t^T],  S_xz = sum E[x_{t+1} z_t^T],  S_xx = sum E[x_{t+1} x_{t+1}^T]      -- dynamics_theta.h's sums in expectation:
//                E[x_t x_t^T] = sP_t + sm_t sm_t^T,  E[x_{t+1} x_t^T] = X_t + sm_{t+1} sm_t^T;  the corner S_zz[D, D] = number of transitions, exactly
//   observations over the steps whose row of y is entirely finite:  So_zz = sum E[z_t z_t^T] (n x n),  S_yz = sum y_t E[z_t]^T (DY x n)
//   M-steps      [F b] = S_xz S_zz^-1,  Q = sym(S_xx - [F b] S_xz^T) / N_tr        (or the mode of dt_posterior's matrix-normal inverse-Wishart: M_n, Psi_n / (nu_n + D + n + 1))
//                [H c] = S_yz So_zz^-1,  R = sym(S_yy - [H c] S_yz^T) / n_obs
//                m0 = mean_s sm_0,  P0 = mean_s [sP_0 + (sm_0 - m0)(sm_0 - m0)^T]
//                With U = chol(S_zz) and Y = S_xz U^-T the product [F b] S_xz^T is Y Y^T, formed on the lower triangle and mirrored: Q, R, P0 symmetric bit for bit.
// PACKED statistics of a segment: [dynamics: DtDims<D>::PACKED sums, dynamics_theta.h's layout | lower triangle of So_zz | S_yz row-major].
// FULL statistics of a sequence (auxssm_kalman_smooth_stats): [S_zz (n, n) | S_xz (D, n) | S_xx (D, D) | So_zz (n, n) | S_yz (dy, n) | sm_0 (D) | sP_0 (D, D)].
#pragma once
#include "dynamics_theta.h"

namespace ax {

constexpr int EM_MAX_DY = 8;
constexpr int EM_THREADS = 256;  // lanes of one statistics workgroup

enum EmFlag {
    EM_OK = 0,
    EM_FAIL_GRAM = 1,      // chol(S_zz), chol(K_n) or chol(So_zz) failed, or the block has no step to sum
    EM_FAIL_RESIDUAL = 2,  // Q, R or P0 is not positive definite (or its diagonal is rounding noise of the terms it is the difference of)
    EM_FAIL_FINITE = 3     // a result is not finite in the model's dtype
};
enum EmBlock { EM_DYNAMICS = 1, EM_OBSERVATIONS = 2, EM_INITIAL = 4 };

AX_HD int em_dyn_full(int dx) { return (dx + 1) * (dx + 1) + dx * (dx + 1) + dx * dx; }
AX_HD int em_dyn_packed(int dx) { return (dx + 1) * (dx + 2) / 2 + dx * (dx + 1) + dx * (dx + 1) / 2; }  // DtDims<dx>::PACKED
AX_HD int em_obs_full(int dx, int dy) { return (dx + 1) * (dx + 1) + dy * (dx + 1); }
AX_HD int em_obs_packed(int dx, int dy) { return (dx + 1) * (dx + 2) / 2 + dy * (dx + 1); }
AX_HD int em_ns(int dx, int dy) { return em_dyn_full(dx) + em_obs_full(dx, dy) + dx + dx * dx; }  // doubles per sequence of stats_out

// ---- the statistics pass (straight-line code: every loop unrolls, so the kernels keep it in registers) ----------------------------------------------------------

// X = sP_{t+1} G_t^T from F, Q, P_t, sP_{t+1} (row-major D x D).  false: chol(S_t) failed by dt_chol's rule; X is then NaN (and so are the sums it enters,
// which the M-step refuses).
template <int D> AX_HD bool em_lag_one(const double* F, const double* Q, const double* P, const double* sPn, double* X) {
    double FP[D * D], M[D * D], S[D * D], L[D * D], G[D * D];
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j < D; ++j) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < D; ++k) s += F[i * D + k] * P[k * D + j];
            FP[i * D + j] = s;
        }
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j < D; ++j) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < D; ++k) s += FP[i * D + k] * F[j * D + k];
            M[i * D + j] = s + Q[i * D + j];
        }
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j < D; ++j) S[i * D + j] = 0.5 * (M[i * D + j] + M[j * D + i]);
    // dt_chol's recursion and pivot rule, without the early return
    bool ok = true;
#pragma unroll
    for (int j = 0; j < D; ++j) {
        double d = S[j * D + j];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= L[j * D + k] * L[j * D + k];
        ok = ok && (d > DT_PIVOT_TOL * S[j * D + j]) && finite_(d);
        const double dj = sqrt(d);
        L[j * D + j] = dj;
#pragma unroll
        for (int i = j + 1; i < D; ++i) {
            double s = S[i * D + j];
#pragma unroll
            for (int k = 0; k < j; ++k) s -= L[i * D + k] * L[j * D + k];
            L[i * D + j] = s / dj;
        }
    }
    // G = (P F^T) L^-T L^-1: dt_solve_right_lt, then dt_solve_right_l
#pragma unroll
    for (int i = 0; i < D; ++i) {
#pragma unroll
        for (int j = 0; j < D; ++j) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < D; ++k) s += P[i * D + k] * F[j * D + k];
            G[i * D + j] = s;
        }
#pragma unroll
        for (int j = 0; j < D; ++j) {
            double s = G[i * D + j];
#pragma unroll
            for (int k = 0; k < j; ++k) s -= G[i * D + k] * L[j * D + k];
            G[i * D + j] = s / L[j * D + j];
        }
#pragma unroll
        for (int j = D - 1; j >= 0; --j) {
            double s = G[i * D + j];
#pragma unroll
            for (int k = j + 1; k < D; ++k) s -= G[i * D + k] * L[k * D + j];
            G[i * D + j] = s / L[j * D + j];
        }
    }
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j < D; ++j) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < D; ++k) s += sPn[i * D + k] * G[j * D + k];
            X[i * D + j] = ok ? s : (double)NAN;
        }
    return ok;
}

// acc += the lower triangle of E[z z^T] for z = [x; 1], x ~ (sm, sP): n (n + 1) / 2 sums, dt_tri's order
template <int D> AX_HD void em_acc_zz(const double* sm, const double* sP, double* acc) {
    int o = 0;
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) acc[o++] += sP[i * D + j] + sm[i] * sm[j];
#pragma unroll
    for (int j = 0; j < D; ++j) acc[o++] += sm[j];
    acc[o] += 1.0;
}

// acc += the packed dynamics statistics of ONE transition t -> t + 1 (dynamics_theta.h's layout, DtDims<D>::PACKED sums)
template <int D> AX_HD void em_acc_dyn(const double* smt, const double* sPt, const double* smn, const double* sPn, const double* X, double* acc) {
    using S = DtDims<D>;
    em_acc_zz<D>(smt, sPt, acc);
    int o = S::ZZ;
#pragma unroll
    for (int i = 0; i < D; ++i) {
#pragma unroll
        for (int j = 0; j < D; ++j) acc[o++] += X[i * D + j] + smn[i] * smt[j];
        acc[o++] += smn[i];
    }
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) acc[o++] += sPn[i * D + j] + smn[i] * smn[j];
}

// acc += the packed observation statistics of ONE observed step: [lower triangle of E[z z^T] | y E[z]^T]
template <int D, int DY> AX_HD void em_acc_obs(const double* y, const double* sm, const double* sP, double* acc) {
    constexpr int n = D + 1;
    em_acc_zz<D>(sm, sP, acc);
    int o = n * (n + 1) / 2;
#pragma unroll
    for (int i = 0; i < DY; ++i) {
#pragma unroll
        for (int j = 0; j < D; ++j) acc[o++] += y[i] * sm[j];
        acc[o++] += y[i];
    }
}

// packed observation sums -> [So_zz (n, n) | S_yz (dy, n)]
AX_HD void em_unpack_obs(int dx, int dy, const double* p, double* f) {
    const int n = dx + 1, zz = n * (n + 1) / 2;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j <= i; ++j) f[i * n + j] = f[j * n + i] = p[dt_tri(i, j)];
    for (int k = 0; k < dy * n; ++k) f[n * n + k] = p[zz + k];
}

// ---- the M-steps (off the throughput path; every bound a compile-time constant) ---------------------------------------------------------------------------------------------------------

// the regression both likelihood M-steps are: the RR rows of Sab (RR x N) against the Gram matrix Saa (N x N), residual of Sbb (RR x RR) over cnt.
//   U = chol(Saa), Y = Sab U^-T, coef = Y U^-1, res = sym(Sbb - Y Y^T) / cnt.  coef (RR x N), res (RR x RR); work: EmWork<N, RR>::SIZE doubles (the kernel
//   hands in LDS, so that its one lane indexes memory and not registers)
template <int N, int RR> struct EmWork {
    static constexpr int SIZE = N * N + RR * N + RR * RR;
};
template <int N, int RR> AX_HD int em_regress(const double* Saa, const double* Sab, const double* Sbb, double cnt, double* coef, double* res, double* work) {
    double *U = work, *Y = work + N * N, *Lr = work + N * N + RR * N;
    if (!(cnt >= 1.0) || !dt_chol<N>(Saa, U)) return EM_FAIL_GRAM;
    for (int k = 0; k < RR * N; ++k) Y[k] = Sab[k];
    dt_solve_right_lt<RR, N>(Y, U);
    for (int k = 0; k < RR * N; ++k) coef[k] = Y[k];
    dt_solve_right_l<RR, N>(coef, U);
    bool lost = false;
    for (int i = 0; i < RR; ++i)
        for (int j = 0; j <= i; ++j) {
            double yy = 0.0;
            for (int k = 0; k < N; ++k) yy += Y[i * N + k] * Y[j * N + k];
            const double v = Sbb[i * RR + j] - yy;
            res[i * RR + j] = res[j * RR + i] = v / cnt;
            if (i == j && !(v > DT_PIVOT_TOL * Sbb[i * RR + j])) lost = true;  // nothing left of the diagonal after the cancellation
        }
    if (lost || !dt_chol<RR>(res, Lr)) return EM_FAIL_RESIDUAL;
    return EM_OK;
}

// dynamics, maximum likelihood, from the FULL dynamics statistics [S_zz | S_xz | S_xx] -> A = [F b] (D x n), Q (D x D)
template <int D> AX_HD int em_mstep_dyn_ml(const double* full, double* A, double* Q, double* work /* EmWork<D + 1, D> */) {
    constexpr int n = D + 1;
    return em_regress<n, D>(full, full + n * n, full + n * n + D * n, full[n * n - 1], A, Q, work);
}
// dynamics, the joint mode under the matrix-normal inverse-Wishart prior: A = M_n, Q = Psi_n / (nu_n + D + n + 1)
template <int D> AX_HD int em_mstep_dyn_map(const double* full, const DtPrior<D>& pr, double* A, double* Q) {
    using S = DtDims<D>;
    constexpr int n = S::n;
    double post[S::POST], U[n * n], L[D * D];
    const double ntr = full[n * n - 1];
    if (!finite_(ntr)) return EM_FAIL_GRAM;
    const int flag = dt_posterior<D>(full, (int)ntr, pr, post, U, L);
    if (flag != DT_OK) return flag == DT_FAIL_KN ? EM_FAIL_GRAM : EM_FAIL_RESIDUAL;
    const double den = post[S::XZ + n * n] + (double)(D + n + 1);
    for (int k = 0; k < D * n; ++k) A[k] = post[k];
    const double* Psi = post + S::XZ + n * n + 1;
    for (int i = 0; i < D; ++i)
        for (int j = 0; j <= i; ++j) Q[i * D + j] = Q[j * D + i] = Psi[i * D + j] / den;
    return EM_OK;
}
// observations from [So_zz (n, n) | S_yz (DY, n)], S_yy (DY, DY) and n_obs -> HC = [H c] (DY x n), R (DY x DY)
template <int D, int DY> AX_HD int em_mstep_obs(const double* obs, const double* Syy, double nobs, double* HC, double* R, double* work /* EmWork<D + 1, DY> */) {
    constexpr int n = D + 1;
    return em_regress<n, DY>(obs, obs + n * n, Syy, nobs, HC, R, work);
}
// initial state from the nseq sequences' (sm_0, sP_0), `stride` doubles apart -> m0 (D), P0 (D x D).  Sums in ascending sequence order.
template <int D> AX_HD int em_mstep_init(int nseq, const double* init, long long stride, double* m0, double* P0) {
    double L[D * D];
    if (nseq < 1) return EM_FAIL_GRAM;
    for (int i = 0; i < D; ++i) {
        double s = 0.0;
        for (int q = 0; q < nseq; ++q) s += init[q * stride + i];
        m0[i] = s / (double)nseq;
    }
    for (int i = 0; i < D; ++i)
        for (int j = 0; j <= i; ++j) {
            double s = 0.0;
            for (int q = 0; q < nseq; ++q) {
                const double* e = init + q * stride;
                s += e[D + i * D + j] + (e[i] - m0[i]) * (e[j] - m0[j]);
            }
            P0[i * D + j] = P0[j * D + i] = s / (double)nseq;
        }
    return dt_chol<D>(P0, L) ? EM_OK : EM_FAIL_RESIDUAL;
}

}  // namespace ax
