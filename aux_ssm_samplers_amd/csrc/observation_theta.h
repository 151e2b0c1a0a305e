// observation_theta.h -- the arithmetic of the conjugate Gibbs step for the linear-Gaussian observation model y_t = H x_t + c + N(0, R)
// (csrc/observation_theta.hip): the sufficient statistics of one observed step, the matrix-normal inverse-Wishart posterior (H, c, R jointly, or R alone with
// H, c fixed) and the draw.  AX_HD functions only: the kernels compile this text for gfx950 and tests/hostsim_observation_theta compiles it with g++
// (tests/observation_theta_np.py is its literal NumPy restatement).  Everything here is in double, whatever the state's type; units that include it are built
// with -ffp-contract=off.  The factorisation, the two triangular solves and the segment length are dynamics_theta.h's.
//
// With z_t = [x_t; 1] (n = DX + 1), A = [H c] (DY x n) and the steps t = 0 .. T - 1 whose row of y is entirely finite (n_obs of them):
//   prior       R ~ IW(nu0, Psi0),  A | R ~ MN(M0, R, K0^-1)
//   statistics  So_zz = sum z_t z_t^T (n x n),  S_yz = sum y_t z_t^T (DY x n)   [per chain, on the device];   S_yy = sum y_t y_t^T, n_obs   [data only: host]
//   joint       K_n = K0 + So_zz,  M_n = (M0 K0 + S_yz) K_n^-1,  nu_n = nu0 + n_obs,  Psi_n = sym(Psi0 + S_yy + M0 K0 M0^T - M_n K_n M_n^T)
//   R alone     nu_n = nu0 + n_obs,  Psi_n = sym(Psi0 + S_yy - A S_yz^T - S_yz A^T + A So_zz A^T)   (A = the chain's present [H c]; M0, K0 not read)
//   draw        L = chol(Psi_n), U = chol(K_n), B lower with B_ii = sqrt(chi_i), chi_i ~ chi^2(nu_n - i), B_ij ~ N(0, 1) (i > j):
//               R = L B^-T B^-1 L^T,  A = M_n + chol(R) E U^-1 with E (DY x n) standard normals  (joint mode only).
// PACKED statistics (what a lane accumulates and a segment writes): [lower triangle of So_zz, row-major (i >= j) | S_yz row-major]: n (n + 1) / 2 + DY n sums,
// 35 at DX = DY = 4.  FULL statistics (auxssm_observation_stats): [So_zz (n x n) | S_yz (DY x n)] row-major.
#pragma once
#include "dynamics_theta.h"

namespace ax {

constexpr int OT_MAX_D = 4;
constexpr int OT_FIN_LANES = 16;  // chains per workgroup of the finish kernel (one lane per chain, its matrices in LDS)
enum OtMode { OT_JOINT = 1, OT_R_ALONE = 2 };

// segments of the statistics pass: dt_segment_len(T) steps each, over the T steps (the dynamics step has T - 1 transitions)
AX_HD int ot_num_segments(int T) { return (T + dt_segment_len(T) - 1) / dt_segment_len(T); }

template <int DX, int DY> struct OtDims {
    static constexpr int n = DX + 1;
    static constexpr int ZZ = n * (n + 1) / 2, YZ = DY * n;
    static constexpr int PACKED = ZZ + YZ;
    static constexpr int FULL = n * n + DY * n;
    static constexpr int POST = DY * n + n * n + 1 + DY * DY;  // post_out: [M_n | K_n | nu_n | Psi_n]
    // doubles of scratch the posterior and the draw ask their caller for (so that a kernel can keep them out of registers)
    static constexpr int WORK_POST = 2 * DY * n, WORK_DRAW = 3 * DY * DY + DY * n;
    static constexpr int WORK = WORK_POST > WORK_DRAW ? WORK_POST : WORK_DRAW;
};

// a row of y with any non-finite entry is skipped whole
template <int DY> AX_HD bool ot_row_observed(const double* y) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < DY; ++k) ok = ok && finite_(y[k]);
    return ok;
}

// acc += the packed statistics of ONE observed step (x_t, y_t); the products are formed in double
template <int DX, int DY> AX_HD void ot_accumulate(const double* x, const double* y, double* acc) {
    using S = OtDims<DX, DY>;
    double z[S::n];
#pragma unroll
    for (int k = 0; k < DX; ++k) z[k] = x[k];
    z[DX] = 1.0;
    int o = 0;
#pragma unroll
    for (int i = 0; i < S::n; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) acc[o++] += z[i] * z[j];
#pragma unroll
    for (int i = 0; i < DY; ++i)
#pragma unroll
        for (int j = 0; j < S::n; ++j) acc[o++] += y[i] * z[j];
}

// packed -> full (both triangles of So_zz from the one stored sum: symmetric bit for bit)
template <int DX, int DY> AX_HD void ot_unpack(const double* p, double* f) {
    using S = OtDims<DX, DY>;
    constexpr int n = S::n;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j <= i; ++j) f[i * n + j] = f[j * n + i] = p[dt_tri(i, j)];
    for (int k = 0; k < S::YZ; ++k) f[n * n + k] = p[S::ZZ + k];
}

// Joint posterior of one chain from its FULL statistics, the data's S_yy (DY x DY) and n_obs; post = [M_n | K_n | nu_n | Psi_n]; U = chol(K_n), L = chol(Psi_n);
// work: OtDims::WORK_POST doubles.  -> DT_OK, DT_FAIL_KN (no observed row, or chol(K_n) failed: post then holds K_n and nu_n, zeros elsewhere) or
// DT_FAIL_PSI (post complete)
template <int DX, int DY>
AX_HD int ot_posterior_joint(const double* full, const double* Syy, double nobs, const double* M0, const double* K0, const double* Psi0, double nu0, double* post,
                             double* U, double* L, double* work) {
    using S = OtDims<DX, DY>;
    constexpr int n = S::n;
    const double *Szz = full, *Syz = full + n * n;
    double *Mn = post, *Kn = post + S::YZ, *Psi = post + S::YZ + n * n + 1;
    double *M0K0 = work, *Y = work + DY * n;
    for (int k = 0; k < S::POST; ++k) post[k] = 0.0;
    for (int k = 0; k < n * n; ++k) Kn[k] = K0[k] + Szz[k];
    post[S::YZ + n * n] = nu0 + nobs;
    if (!(nobs > 0.0) || !dt_chol<n>(Kn, U)) return DT_FAIL_KN;
    // G = M0 K0 + S_yz;  Y = G U^-T;  M_n = Y U^-1;  M_n K_n M_n^T = Y Y^T
    for (int i = 0; i < DY; ++i)
        for (int j = 0; j < n; ++j) {
            double s = 0.0;
            for (int k = 0; k < n; ++k) s += M0[i * n + k] * K0[k * n + j];
            M0K0[i * n + j] = s;
            Y[i * n + j] = s + Syz[i * n + j];
        }
    dt_solve_right_lt<DY, n>(Y, U);
    for (int k = 0; k < DY * n; ++k) Mn[k] = Y[k];
    dt_solve_right_l<DY, n>(Mn, U);
    bool lost = false;
    for (int i = 0; i < DY; ++i)
        for (int j = 0; j <= i; ++j) {
            double pm = 0.0, yy = 0.0;
            for (int k = 0; k < n; ++k) pm += M0K0[i * n + k] * M0[j * n + k];
            for (int k = 0; k < n; ++k) yy += Y[i * n + k] * Y[j * n + k];
            const double plus = (Psi0[i * DY + j] + Syy[i * DY + j]) + pm;
            const double v = plus - yy;
            Psi[i * DY + j] = Psi[j * DY + i] = v;
            if (i == j && !(v > DT_PIVOT_TOL * plus)) lost = true;  // nothing left of the diagonal after the cancellation
        }
    if (lost || !dt_chol<DY>(Psi, L)) return DT_FAIL_PSI;
    return DT_OK;
}

// Posterior of R alone, A = [H c] (DY x n) fixed: post = [A | So_zz | nu_n | Psi_n], L = chol(Psi_n); work: DY n doubles.
// -> DT_OK, DT_FAIL_KN (no observed row) or DT_FAIL_PSI
template <int DX, int DY>
AX_HD int ot_posterior_r(const double* full, const double* Syy, double nobs, const double* Psi0, double nu0, const double* A, double* post, double* L,
                         double* work) {
    using S = OtDims<DX, DY>;
    constexpr int n = S::n;
    const double *Szz = full, *Syz = full + n * n;
    double *Psi = post + S::YZ + n * n + 1, *AZ = work;
    for (int k = 0; k < S::POST; ++k) post[k] = 0.0;
    for (int k = 0; k < DY * n; ++k) post[k] = A[k];
    for (int k = 0; k < n * n; ++k) post[S::YZ + k] = Szz[k];
    post[S::YZ + n * n] = nu0 + nobs;
    if (!(nobs > 0.0)) return DT_FAIL_KN;
    for (int i = 0; i < DY; ++i)
        for (int j = 0; j < n; ++j) {
            double s = 0.0;
            for (int k = 0; k < n; ++k) s += A[i * n + k] * Szz[k * n + j];
            AZ[i * n + j] = s;
        }
    bool lost = false;
    for (int i = 0; i < DY; ++i)
        for (int j = 0; j <= i; ++j) {
            double aza = 0.0, cross = 0.0;
            for (int k = 0; k < n; ++k) aza += AZ[i * n + k] * A[j * n + k];
            for (int k = 0; k < n; ++k) cross += A[i * n + k] * Syz[j * n + k] + Syz[i * n + k] * A[j * n + k];
            const double plus = (Psi0[i * DY + j] + Syy[i * DY + j]) + aza;
            const double v = plus - cross;
            Psi[i * DY + j] = Psi[j * DY + i] = v;
            if (i == j && !(v > DT_PIVOT_TOL * plus)) lost = true;
        }
    if (lost || !dt_chol<DY>(Psi, L)) return DT_FAIL_PSI;
    return DT_OK;
}

// the draw: chi (DY) chi-square values before scaling, ew (DY x DY; the strict lower triangle is read), ea (DY x n; joint mode) -> Rm (symmetric bit for
// bit) and, joint, A = [H c]; work: OtDims::WORK_DRAW doubles.  -> DT_OK, DT_FAIL_CHI (a chi that is not positive and finite) or DT_FAIL_Q (chol(R) failed
// or a result is not finite); Rm / A are then not to be used
template <int DX, int DY>
AX_HD int ot_draw(bool joint, const double* Mn, const double* U, const double* L, double chi_scale, const double* chi, const double* ew, const double* ea,
                  double* Rm, double* A, double* work) {
    constexpr int n = DX + 1;
    double *B = work, *W = work + DY * DY, *Lr = work + 2 * DY * DY, *X = work + 3 * DY * DY;
    for (int i = 0; i < DY; ++i)
        for (int j = 0; j < DY; ++j) B[i * DY + j] = j < i ? ew[i * DY + j] : 0.0;
    for (int i = 0; i < DY; ++i) {
        const double c = chi_scale * chi[i];
        if (!(c > 0.0) || !finite_(c)) return DT_FAIL_CHI;
        B[i * DY + i] = sqrt(c);
    }
    // W = L B^-T;  R = W W^T
    for (int k = 0; k < DY * DY; ++k) W[k] = L[k];
    dt_solve_right_lt<DY, DY>(W, B);
    for (int i = 0; i < DY; ++i)
        for (int j = 0; j <= i; ++j) {
            double s = 0.0;
            for (int k = 0; k < DY; ++k) s += W[i * DY + k] * W[j * DY + k];
            Rm[i * DY + j] = Rm[j * DY + i] = s;
        }
    if (!dt_chol<DY>(Rm, Lr)) return DT_FAIL_Q;
    bool fin = true;
    for (int k = 0; k < DY * DY; ++k) fin = fin && finite_(Rm[k]);
    if (joint) {
        // A = M_n + chol(R) (E U^-1)
        for (int k = 0; k < DY * n; ++k) X[k] = ea[k];
        dt_solve_right_l<DY, n>(X, U);
        for (int i = 0; i < DY; ++i)
            for (int j = 0; j < n; ++j) {
                double s = 0.0;
                for (int k = 0; k <= i; ++k) s += Lr[i * DY + k] * X[k * n + j];
                A[i * n + j] = Mn[i * n + j] + s;
                fin = fin && finite_(A[i * n + j]);
            }
    }
    return fin ? DT_OK : DT_FAIL_Q;
}

}  // namespace ax
