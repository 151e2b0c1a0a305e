// dynamics_theta.h -- the arithmetic of the conjugate Gibbs step for linear-Gaussian dynamics x_{t+1} = F x_t + b + N(0, Q) (csrc/dynamics_theta.hip): the
// sufficient statistics of one transition, the matrix-normal inverse-Wishart posterior, the draw, and the Marsaglia-Tsang gamma generator.  AX_HD functions only:
// the kernels compile this text for gfx950 and tests/hostsim_dynamics_theta compiles it with g++ (tests/dynamics_theta_np.py is its literal NumPy restatement).
// Everything here is in double, whatever the state's type; units that include it are built with -ffp-contract=off.
//
// With z_t = [x_t; 1] (n = D + 1), A = [F b] (D x n) and the T - 1 transitions t = 0 .. T - 2:
//   prior       Q ~ IW(nu0, Psi0),  A | Q ~ MN(M0, Q, K0^-1)
//   statistics  S_zz = sum z_t z_t^T (n x n),  S_xz = sum x_{t+1} z_t^T (D x n),  S_xx = sum x_{t+1} x_{t+1}^T (D x D)
//   posterior   K_n = K0 + S_zz,  M_n = (M0 K0 + S_xz) K_n^-1,  nu_n = nu0 + T - 1,  Psi_n = sym(Psi0 + S_xx + M0 K0 M0^T - M_n K_n M_n^T)
//   draw        L = chol(Psi_n), U = chol(K_n), B lower with B_ii = sqrt(chi_i), chi_i ~ chi^2(nu_n - i), B_ij ~ N(0, 1) (i > j):
//               Q = L B^-T B^-1 L^T,  A = M_n + chol(Q) E U^-1 with E (D x n) standard normals.
// PACKED statistics (what a lane accumulates and a segment writes): [lower triangle of S_zz, row-major (i >= j) | S_xz row-major | lower triangle of S_xx]:
// n (n + 1) / 2 + D n + D (D + 1) / 2 sums, 45 at D = 4.  FULL statistics (auxssm_dynamics_stats): [S_zz (n x n) | S_xz (D x n) | S_xx (D x D)] row-major.
#pragma once
#include "rng.h"

namespace ax {

constexpr int DT_MAX_D = 4;
constexpr int DT_THREADS = 256;          // lanes of one statistics workgroup
constexpr int DT_CM_LANES = 64;          // chain-minor: chains per workgroup (one wave across chains) ...
constexpr int DT_CM_SLICES = 4;          // ... times this many interleaved time slices
constexpr int DT_GAMMA_ATTEMPTS = 16;    // cap of the gamma rejection loop: a proposal is accepted with probability > 0.95, so the cap is met with p < 1e-20
// a Cholesky pivot (or a diagonal entry of Psi_n) below this fraction of the quantity it is the remainder of is rounding noise: the factorisation FAILS
constexpr double DT_PIVOT_TOL = 1.4210854715202004e-14;  // 2^-46

// transitions per segment of the statistics pass: a function of T alone (so a chain's partial sums, and their order, do not depend on the batch it is in)
// A constant today: 512 keeps 128 workgroups busy at one chain of T = 65 536 and gives a dense lane two transitions.  T is a parameter so that the length may grow
// with T (fewer block reductions per byte in the dense kernel, which is bound by them at a few chains) without touching a caller: whatever it returns must
// remain a function of T alone, and tests/dynamics_theta_np.py::SEGMENT_LEN and the cells built on it follow it.
AX_HD int dt_segment_len(int T) { (void)T; return 512; }
AX_HD int dt_num_segments(int T) { return (T - 1 + dt_segment_len(T) - 1) / dt_segment_len(T); }

template <int D> struct DtDims {
    static constexpr int n = D + 1;
    static constexpr int ZZ = n * (n + 1) / 2, XZ = D * n, XX = D * (D + 1) / 2;
    static constexpr int PACKED = ZZ + XZ + XX;
    static constexpr int FULL = n * n + D * n + D * D;
    static constexpr int POST = D * n + n * n + 1 + D * D;  // post_out: [M_n | K_n | nu_n | Psi_n]
};
AX_HD int dt_tri(int i, int j) { return i * (i + 1) / 2 + j; }  // (i >= j)

// acc += the packed statistics of ONE transition x_t -> x_{t+1}; the products are formed in double
template <int D> AX_HD void dt_accumulate(const double* xt, const double* xn, double* acc) {
    using S = DtDims<D>;
    double z[S::n];
#pragma unroll
    for (int k = 0; k < D; ++k) z[k] = xt[k];
    z[D] = 1.0;
    int o = 0;
#pragma unroll
    for (int i = 0; i < S::n; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) acc[o++] += z[i] * z[j];
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j < S::n; ++j) acc[o++] += xn[i] * z[j];
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) acc[o++] += xn[i] * xn[j];
}

// packed -> full (both triangles of the symmetric parts from the one stored sum: symmetric bit for bit)
template <int D> AX_HD void dt_unpack(const double* p, double* f) {
    using S = DtDims<D>;
    constexpr int n = S::n;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j <= i; ++j) f[i * n + j] = f[j * n + i] = p[dt_tri(i, j)];
    for (int k = 0; k < S::XZ; ++k) f[n * n + k] = p[S::ZZ + k];
    for (int i = 0; i < D; ++i)
        for (int j = 0; j <= i; ++j) f[n * n + S::XZ + i * D + j] = f[n * n + S::XZ + j * D + i] = p[S::ZZ + S::XZ + dt_tri(i, j)];
}

// lower Cholesky factor of the N x N matrix a (lower triangle read) -> l (upper triangle zero).  false: a pivot is not finite, not positive, or below
// DT_PIVOT_TOL of its diagonal entry (l is then incomplete).
template <int N> AX_HD bool dt_chol(const double* a, double* l) {
    for (int k = 0; k < N * N; ++k) l[k] = 0.0;
    for (int j = 0; j < N; ++j) {
        double d = a[j * N + j];
        for (int k = 0; k < j; ++k) d -= l[j * N + k] * l[j * N + k];
        if (!(d > DT_PIVOT_TOL * a[j * N + j]) || !finite_(d)) return false;
        const double dj = sqrt(d);
        l[j * N + j] = dj;
        for (int i = j + 1; i < N; ++i) {
            double s = a[i * N + j];
            for (int k = 0; k < j; ++k) s -= l[i * N + k] * l[j * N + k];
            l[i * N + j] = s / dj;
        }
    }
    return true;
}
// X <- X U^-T (rows r, U lower N x N): column j = (x_j - sum_{k < j} X_k U_jk) / U_jj, ascending j
template <int R_, int N> AX_HD void dt_solve_right_lt(double* x, const double* u) {
    for (int r = 0; r < R_; ++r)
        for (int j = 0; j < N; ++j) {
            double s = x[r * N + j];
            for (int k = 0; k < j; ++k) s -= x[r * N + k] * u[j * N + k];
            x[r * N + j] = s / u[j * N + j];
        }
}
// X <- X U^-1 (rows r, U lower N x N): column j = (x_j - sum_{k > j} X_k U_kj) / U_jj, descending j
template <int R_, int N> AX_HD void dt_solve_right_l(double* x, const double* u) {
    for (int r = 0; r < R_; ++r)
        for (int j = N - 1; j >= 0; --j) {
            double s = x[r * N + j];
            for (int k = j + 1; k < N; ++k) s -= x[r * N + k] * u[k * N + j];
            x[r * N + j] = s / u[j * N + j];
        }
}

// the prior as the kernels take it (auxssm_mniw_prior with the leading D x n, n x n, D x D blocks packed to the state's size)
template <int D> struct DtPrior {
    double M0[D * (D + 1)], K0[(D + 1) * (D + 1)], Psi0[D * D], nu0, chi_scale;
};

enum DtFlag { DT_OK = 0, DT_FAIL_KN = 1, DT_FAIL_PSI = 2, DT_FAIL_CHI = 3, DT_FAIL_Q = 4 };

// posterior of one chain from its FULL statistics and the number of transitions; post = [M_n | K_n | nu_n | Psi_n]; U = chol(K_n), L = chol(Psi_n).
// -> DT_OK, DT_FAIL_KN (post then holds K_n and nu_n, zeros elsewhere) or DT_FAIL_PSI (post complete)
template <int D> AX_HD int dt_posterior(const double* full, int ntrans, const DtPrior<D>& pr, double* post, double* U, double* L) {
    using S = DtDims<D>;
    constexpr int n = S::n;
    const double *Szz = full, *Sxz = full + n * n, *Sxx = full + n * n + S::XZ;
    double *Mn = post, *Kn = post + S::XZ, *Psi = post + S::XZ + n * n + 1;
    for (int k = 0; k < S::POST; ++k) post[k] = 0.0;
    for (int k = 0; k < n * n; ++k) Kn[k] = pr.K0[k] + Szz[k];
    post[S::XZ + n * n] = pr.nu0 + (double)ntrans;
    if (!dt_chol<n>(Kn, U)) return DT_FAIL_KN;
    // G = M0 K0 + S_xz;  Y = G U^-T;  M_n = Y U^-1;  M_n K_n M_n^T = Y Y^T
    double G[D * n], Y[D * n], M0K0[D * n];
    for (int i = 0; i < D; ++i)
        for (int j = 0; j < n; ++j) {
            double s = 0.0;
            for (int k = 0; k < n; ++k) s += pr.M0[i * n + k] * pr.K0[k * n + j];
            M0K0[i * n + j] = s;
            G[i * n + j] = s + Sxz[i * n + j];
        }
    for (int k = 0; k < D * n; ++k) Y[k] = G[k];
    dt_solve_right_lt<D, n>(Y, U);
    for (int k = 0; k < D * n; ++k) Mn[k] = Y[k];
    dt_solve_right_l<D, n>(Mn, U);
    bool lost = false;
    for (int i = 0; i < D; ++i)
        for (int j = 0; j <= i; ++j) {
            double pm = 0.0, yy = 0.0;
            for (int k = 0; k < n; ++k) pm += M0K0[i * n + k] * pr.M0[j * n + k];
            for (int k = 0; k < n; ++k) yy += Y[i * n + k] * Y[j * n + k];
            const double plus = (pr.Psi0[i * D + j] + Sxx[i * D + j]) + pm;
            const double v = plus - yy;
            Psi[i * D + j] = Psi[j * D + i] = v;
            if (i == j && !(v > DT_PIVOT_TOL * plus)) lost = true;  // nothing left of the diagonal after the cancellation
        }
    if (lost || !dt_chol<D>(Psi, L)) return DT_FAIL_PSI;
    return DT_OK;
}

// the draw: chi (D) chi-square values before scaling, ew (D x D; the strict lower triangle is read), ea (D x n) -> Q (symmetric bit for bit), A = [F b].
// -> DT_OK, DT_FAIL_CHI (a chi that is not positive and finite) or DT_FAIL_Q (chol(Q) failed or a result is not finite); Q / A are then not to be used
template <int D> AX_HD int dt_draw(const double* Mn, const double* U, const double* L, double chi_scale, const double* chi, const double* ew, const double* ea,
                                   double* Q, double* A) {
    constexpr int n = D + 1;
    double B[D * D], W[D * D], Lq[D * D], X[D * n];
    for (int i = 0; i < D; ++i)
        for (int j = 0; j < D; ++j) B[i * D + j] = j < i ? ew[i * D + j] : 0.0;
    for (int i = 0; i < D; ++i) {
        const double c = chi_scale * chi[i];
        if (!(c > 0.0) || !finite_(c)) return DT_FAIL_CHI;
        B[i * D + i] = sqrt(c);
    }
    // W = L B^-T;  Q = W W^T
    for (int k = 0; k < D * D; ++k) W[k] = L[k];
    dt_solve_right_lt<D, D>(W, B);
    for (int i = 0; i < D; ++i)
        for (int j = 0; j <= i; ++j) {
            double s = 0.0;
            for (int k = 0; k < D; ++k) s += W[i * D + k] * W[j * D + k];
            Q[i * D + j] = Q[j * D + i] = s;
        }
    if (!dt_chol<D>(Q, Lq)) return DT_FAIL_Q;
    // A = M_n + chol(Q) (E U^-1)
    for (int k = 0; k < D * n; ++k) X[k] = ea[k];
    dt_solve_right_l<D, n>(X, U);
    bool fin = true;
    for (int i = 0; i < D; ++i)
        for (int j = 0; j < n; ++j) {
            double s = 0.0;
            for (int k = 0; k <= i; ++k) s += Lq[i * D + k] * X[k * n + j];
            A[i * n + j] = Mn[i * n + j] + s;
            fin = fin && finite_(A[i * n + j]);
        }
    for (int k = 0; k < D * D; ++k) fin = fin && finite_(Q[k]);
    return fin ? DT_OK : DT_FAIL_Q;
}

// ---- Gamma(shape, 1) by Marsaglia & Tsang (2000) ------------------------------------------------------------------------------------
// shape a >= 1: d = a - 1/3, c = 1 / sqrt(9 d); attempt k: x ~ N(0, 1), v = (1 + c x)^3, rejected if v <= 0; u ~ U(0, 1); accepted if
// log u < x^2 / 2 + d - d v + d log v; the draw is d v.  shape a < 1: the draw of shape a + 1 times u'^(1 / a).  The logarithms (and the power, as
// exp(log(u') / a)) are det_math.h's fixed sequences, so a host restatement takes the same decisions.  The caller gives each attempt its variates:
// x, u in (0, 1) and u' in (0, 1) -- a pure function of (key, stream, flat index, attempt) in the kernel (dt_gamma_variates).
struct DtGammaShape {
    double d, c, inv_a;  // inv_a = 1 / a for a < 1, else 0 (no boost)
};
inline DtGammaShape dt_gamma_shape(double a) {  // host side: c by the host's sqrt, handed to the kernel as a number
    const double a1 = a < 1.0 ? a + 1.0 : a;
    DtGammaShape s;
    s.d = a1 - 1.0 / 3.0;
    s.c = 1.0 / sqrt(9.0 * s.d);
    s.inv_a = a < 1.0 ? 1.0 / a : 0.0;
    return s;
}
// one attempt: true = accepted, *out the draw; margin (if non-NULL) = threshold - log u, the distance of the decision from its boundary (NaN for v <= 0)
AX_HD bool dt_gamma_attempt(const DtGammaShape& s, double x, double u, double ub, double* out, double* margin) {
    const double t = 1.0 + s.c * x;
    const double v = t * t * t;
    if (margin) *margin = (double)NAN;
    if (!(v > 0.0)) return false;
    const double thr = ((0.5 * x * x + s.d) - s.d * v) + s.d * det_log(v);
    const double lu = det_log(u);
    if (margin) *margin = thr - lu;
    if (!(lu < thr)) return false;
    double g = s.d * v;
    if (s.inv_a != 0.0) g = g * det_exp(det_log(ub) * s.inv_a);
    *out = g;
    return true;
}
// the variates of attempt k of draw number g (flat index into out (n, m)) on the Threefry stream (key, stream): blocks 2 (g ATTEMPTS + k) and that + 1 of
// the stream (rng.h::stream_counter).  x = the cos branch of the fp64 Box-Muller transform of the first block (both dtypes), u and u' = the two words of
// the second one as (b + 1/2) 2^-32, never 0 or 1.
AX_HD void dt_gamma_variates(uint32_t k0, uint32_t k1, uint32_t stream, unsigned long long g, int k, double& x, double& u, double& ub) {
    const unsigned long long blk = 2ull * (g * (unsigned long long)DT_GAMMA_ATTEMPTS + (unsigned long long)k);
    uint32_t a0, a1, b0, b1;
    stream_counter(stream, blk, a0, a1);
    threefry2x32(k0, k1, a0, a1);
    double z1;
    bm_fp64(a0, a1, NormTabGlobal{}, x, z1);
    stream_counter(stream, blk + 1, b0, b1);
    threefry2x32(k0, k1, b0, b1);
    u = ((double)b0 + 0.5) * 2.3283064365386963e-10;
    ub = ((double)b1 + 0.5) * 2.3283064365386963e-10;
}
// draw number g of shape s: the first accepted attempt, NaN if none of DT_GAMMA_ATTEMPTS is
AX_HD double dt_gamma_draw(uint32_t k0, uint32_t k1, uint32_t stream, unsigned long long g, const DtGammaShape& s) {
    for (int k = 0; k < DT_GAMMA_ATTEMPTS; ++k) {
        double x, u, ub, out;
        dt_gamma_variates(k0, k1, stream, g, k, x, u, ub);
        if (dt_gamma_attempt(s, x, u, ub, &out, nullptr)) return out;
    }
    return (double)NAN;
}

}  // namespace ax
