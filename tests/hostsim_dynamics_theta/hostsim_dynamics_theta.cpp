// TEST INFRASTRUCTURE ONLY: csrc/dynamics_theta.h -- the text the kernels of dynamics_theta.hip compile -- run on the CPU by a plain g++ build, behind a C interface
// for tests/hostsim_dynamics_theta/__init__.py.  One chain at a time, doubles throughout (the caller rounds fp32 inputs itself).
#include <cstdint>

#include "../../aux_ssm_samplers_amd/csrc/dynamics_theta.h"

using namespace ax;

template <int D> static void stats_d(int T, const double* x, double* full) {
    double acc[DtDims<D>::PACKED] = {0};
    for (int t = 0; t + 1 < T; ++t) dt_accumulate<D>(x + (long long)t * D, x + (long long)(t + 1) * D, acc);
    dt_unpack<D>(acc, full);
}
template <int D>
static int update_d(int ntrans, const double* full, const double* M0, const double* K0, double nu0, const double* Psi0, double chi_scale, const double* chi,
                    const double* ew, const double* ea, double* post, double* Q, double* A) {
    constexpr int n = D + 1;
    DtPrior<D> pr;
    for (int k = 0; k < D * n; ++k) pr.M0[k] = M0[k];
    for (int k = 0; k < n * n; ++k) pr.K0[k] = K0[k];
    for (int k = 0; k < D * D; ++k) pr.Psi0[k] = Psi0[k];
    pr.nu0 = nu0;
    pr.chi_scale = chi_scale;
    double U[n * n], L[D * D];
    int flag = dt_posterior<D>(full, ntrans, pr, post, U, L);
    if (flag != DT_OK) return flag;
    return dt_draw<D>(post, U, L, chi_scale, chi, ew, ea, Q, A);
}

extern "C" {

int hs_dt_segment_len(int T) { return dt_segment_len(T); }

int hs_dt_stats(int d, int T, const double* x, double* full) {
    switch (d) {
        case 1: stats_d<1>(T, x, full); return 0;
        case 2: stats_d<2>(T, x, full); return 0;
        case 3: stats_d<3>(T, x, full); return 0;
        case 4: stats_d<4>(T, x, full); return 0;
    }
    return -1;
}

int hs_dt_update(int d, int ntrans, const double* full, const double* M0, const double* K0, double nu0, const double* Psi0, double chi_scale,
                 const double* chi, const double* ew, const double* ea, double* post, double* Q, double* A) {
    switch (d) {
        case 1: return update_d<1>(ntrans, full, M0, K0, nu0, Psi0, chi_scale, chi, ew, ea, post, Q, A);
        case 2: return update_d<2>(ntrans, full, M0, K0, nu0, Psi0, chi_scale, chi, ew, ea, post, Q, A);
        case 3: return update_d<3>(ntrans, full, M0, K0, nu0, Psi0, chi_scale, chi, ew, ea, post, Q, A);
        case 4: return update_d<4>(ntrans, full, M0, K0, nu0, Psi0, chi_scale, chi, ew, ea, post, Q, A);
    }
    return -1;
}

// out (n, m) <- the draws auxssm_rng_gamma defines; margin (n m) <- threshold - log u of the ACCEPTED attempt
int hs_dt_gamma(uint32_t k0, uint32_t k1, uint32_t stream, long long n, int m, const double* shapes, double* out, double* margin) {
    if (m < 1 || m > 8) return -1;
    DtGammaShape s[8];
    for (int i = 0; i < m; ++i) s[i] = dt_gamma_shape(shapes[i]);
    for (long long g = 0; g < n * m; ++g) {
        out[g] = dt_gamma_draw(k0, k1, stream, (unsigned long long)g, s[g % m]);
        margin[g] = (double)NAN;
        for (int k = 0; k < DT_GAMMA_ATTEMPTS; ++k) {
            double x, u, ub, o, mg;
            dt_gamma_variates(k0, k1, stream, (unsigned long long)g, k, x, u, ub);
            if (dt_gamma_attempt(s[g % m], x, u, ub, &o, &mg)) {
                margin[g] = mg;
                break;
            }
        }
    }
    return 0;
}

int hs_dt_gamma_variates(uint32_t k0, uint32_t k1, uint32_t stream, long long g, int k, double* xuu) {
    dt_gamma_variates(k0, k1, stream, (unsigned long long)g, k, xuu[0], xuu[1], xuu[2]);
    return 0;
}

}  // extern "C"
