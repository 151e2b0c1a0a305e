// TEST INFRASTRUCTURE ONLY: csrc/lgssm_em.h -- the text the kernels of lgssm_em.hip compile -- run on the CPU by a plain g++ build, behind a C interface for
// tests/hostsim_lgssm_em/__init__.py.  One sequence at a time, doubles throughout.
#include <cmath>
#include <cstdint>

#include "../../aux_ssm_samplers_amd/csrc/lgssm_em.h"

using namespace ax;

template <int D> static int lag_one_d(const double* F, const double* Q, const double* P, const double* sPn, double* X) { return em_lag_one<D>(F, Q, P, sPn, X) ? 0 : 1; }

// FULL statistics of one sequence, step by step in ascending time (the kernels' per-step functions, one accumulator)
template <int D, int DY>
static void stats_d(int T, const double* F, const double* Q, const double* ys, const double* Ps, const double* sms, const double* sPs, double* cross, double* full) {
    constexpr int n = D + 1, DD = D * D, PO = n * (n + 1) / 2 + DY * n;
    double dyn[DtDims<D>::PACKED] = {0}, obs[PO] = {0};
    for (int t = 0; t + 1 < T; ++t) {
        double X[DD];
        em_lag_one<D>(F, Q, Ps + (long long)t * DD, sPs + (long long)(t + 1) * DD, X);
        for (int k = 0; k < DD; ++k) cross[(long long)t * DD + k] = X[k];
        em_acc_dyn<D>(sms + (long long)t * D, sPs + (long long)t * DD, sms + (long long)(t + 1) * D, sPs + (long long)(t + 1) * DD, X, dyn);
    }
    for (int t = 0; t < T; ++t) {
        bool seen = true;
        for (int k = 0; k < DY; ++k) seen = seen && std::isfinite(ys[(long long)t * DY + k]);
        if (seen) em_acc_obs<D, DY>(ys + (long long)t * DY, sms + (long long)t * D, sPs + (long long)t * DD, obs);
    }
    dt_unpack<D>(dyn, full);
    em_unpack_obs(D, DY, obs, full + DtDims<D>::FULL);
    double* init = full + DtDims<D>::FULL + em_obs_full(D, DY);
    for (int k = 0; k < D; ++k) init[k] = sms[k];
    for (int k = 0; k < DD; ++k) init[D + k] = sPs[k];
}
template <int D> static int stats_dy(int dy, int T, const double* F, const double* Q, const double* ys, const double* Ps, const double* sms, const double* sPs, double* cross,
                                     double* full) {
    switch (dy) {
        case 1: stats_d<D, 1>(T, F, Q, ys, Ps, sms, sPs, cross, full); return 0;
        case 2: stats_d<D, 2>(T, F, Q, ys, Ps, sms, sPs, cross, full); return 0;
        case 3: stats_d<D, 3>(T, F, Q, ys, Ps, sms, sPs, cross, full); return 0;
        case 8: stats_d<D, 8>(T, F, Q, ys, Ps, sms, sPs, cross, full); return 0;
    }
    return -1;
}

template <int D> static int dyn_d(const double* full, const double* M0, const double* K0, double nu0, const double* Psi0, double* A, double* Q) {
    constexpr int n = D + 1;
    double work[EmWork<n, D>::SIZE];
    if (!M0) return em_mstep_dyn_ml<D>(full, A, Q, work);
    DtPrior<D> pr;
    for (int k = 0; k < D * n; ++k) pr.M0[k] = M0[k];
    for (int k = 0; k < n * n; ++k) pr.K0[k] = K0[k];
    for (int k = 0; k < D * D; ++k) pr.Psi0[k] = Psi0[k];
    pr.nu0 = nu0;
    pr.chi_scale = 1.0;
    return em_mstep_dyn_map<D>(full, pr, A, Q);
}

template <int D> static int obs_dy(int dy, const double* obs, const double* Syy, double nobs, double* HC, double* R) {
    double work[EmWork<D + 1, 8>::SIZE];
    switch (dy) {
        case 1: return em_mstep_obs<D, 1>(obs, Syy, nobs, HC, R, work);
        case 2: return em_mstep_obs<D, 2>(obs, Syy, nobs, HC, R, work);
        case 3: return em_mstep_obs<D, 3>(obs, Syy, nobs, HC, R, work);
        case 8: return em_mstep_obs<D, 8>(obs, Syy, nobs, HC, R, work);
    }
    return -1;
}

#define BY_D(d, call)               \
    switch (d) {                    \
        case 1: { constexpr int D = 1; return call; } \
        case 2: { constexpr int D = 2; return call; } \
        case 3: { constexpr int D = 3; return call; } \
        case 4: { constexpr int D = 4; return call; } \
    }                               \
    return -1

extern "C" {

int hs_em_ns(int dx, int dy) { return em_ns(dx, dy); }

int hs_em_lag_one(int d, const double* F, const double* Q, const double* P, const double* sPn, double* X) { BY_D(d, lag_one_d<D>(F, Q, P, sPn, X)); }

int hs_em_stats(int d, int dy, int T, const double* F, const double* Q, const double* ys, const double* Ps, const double* sms, const double* sPs, double* cross,
                double* full) {
    BY_D(d, stats_dy<D>(dy, T, F, Q, ys, Ps, sms, sPs, cross, full));
}

// M0 == NULL: maximum likelihood
int hs_em_mstep_dyn(int d, const double* full, const double* M0, const double* K0, double nu0, const double* Psi0, double* A, double* Q) {
    BY_D(d, dyn_d<D>(full, M0, K0, nu0, Psi0, A, Q));
}
int hs_em_mstep_obs(int d, int dy, const double* obs, const double* Syy, double nobs, double* HC, double* R) { BY_D(d, obs_dy<D>(dy, obs, Syy, nobs, HC, R)); }
int hs_em_mstep_init(int d, int nseq, const double* init, long long stride, double* m0, double* P0) { BY_D(d, em_mstep_init<D>(nseq, init, stride, m0, P0)); }

}  // extern "C"
