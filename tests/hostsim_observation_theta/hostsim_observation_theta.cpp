// TEST INFRASTRUCTURE ONLY: csrc/observation_theta.h -- the text the kernels of observation_theta.hip compile -- run on the CPU by a plain g++ build, behind a C
// interface for tests/hostsim_observation_theta/__init__.py.  One chain at a time, doubles throughout (the caller rounds fp32 inputs itself).
#include <cstdint>

#include "../../aux_ssm_samplers_amd/csrc/observation_theta.h"

using namespace ax;

template <int DX, int DY> struct HsOt {
    using S = OtDims<DX, DY>;
    static int stats(int T, const double* x, const double* y, double* full) {
        double acc[S::PACKED] = {0};
        for (int t = 0; t < T; ++t)
            if (ot_row_observed<DY>(y + (long long)t * DY)) ot_accumulate<DX, DY>(x + (long long)t * DX, y + (long long)t * DY, acc);
        ot_unpack<DX, DY>(acc, full);
        return 0;
    }
    // mode 1: joint (A_io is written); mode 2: R alone (A_io is read)
    static int update(int mode, const double* full, const double* syy, double nobs, const double* M0, const double* K0, double nu0, const double* Psi0,
                      double chi_scale, const double* chi, const double* ew, const double* ea, double* post, double* Rm, double* A_io) {
        constexpr int n = S::n;
        double U[n * n] = {0}, L[DY * DY], work[S::WORK];
        const bool joint = mode == OT_JOINT;
        const int flag = joint ? ot_posterior_joint<DX, DY>(full, syy, nobs, M0, K0, Psi0, nu0, post, U, L, work)
                               : ot_posterior_r<DX, DY>(full, syy, nobs, Psi0, nu0, A_io, post, L, work);
        if (flag != DT_OK) return flag;
        return ot_draw<DX, DY>(joint, post, U, L, chi_scale, chi, ew, ea, Rm, A_io, work);
    }
};

template <typename F> static int by_d(int d, F&& f) {
    switch (d) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        case 4: return f(std::integral_constant<int, 4>{});
    }
    return -1;
}

extern "C" {

int hs_ot_num_segments(int T) { return ot_num_segments(T); }

int hs_ot_stats(int dx, int dy, int T, const double* x, const double* y, double* full) {
    return by_d(dx, [&](auto a) { return by_d(dy, [&](auto b) { return HsOt<decltype(a)::value, decltype(b)::value>::stats(T, x, y, full); }); });
}

int hs_ot_update(int dx, int dy, int mode, const double* full, const double* syy, double nobs, const double* M0, const double* K0, double nu0, const double* Psi0,
                 double chi_scale, const double* chi, const double* ew, const double* ea, double* post, double* Rm, double* A_io) {
    return by_d(dx, [&](auto a) {
        return by_d(dy, [&](auto b) {
            return HsOt<decltype(a)::value, decltype(b)::value>::update(mode, full, syy, nobs, M0, K0, nu0, Psi0, chi_scale, chi, ew, ea, post, Rm, A_io);
        });
    });
}

}  // extern "C"
