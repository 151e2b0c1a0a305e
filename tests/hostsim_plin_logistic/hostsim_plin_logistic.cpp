// hostsim_plin_logistic.cpp -- TEST INFRASTRUCTURE ONLY.  Runs the per-step arithmetic of the logistic-linear Kalman factory (csrc/kalman_plin.h::plin_step_logistic,
// AX_HD: the text k_plin_obs_logistic of kalman_plin.hip compiles) on the host, one call per time step, so that value, ys and Om can be checked against the NumPy
// factories of kalman.BinomialLinearModel / NegBinomialLinearModel without a GPU.  A sibling of tests/hostsim_plin.  Never loaded by the product package.
#include "../../aux_ssm_samplers_amd/csrc/kalman_plin.h"

using namespace ax;

// x, u (T, D); y (T, dy); H (dy, D); csw (3, dy) = [c; s; w]  ->  value (T) in double, ys (T, D), Om (T, D, D) full and symmetric (order 2; untouched for order 1)
template <typename R, int D>
static int steps_T(int T, int dy, int order, double delta, const void* x_, const void* u_, const void* y_, const void* H_, const void* csw_, double* value,
                   void* ys_, void* Om_) {
    const R *x = (const R*)x_, *u = (const R*)u_, *y = (const R*)y_, *H = (const R*)H_, *csw = (const R*)csw_;
    R *ys = (R*)ys_, *Om = (R*)Om_;
    for (int t = 0; t < T; ++t) {
        Acc v;
        R om[symsize(D)];
        plin_step_logistic<R, D>(x + (long long)t * D, u + (long long)t * D, y + (long long)t * dy, H, csw, dy, (R)delta, order, v, ys + (long long)t * D, om);
        value[t] = v;
        if (order == 2)
            for (int k = 0; k < D; ++k)
                for (int l = 0; l < D; ++l) Om[((long long)t * D + k) * D + l] = om[sidx(D, k, l)];
    }
    return 0;
}

#define HS_DISPATCH_D(R)                                                                   \
    switch (D) {                                                                           \
        case 1: return steps_T<R, 1>(T, dy, order, delta, x, u, y, H, csw, value, ys, Om); \
        case 2: return steps_T<R, 2>(T, dy, order, delta, x, u, y, H, csw, value, ys, Om); \
        case 3: return steps_T<R, 3>(T, dy, order, delta, x, u, y, H, csw, value, ys, Om); \
        case 4: return steps_T<R, 4>(T, dy, order, delta, x, u, y, H, csw, value, ys, Om); \
    }                                                                                      \
    return -2;

extern "C" int hs_plin_logistic_steps(int dtype, int D, int T, int dy, int order, double delta, const void* x, const void* u, const void* y, const void* H,
                                      const void* csw, double* value, void* ys, void* Om) {
    if (dtype == 0) { HS_DISPATCH_D(float) }
    HS_DISPATCH_D(double)
}
