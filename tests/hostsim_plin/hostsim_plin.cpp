// hostsim_plin.cpp -- TEST INFRASTRUCTURE ONLY.  Runs the per-step arithmetic of the Poisson-linear Kalman factory (csrc/kalman_plin.h::plin_step, AX_HD: the text
// the kernels of kalman_plin.hip compile) on the host, one call per time step, so that value, ys and Om can be checked against the NumPy factories without a GPU.
// Never loaded by the product package.
#include "../../aux_ssm_samplers_amd/csrc/kalman_plin.h"

using namespace ax;

// x, u (T, D); y (T, dy); H (dy, D); c (dy)  ->  value (T) in double, ys (T, D), Om (T, D, D) full and symmetric (order 2; untouched for order 1), all row-major
template <typename R, int D>
static int steps_T(int T, int dy, int order, double delta, const void* x_, const void* u_, const void* y_, const void* H_, const void* c_, double* value, void* ys_,
                   void* Om_) {
    const R *x = (const R*)x_, *u = (const R*)u_, *y = (const R*)y_, *H = (const R*)H_, *c = (const R*)c_;
    R *ys = (R*)ys_, *Om = (R*)Om_;
    for (int t = 0; t < T; ++t) {
        Acc v;
        R om[symsize(D)];
        plin_step<R, D>(x + (long long)t * D, u + (long long)t * D, y + (long long)t * dy, H, c, dy, (R)delta, order, v, ys + (long long)t * D, om);
        value[t] = v;
        if (order == 2)
            for (int k = 0; k < D; ++k)
                for (int l = 0; l < D; ++l) Om[((long long)t * D + k) * D + l] = om[sidx(D, k, l)];
    }
    return 0;
}
// log N(y_t; x_t, Om_t) per step with Om (T, D, D) dense (its upper triangle is read): what k_plin_terms adds up
template <typename R, int D> static int norm_T(int T, const void* y_, const void* x_, const void* Om_, double* out) {
    const R *y = (const R*)y_, *x = (const R*)x_, *Om = (const R*)Om_;
    for (int t = 0; t < T; ++t) {
        R om[symsize(D)];
        for (int k = 0; k < D; ++k)
            for (int l = k; l < D; ++l) om[sidx_u(D, k, l)] = Om[((long long)t * D + k) * D + l];
        out[t] = (double)plin_norm_logpdf<R, D>(y + (long long)t * D, x + (long long)t * D, om);
    }
    return 0;
}

#define HS_DISPATCH_D(R, CALL)               \
    switch (D) {                             \
        case 1: return CALL(R, 1);           \
        case 2: return CALL(R, 2);           \
        case 3: return CALL(R, 3);           \
        case 4: return CALL(R, 4);           \
    }                                        \
    return -2;

extern "C" int hs_plin_steps(int dtype, int D, int T, int dy, int order, double delta, const void* x, const void* u, const void* y, const void* H, const void* c,
                             double* value, void* ys, void* Om) {
#define CALL_STEPS(R, DD) steps_T<R, DD>(T, dy, order, delta, x, u, y, H, c, value, ys, Om)
    if (dtype == 0) { HS_DISPATCH_D(float, CALL_STEPS) }
    HS_DISPATCH_D(double, CALL_STEPS)
}
extern "C" int hs_plin_norm(int dtype, int D, int T, const void* y, const void* x, const void* Om, double* out) {
#define CALL_NORM(R, DD) norm_T<R, DD>(T, y, x, Om, out)
    if (dtype == 0) { HS_DISPATCH_D(float, CALL_NORM) }
    HS_DISPATCH_D(double, CALL_NORM)
}
