// hostsim_smooth.cpp -- TEST INFRASTRUCTURE ONLY.  Runs the product's RTS-smoother scan operator (csrc/kalman_bodies.h::SmoothOp, AX_HD) on the host in plain
// loops, with the chunked three-pass structure of kernels.hip.h (chunk reduce -> aggregate scan -> re-walk with the cheap "apply"), so that the operator's math and
// indexing can be checked against the oracle without a GPU.  Never loaded by the product package.
#include <algorithm>
#include <vector>

#include "../../aux_ssm_samplers_amd/csrc/kalman_bodies.h"

using namespace ax;

struct HsArr { const void* ptr; long long sc, st, sb; };
static Arr cv(const HsArr& a) { return Arr{a.ptr, a.sc, a.st, a.sb, 1}; }

template <class Op> static void scan_host(typename Op::Args& a, int S, int n) {
    using Full = typename Op::Full;
    using Pre = typename Op::Pre;
    const ScanLayout lay = Op::layout(a);
    const int E = lay.E, nchunk = lay.nchunk;
    std::vector<Full> agg((size_t)S * nchunk);
    std::vector<Pre> pre((size_t)S * nchunk);
    for (int s = 0; s < S; ++s)
        for (int ch = 0; ch < nchunk; ++ch) {
            const int i0 = ch * E, i1 = std::min(n, i0 + E);
            Full acc;
            Op::load_elem(a, s, i0, acc);
            for (int i = i0 + 1; i < i1; ++i) {
                Full e, o;
                Op::load_elem(a, s, i, e);
                Op::combine(acc, e, o);
                acc = o;
            }
            agg[(size_t)s * nchunk + ch] = acc;
        }
    for (int s = 0; s < S; ++s) {
        Full ex;
        Op::identity(ex);
        for (int ch = 0; ch < nchunk; ++ch) {
            Op::to_pre(ex, pre[(size_t)s * nchunk + ch]);
            Full o;
            Op::combine(ex, agg[(size_t)s * nchunk + ch], o);
            ex = o;
        }
    }
    for (int s = 0; s < S; ++s)
        for (int ch = 0; ch < nchunk; ++ch) {
            const int i0 = ch * E, i1 = std::min(n, i0 + E);
            // through the prefix's memory record, as the device passes hand it over
            typename Op::R rec[Pre::NPAD];
            Pre p;
            Op::store_pre(rec, pre[(size_t)s * nchunk + ch]);
            Op::load_pre(rec, p);
            for (int i = i0; i < i1; ++i) {
                Full e;
                Pre o;
                Op::load_elem(a, s, i, e);
                Op::apply(p, e, o);
                p = o;
                Op::write_out(a, s, i, p);
            }
        }
}

// fly != 0: elements are built by SmoothOpFly in every pass instead of being read back from the element buffer
template <typename R, int D>
static int smooth_T(int C, int T, int B, const HsArr* g, const void* ms, const void* Ps, int E, int fly, void* sms, void* sPs) {
    SmoothArgs a;
    a.d = KDims{C, T, B};
    a.Fs = cv(g[2]); a.Qs = cv(g[3]); a.bs = cv(g[4]);
    const int S = C * B;
    if (E <= 0 || E > T) E = T;
    const int nchunk = (T + E - 1) / E, W = nchunk < 64 ? nchunk : 64;
    a.lay = ScanLayout{E, nchunk, (nchunk + W - 1) / W, W, 0, S};
    a.ms = dense_arr(ms, a.d, D);
    a.Ps = dense_arr(Ps, a.d, D * D);
    a.sms = dense_arr(sms, a.d, D);
    a.sPs = dense_arr(sPs, a.d, D * D);
    std::vector<R> elem((size_t)a.lay.total_reals(T, S, SmoothElem<R, D>::NPAD) + 16);
    a.elem = elem.data();
    if (fly) {
        scan_host<SmoothOpFly<R, D>>(a, S, T);
        return 0;
    }
    DirectIO io;
    for (int s = 0; s < S; ++s) {
        body_smooth_last<R, D>(a, s);
        for (int jp = 0; jp < T - 1; ++jp) body_smooth_init<R, D>(a, io, s, jp, true);
    }
    scan_host<SmoothOp<R, D>>(a, S, T);
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

extern "C" int hs_smooth(int dtype, int D, int C, int T, int B, const HsArr* g, const void* ms, const void* Ps, int E, int fly, void* sms, void* sPs) {
#define CALL_SMOOTH(R, DD) smooth_T<R, DD>(C, T, B, g, ms, Ps, E, fly, sms, sPs)
    if (dtype == 0) { HS_DISPATCH_D(float, CALL_SMOOTH) }
    HS_DISPATCH_D(double, CALL_SMOOTH)
}
