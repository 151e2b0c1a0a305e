// TEST INFRASTRUCTURE ONLY (plain g++, no GPU): the claim k_fs_mid (csrc/fused_shared.h) rests on.
// The aggregate scan of k_aff_aggs (csrc/kernels.hip.h) carries full affine elements (G_j, e_j) although every G_j is chain-shared.  k_fs_gtab runs the same
// schedule on the matrices alone and records, per Kogge-Stone stage and lane, the lane's matrix at the start of the stage; k_fs_mid then scans the offsets only
// and takes that matrix from the table.  Here both schedules run on the host, the 256 lanes of a workgroup simulated in a loop, with the arithmetic of
// csrc/kalman_math.h (sample_combine / sample_apply against mm / sample_offset); the two exclusive-prefix arrays must be equal byte for byte.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../aux_ssm_samplers_amd/csrc/kalman_math.h"

using namespace ax;

constexpr int TB = 256;  // TB_AGGS
constexpr int NST = 8;   // log2(TB_AGGS)

template <typename R, int D> struct Lanes {
    int nchunk, E2;
    int j0(int tid) const { return std::min(nchunk, tid * E2); }
    int j1(int tid) const { return std::min(nchunk, j0(tid) + E2); }
};

template <typename R, int D> static void identity(SampElem<R, D>& e) {
    for (int i = 0; i < D * D; ++i) e.G[i] = (i / D == i % D) ? (R)1 : (R)0;
    for (int i = 0; i < D; ++i) e.e[i] = 0;
}

// k_aff_aggs, lane by lane: serial product of the lane's chunks, Kogge-Stone over the lanes, exclusive prefixes on the way down
template <typename R, int D> static void scan_full(int nchunk, const R* cprod, const R* agg, R* pre) {
    using Full = SampElem<R, D>;
    using Pre = SampPre<R, D>;
    const Lanes<R, D> L{nchunk, (nchunk + TB - 1) / TB};
    auto load = [&](int j, Full& e) {
        for (int k = 0; k < D * D; ++k) e.G[k] = cprod[(size_t)j * D * D + k];
        for (int k = 0; k < D; ++k) e.e[k] = agg[(size_t)j * D + k];
    };
    std::vector<Full> acc(TB), lds(TB);
    for (int tid = 0; tid < TB; ++tid) {
        identity<R, D>(acc[tid]);
        if (L.j0(tid) < L.j1(tid)) load(L.j0(tid), acc[tid]);
        for (int j = L.j0(tid) + 1; j < L.j1(tid); ++j) {
            Full e, o;
            load(j, e);
            sample_combine<R, D>(acc[tid], e, o);
            acc[tid] = o;
        }
    }
    for (int off = 1; off < TB; off <<= 1) {
        lds = acc;
        for (int tid = off; tid < TB; ++tid) {
            Full o;
            sample_combine<R, D>(lds[tid - off], acc[tid], o);
            acc[tid] = o;
        }
    }
    lds = acc;
    for (int tid = 0; tid < TB; ++tid) {
        Full ex;
        identity<R, D>(ex);
        if (tid > 0) ex = lds[tid - 1];
        Pre p;
        for (int i = 0; i < D; ++i) p.e[i] = ex.e[i];
        for (int j = L.j0(tid); j < L.j1(tid); ++j) {
            for (int i = 0; i < D; ++i) pre[(size_t)j * D + i] = p.e[i];
            if (j + 1 < L.j1(tid)) {
                Full e;
                Pre o;
                load(j, e);
                sample_apply<R, D>(p, e, o);
                p = o;
            }
        }
    }
}

// k_fs_gtab: the same schedule on the matrices alone; tab[stage][lane] = the lane's matrix at the start of the stage
template <typename R, int D> static void build_table(int nchunk, const R* cprod, R* tab) {
    constexpr int DD = D * D;
    const Lanes<R, D> L{nchunk, (nchunk + TB - 1) / TB};
    std::vector<R> G((size_t)TB * DD), lds((size_t)TB * DD);
    for (int tid = 0; tid < TB; ++tid) {
        R* g = &G[(size_t)tid * DD];
        for (int k = 0; k < DD; ++k) g[k] = (k / D == k % D) ? (R)1 : (R)0;
        if (L.j0(tid) < L.j1(tid))
            for (int k = 0; k < DD; ++k) g[k] = cprod[(size_t)L.j0(tid) * DD + k];
        for (int j = L.j0(tid) + 1; j < L.j1(tid); ++j) {
            R o[DD];
            mm<R, D, D, D>(cprod + (size_t)j * DD, g, o);
            for (int k = 0; k < DD; ++k) g[k] = o[k];
        }
    }
    int s = 0;
    for (int off = 1; off < TB; off <<= 1, ++s) {
        std::memcpy(tab + (size_t)s * TB * DD, G.data(), sizeof(R) * TB * DD);
        lds = G;
        for (int tid = off; tid < TB; ++tid) {
            R o[DD];
            mm<R, D, D, D>(&G[(size_t)tid * DD], &lds[(size_t)(tid - off) * DD], o);
            for (int k = 0; k < DD; ++k) G[(size_t)tid * DD + k] = o[k];
        }
    }
}

// k_fs_mid's scan: offsets only
template <typename R, int D> static void scan_offsets(int nchunk, const R* cprod, const R* tab, const R* agg, R* pre) {
    constexpr int DD = D * D;
    const Lanes<R, D> L{nchunk, (nchunk + TB - 1) / TB};
    std::vector<R> acc((size_t)TB * D), lds((size_t)TB * D);
    for (int tid = 0; tid < TB; ++tid) {
        R* a = &acc[(size_t)tid * D];
        for (int i = 0; i < D; ++i) a[i] = 0;
        if (L.j0(tid) < L.j1(tid))
            for (int i = 0; i < D; ++i) a[i] = agg[(size_t)L.j0(tid) * D + i];
        for (int j = L.j0(tid) + 1; j < L.j1(tid); ++j) {
            R o[D];
            sample_offset<R, D>(cprod + (size_t)j * DD, a, agg + (size_t)j * D, o);
            for (int i = 0; i < D; ++i) a[i] = o[i];
        }
    }
    int s = 0;
    for (int off = 1; off < TB; off <<= 1, ++s) {
        lds = acc;
        for (int tid = off; tid < TB; ++tid) {
            R o[D], cur[D];
            for (int i = 0; i < D; ++i) cur[i] = acc[(size_t)tid * D + i];
            sample_offset<R, D>(tab + ((size_t)s * TB + tid) * DD, &lds[(size_t)(tid - off) * D], cur, o);
            for (int i = 0; i < D; ++i) acc[(size_t)tid * D + i] = o[i];
        }
    }
    lds = acc;
    for (int tid = 0; tid < TB; ++tid) {
        R p[D];
        for (int i = 0; i < D; ++i) p[i] = tid > 0 ? lds[(size_t)(tid - 1) * D + i] : (R)0;
        for (int j = L.j0(tid); j < L.j1(tid); ++j) {
            for (int i = 0; i < D; ++i) pre[(size_t)j * D + i] = p[i];
            if (j + 1 < L.j1(tid)) {
                R o[D];
                sample_offset<R, D>(cprod + (size_t)j * DD, p, agg + (size_t)j * D, o);
                for (int i = 0; i < D; ++i) p[i] = o[i];
            }
        }
    }
}

template <typename R, int D> static int check(int nchunk, unsigned seed, const char* rname) {
    constexpr int DD = D * D;
    std::mt19937_64 gen(seed);
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    std::vector<R> cprod((size_t)nchunk * DD), agg((size_t)nchunk * D);
    for (int j = 0; j < nchunk; ++j) {
        for (int k = 0; k < DD; ++k) cprod[(size_t)j * DD + k] = (R)((k / D == k % D ? 0.9 : 0.0) + 0.3 * U(gen));
        for (int i = 0; i < D; ++i) agg[(size_t)j * D + i] = (R)(3.0 * U(gen));
    }
    std::vector<R> want((size_t)nchunk * D, (R)-7), got((size_t)nchunk * D, (R)7), tab((size_t)NST * TB * DD);
    scan_full<R, D>(nchunk, cprod.data(), agg.data(), want.data());
    build_table<R, D>(nchunk, cprod.data(), tab.data());
    scan_offsets<R, D>(nchunk, cprod.data(), tab.data(), agg.data(), got.data());
    const bool same = std::memcmp(want.data(), got.data(), sizeof(R) * want.size()) == 0;
    // the prefixes are not trivially equal: the last one depends on every element before it
    bool moved = nchunk == 1;
    for (size_t k = D; k < want.size(); ++k) moved = moved || want[k] != (R)0;
    std::printf("%s D=%d nchunk=%d: %s\n", rname, D, nchunk, same && moved ? "equal" : "DIFFERENT");
    return same && moved ? 0 : 1;
}

int main() {
    int bad = 0;
    const int sizes[] = {1, 2, 3, 255, 256, 257, 513, 2048};
    unsigned seed = 1;
    for (int n : sizes) {
        bad += check<double, 1>(n, seed++, "fp64");
        bad += check<double, 4>(n, seed++, "fp64");
        bad += check<float, 1>(n, seed++, "fp32");
        bad += check<float, 4>(n, seed++, "fp32");
    }
    return bad ? 1 : 0;
}
