// TEST INFRASTRUCTURE ONLY: csrc/chain_dynamics.h -- the per-chain body of auxssm_csmc_dynamics_commit, the text the kernel of csmc_chain.hip compiles -- run on the
// CPU by a plain g++ build, behind a C interface for tests/hostsim_chain_dynamics/__init__.py.  Chain by chain, in the chains' own type (dtype 0 = float, 1 = double).
#include <cstdint>

#include "../../aux_ssm_samplers_amd/csrc/chain_dynamics.h"

using namespace ax;

template <typename R, int D>
static void commit_rd(int C, const void* Fn, const void* bn, const void* Qn, const int32_t* sf, void* F, void* b, void* Q, void* LQ, int32_t* flags) {
    for (int c = 0; c < C; ++c) {
        const long long m = (long long)c * D * D, v = (long long)c * D;
        flags[c] = cd_commit<R, D>(sf[c], (const R*)Fn + m, (const R*)bn + v, (const R*)Qn + m, (R*)F + m, (R*)b + v, (R*)Q + m, (R*)LQ + m);
    }
}
template <typename R>
static int commit_r(int C, int d, const void* Fn, const void* bn, const void* Qn, const int32_t* sf, void* F, void* b, void* Q, void* LQ, int32_t* flags) {
    switch (d) {
        case 1: commit_rd<R, 1>(C, Fn, bn, Qn, sf, F, b, Q, LQ, flags); return 0;
        case 2: commit_rd<R, 2>(C, Fn, bn, Qn, sf, F, b, Q, LQ, flags); return 0;
        case 3: commit_rd<R, 3>(C, Fn, bn, Qn, sf, F, b, Q, LQ, flags); return 0;
        case 4: commit_rd<R, 4>(C, Fn, bn, Qn, sf, F, b, Q, LQ, flags); return 0;
    }
    return -1;
}

extern "C" int hs_cd_commit(int dtype, int C, int d, const void* Fn, const void* bn, const void* Qn, const int32_t* sf, void* F, void* b, void* Q, void* LQ,
                            int32_t* flags) {
    return dtype == 0 ? commit_r<float>(C, d, Fn, bn, Qn, sf, F, b, Q, LQ, flags) : commit_r<double>(C, d, Fn, bn, Qn, sf, F, b, Q, LQ, flags);
}
