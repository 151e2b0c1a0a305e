// csmc_chain.hip -- the sequential conditional-SMC sweep on PER-CHAIN, time-invariant linear-Gaussian transitions (auxssm_csmc_sweep_chain_dynamics: the x | theta, y
// half of particle Gibbs over (x, F, b, Q)) and the commit of a conjugate draw into the arrays it reads (auxssm_csmc_dynamics_commit: the theta | x half is
// dynamics_theta.hip's).  Compiled with -ffp-contract=off, as csmc.hip.
//
// The sweep is csmc.hip's: csmc_sweep_impl validates, plans the workspace, batches the chains and hands run_csmc_chain the same CsmcArgs.  What differs is where a
// step's transition comes from -- row c0 + blockIdx.x of the per-chain arrays instead of the kernel argument -- and that is a property of the kernels' model POLICY
// (csmc_sweep.h::FkBuiltinChain, ChainDyn), so this unit holds its own instantiations of k_csmc_grad / k_csmc_fwd / k_csmc_bwd and csmc.hip's keep their code:
//   k_csmc_fwd<R, D, false, GRAD, nw, 0, FkBuiltinChain<R, D, V>>      V != SEP: the generic workgroup for every N, as in csmc.hip::fwd_kernel
//   k_csmc_fwd<float, 1, false, false, 16, 1, FkBuiltinChain<float, 1>>  config C3's shape, the model kinds folded as in the shared-parameter sweep
//   k_csmc_bwd<R, D, false, nw, FkBuiltinChain<R, D>>
// Each workgroup copies its chain's row into scalar registers before its time loop (csmc_sweep.h::TransC); the constants and reciprocal diagonals of the C factors
// come from k_csmc_ctrans, the kernel of the time-varying transitions, run over C rows -- so a chain's sweep is bit for bit the one-chain time-varying sweep whose
// T - 1 rows repeat that chain's (F, b, chol_Q) (tests/test_gpu_csmc_chain_dynamics.py).
// Not here: guided proposals (their K_t / chol Lambda_t tables would be per chain and step), dx > 4, the Lorenz-63 transition, user programs, the parallel-in-time sweep.
#include "csmc_host.h"
#include "chain_dynamics.h"

namespace ax {

template <typename R, int D> static bool c3_shape_chain(const FkDev<R>& m, const CsmcArgs& a, int nw) {
    return D == 1 && sizeof(R) == 4 && nw == 16 && !m.gradient && m.proposal == AUXSSM_PROP_AUX_INDEPENDENT && m.potential == AUXSSM_POT_SV && a.As == nullptr &&
           a.noise_mode != AUXSSM_NOISE_EXPLICIT && !a.pregen;
}
template <typename R, int D> static SweepKernel<R> fwd_kernel_chain(const FkDev<R>& m, const CsmcArgs& a, int nw) {
    return with_bool(m.gradient != 0, [&](auto gr) {
        return with_pot(m.potential, [&](auto pv) -> SweepKernel<R> {
            constexpr bool GR = decltype(gr)::value, SEP = decltype(pv)::value == PotV::SEP;
            using P = FkBuiltinChain<R, D, decltype(pv)::value>;
            if constexpr (D == 1 && sizeof(R) == 4 && !GR && SEP) {
                if (c3_shape_chain<R, D>(m, a, nw)) return k_csmc_fwd<R, D, false, false, 16, 1, P>;
            }
            if constexpr (!SEP) return k_csmc_fwd<R, D, false, GR, 0, 0, P>;
            else return with_nw(nw, [&](auto n) -> SweepKernel<R> { return k_csmc_fwd<R, D, false, GR, decltype(n)::value, 0, P>; });
        });
    });
}
template <typename R, int D> static SweepKernel<R> bwd_kernel_chain(int nw) {
    return with_nw(nw, [&](auto n) -> SweepKernel<R> { return k_csmc_bwd<R, D, false, decltype(n)::value, FkBuiltinChain<R, D>>; });
}

// run_csmc (csmc.hip) on per-chain transitions; ctt: C (1 + D) reals of workspace for the constants and the reciprocal diagonals of the C factors
template <typename R, int D>
static int run_csmc_chain_rd(auxssm_ctx* h, const auxssm_fk_model* fk, const auxssm_fk_chain_dynamics* dyn, CsmcArgs& a, void* ctt) {
    FkDev<R> m = fk_dev<R>(fk);
    m.Ft = (const R*)dyn->F;
    m.bt = (const R*)dyn->b;
    m.LQt = (const R*)dyn->chol_Q;
    m.ctt = (const R*)ctt;
    m.idt = (const R*)ctt + a.C;
    hipLaunchKernelGGL((k_csmc_ctrans<R>), dim3((a.C + 255) / 256), dim3(256), 0, h->stream, a.C, D, m.LQt, (R*)ctt, (R*)ctt + a.C);
    // (fk->F_t is NULL -- csmc_sweep_impl has refused anything else -- so the prologue leaves the five pointers as they are)
    int rc = csmc_prologue<R>(h, fk, a, nullptr, m, false, [&] {
        const dim3 grid((unsigned)(((long long)a.C * a.T + 255) / 256));
        with_pot(m.potential, [&](auto pv) { hipLaunchKernelGGL((k_csmc_grad<R, D, FkBuiltinChain<R, D, decltype(pv)::value>>), grid, dim3(256), 0, h->stream, a, m); });
        return (int)AUXSSM_OK;
    });
    if (rc) return rc;
    const int TB = (a.N + 63) / 64 * 64, nw = nw_class(a.N);
    const int cb = a.cb > 0 ? a.cb : a.C;
    for (int c0 = 0; c0 < a.C; c0 += cb) {
        const CsmcArgs ab = csmc_batch(a, c0, cb);
        {
            ProfScope ps(h, AUXSSM_K_CSMC_FWD);
            if ((rc = launch(h, fwd_kernel_chain<R, D>(m, ab, nw), dim3(ab.C), dim3(TB), fwd_lds(TB, D, sizeof(R)), ab, m))) return rc;
        }
        {
            ProfScope ps(h, AUXSSM_K_CSMC_BWD);
            if ((rc = launch(h, bwd_kernel_chain<R, D>(nw), dim3(ab.C), dim3(TB), bwd_lds(TB, D, sizeof(R)), ab, m))) return rc;
        }
    }
    AX_HIP(hipGetLastError());
    return AUXSSM_OK;
}

int run_csmc_chain(auxssm_ctx* h, int dtype, const auxssm_fk_model* fk, const auxssm_fk_chain_dynamics* dyn, CsmcArgs& a, void* ctt) {
    return csmc_dispatch(dtype, fk->dx, [&](auto r, auto d) { return run_csmc_chain_rd<decltype(r), decltype(d)::value>(h, fk, dyn, a, ctt); });
}

// one lane per chain: chain_dynamics.h::cd_commit
template <typename R, int D>
__global__ void __launch_bounds__(64) k_cd_commit(int C, const R* __restrict__ Fn, const R* __restrict__ bn, const R* __restrict__ Qn, const int32_t* step_flags,
                                                  R* __restrict__ F, R* __restrict__ b, R* __restrict__ Q, R* __restrict__ LQ, int32_t* flags) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const long long m = (long long)c * D * D, v = (long long)c * D;
    flags[c] = cd_commit<R, D>(step_flags[c], Fn + m, bn + v, Qn + m, F + m, b + v, Q + m, LQ + m);
}

}  // namespace ax

using namespace ax;

extern "C" int auxssm_csmc_dynamics_commit(auxssm_handle h, int dtype, int32_t C, int32_t dx, const void* F_new, const void* b_new, const void* Q_new,
                                           const int32_t* step_flags, void* F, void* b, void* Q, void* chol_Q, int32_t* flags) {
    AX_NEED_H(h);
    if (int rc = check_dtype(dtype)) return rc;
    if (C < 1) {
        set_error("need C >= 1 chains (got C=%d)", C);
        return AUXSSM_ERR_ARG;
    }
    if (dx < 1) {
        set_error("need dx >= 1 (got dx=%d)", dx);
        return AUXSSM_ERR_ARG;
    }
    if (dx > CS_MAXD) {
        set_error("dx=%d: per-chain dynamics belong to the register sweep kernels, dx <= %d", dx, CS_MAXD);
        return AUXSSM_ERR_UNSUPPORTED;
    }
    const void* ptrs[] = {F_new, b_new, Q_new, step_flags, F, b, Q, chol_Q, flags};
    const char* names[] = {"F_new", "b_new", "Q_new", "step_flags", "F", "b", "Q", "chol_Q", "flags"};
    for (int k = 0; k < 9; ++k)
        if (!ptrs[k]) {
            set_error("%s must be non-NULL", names[k]);
            return AUXSSM_ERR_ARG;
        }
    if (F_new == F || b_new == b || Q_new == Q) {  // (a commit in place could not leave a refused chain's live values untouched)
        set_error("%s is its own staging buffer: the draw is committed from staging buffers into the live ones", F_new == F ? "F" : (b_new == b ? "b" : "Q"));
        return AUXSSM_ERR_ARG;
    }
    const unsigned grid = (unsigned)((C + 63) / 64);
    csmc_dispatch(dtype, dx, [&](auto r, auto d) {
        using R = decltype(r);
        constexpr int D = decltype(d)::value;
        hipLaunchKernelGGL((k_cd_commit<R, D>), dim3(grid), dim3(64), 0, h->stream, C, (const R*)F_new, (const R*)b_new, (const R*)Q_new, step_flags, (R*)F, (R*)b,
                           (R*)Q, (R*)chol_Q, flags);
        return (int)AUXSSM_OK;
    });
    AX_HIP(hipGetLastError());
    return AUXSSM_OK;
}
