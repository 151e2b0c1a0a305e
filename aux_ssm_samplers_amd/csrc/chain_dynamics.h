// chain_dynamics.h -- the per-chain body of auxssm_csmc_dynamics_commit (csrc/csmc_chain.hip): what stands between the conjugate draw of (F, b, Q) | x
// (auxssm_dynamics_theta_update, which writes STAGING buffers) and the per-chain transition arrays the cSMC sweep reads (auxssm_csmc_sweep_chain_dynamics).
// AX_HD functions only: the kernel compiles this text for gfx950 and tests/hostsim_chain_dynamics compiles it with g++ (tests/test_csmc_chain_dynamics_host.py
// holds its NumPy restatement).  Units that include it are built with -ffp-contract=off.
//
// Why a commit: the sweep reads chol(Q), in the chains' dtype R, and the draw gives Q.  The factor is taken in double from Q AS ROUNDED TO R -- the matrix the
// live buffer will hold, so that chol_Q chol_Q^T is the live Q to rounding -- and a Q that is positive definite in double may lose that once rounded to fp32.
// The chain's whole quadruple (F, b, Q, chol_Q) is therefore written together or not at all: a sweep never sees a non-finite factor, or an F from one draw
// beside a Q from another.
#pragma once
#include "dynamics_theta.h"

namespace ax {

constexpr int CD_FAIL_ROUNDED_Q = 5;  // after DtFlag's 1 - 4: Q is not positive definite once rounded to R (or an entry of the quadruple is not finite in R)

// One chain.  step_flag: what auxssm_dynamics_theta_update left in its flags for the chain (0, or 1 - 4: its staging values are then stale and are not read).
// Fn (D, D), bn (D), Qn (D, D): the staging values, of type R.  F, b, Q, LQ: the live quadruple (LQ lower, its strict upper triangle zero).
// -> 0 and the live quadruple rewritten, or the code that left it untouched: step_flag, or CD_FAIL_ROUNDED_Q when
//    an entry of Fn / bn / Qn is not finite, dt_chol (double, pivots below 2^-46 of their diagonal entry fail) refuses Qn, or the factor rounded to R has an
//    entry that is not finite or a diagonal entry that is not positive (its reciprocal is what the sweep multiplies by).
template <typename R, int D> AX_HD int cd_commit(int step_flag, const R* Fn, const R* bn, const R* Qn, R* F, R* b, R* Q, R* LQ) {
    if (step_flag != 0) return step_flag;
    double q[D * D], l[D * D];
    bool fin = true;
    for (int k = 0; k < D * D; ++k) {
        q[k] = (double)Qn[k];
        fin = fin && finite_(Qn[k]) && finite_(Fn[k]);
    }
    for (int k = 0; k < D; ++k) fin = fin && finite_(bn[k]);
    if (!fin || !dt_chol<D>(q, l)) return CD_FAIL_ROUNDED_Q;
    R lr[D * D];
    for (int k = 0; k < D * D; ++k) {
        lr[k] = (R)l[k];
        fin = fin && finite_(lr[k]);
    }
    for (int k = 0; k < D; ++k) fin = fin && lr[k * D + k] > (R)0;
    if (!fin) return CD_FAIL_ROUNDED_Q;
    for (int k = 0; k < D * D; ++k) F[k] = Fn[k], Q[k] = Qn[k], LQ[k] = lr[k];
    for (int k = 0; k < D; ++k) b[k] = bn[k];
    return 0;
}

}  // namespace ax
