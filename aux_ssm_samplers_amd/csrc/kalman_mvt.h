// kalman_mvt.h -- the batched multivariate-t sweep (AUXSSM_KMODEL_MVT_FIRST / _SECOND) as api.hip hands it to kalman_mvt.hip.
// Host-side declarations only: nothing here is compiled for the device, and no other unit includes it.
#pragma once
#include "ctx.h"

namespace ax {

// One sweep up to (not including) the accept / select step.  Everything per-chain is dense (C, T, D); the model is d independent scalar random-walk
// LGSSMs coupled through the potential: m0, P0, F, Q, b are (D) vectors of the sweep's dtype, prec (D, D) row-major, nu one device scalar.
struct MvtArgs {
    int C, T, D, order;       // order: 1 or 2 (the first- / second-order auxiliary observation factory)
    double delta;             // host step size (a placeholder when dptr is set)
    const double* dptr;       // device-resident {delta, sqrt(delta / 2)}, or null
    const void *m0, *P0, *F, *Q, *b, *prec, *nu;
    const void* yobs;         // (T, D), time stride y_st elements
    long long y_st;
    const void *x, *eps_aux, *eps_samp;
    void* xp;                 // out: the proposal x'
    Acc* sums;                // out [5][C]: lp_prop, lp_rev (the filters' log-likelihoods already taken off, in Acc), lt_prop, lt_rev, corr
    void* ell0;               // out (C): zeros, the `ell` launch_accept subtracts
};
size_t mvt_ws_bytes(int dtype, int C, int T, int D);  // what run_mvt takes from the handle's slab (reserved by the caller)
int run_mvt(auxssm_ctx* h, int dtype, const MvtArgs& a);

}  // namespace ax
