// csmc.hip -- conditional SMC (particle Gibbs) sweep: reference aux_samplers/_primitives/csmc/csmc.py,
// resamplings.py::multinomial, math/utils.py::normalize, and the auxiliary wrappers csmc/generic.py and
// csmc/independent.py (classical, non-gradient branch).  Compiled with -ffp-contract=off; every multiply-add that
// is meant to be fused is an explicit fma so that the CPU oracle reproduces the arithmetic bit for bit.
//
// Execution model: ONE workgroup per chain, one lane per particle (N <= 1024), a persistent loop over the T
// time steps (the recursion is sequential in t; throughput comes from running >= 256 chains side by side).
// Per step: block inclusive scan of the normalised weights (wave-level Kogge-Stone with shuffles + ordered wave
// totals through LDS) -> N binary searches in LDS (conditional multinomial resampling, index 0 pinned) -> gather
// parents from LDS -> propagate -> pin particle 0 to the reference trajectory -> log-weights -> block max / sum
// -> normalise.  xs, log_ws, As stream to HBM with the particle index fastest (coalesced).
//
// Reduction orders (the contract the oracle restates, SURVEY 7 "bit-exact ancestors"): the sweep kernels follow the "sweep contract"
// of csmc_sweep.h (unnormalised weights exp(lw - max), the hardware's DPP scan order, two-level search, ballot-counted single draw);
// the standalone primitives (normalize / multinomial / systematic) and the parallel-in-time sweep keep the Kogge-Stone-in-64 cumsum,
// the balanced-tree-in-64 sum and the plain binary search of csmc_sweep.h.
//
// Host side: csmc_sweep_impl validates, batches the chains and lays out the workspace (ctx.h::WsPlan); run_csmc / run_csmc_program enqueue the shared
// prologue (csmc_host.h::csmc_prologue) and then, batch by batch, the forward and the backward pass that fwd_kernel / bwd_kernel (a program's module:
// fk_fwd_index / fk_bwd_index) pick for the model and nw_class(N).
#include "csmc_host.h"
#include "fk_program.h"

namespace ax {

// ---- standalone primitives: normalize (math/utils.py:23-39) and conditional multinomial resampling (resamplings.py:14-37),
// one workgroup per row, exactly the block primitives of the forward pass
template <typename R> __global__ void __launch_bounds__(1024) k_normalize_resample(int N, const R* lw, const R* w_in, const R* un, R* w_out, int32_t* idx) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int TB = blockDim.x, nw = TB >> 6, tid = threadIdx.x;
    R* c = (R*)smem;
    R* red = c + TB;
    const long long row = (long long)blockIdx.x * N;
    const bool live = tid < N;
    R w;
    if (lw) {
        w = block_normalize<R>(live ? lw[row + tid] : (R)-INFINITY, red, tid, nw);
        if (live && w_out) w_out[row + tid] = w;
    } else {
        w = live ? w_in[row + tid] : (R)0;
    }
    if (!idx) return;
    block_cumsum<R>(w, c, red, tid, nw);
    if (live) {
        int i = 0;
        if (tid > 0) {
            const R r = c[N - 1] * ((R)1 - un[row + tid]);
            i = lower_bound<R>(c, N, r);
            i = i < N - 1 ? i : N - 1;
        }
        idx[row + tid] = i;
    }
}

// conditional systematic resampling (resamplings.py:40-86; Chopin & Singh, Algorithm 4): M normalised weights -> N indices, index 0 kept at
// position 0.  One workgroup per row; (U, V, W) ~ U[0,1)^3 given per row.  Same block cumsum as the multinomial path.
template <typename R>
__global__ void __launch_bounds__(1024) k_systematic(int M, int N, const R* __restrict__ w_in, const R* __restrict__ uvw, int32_t* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int TB = blockDim.x, nw = TB >> 6, tid = threadIdx.x;
    R* c = (R*)smem;
    R* red = c + TB;
    int* idx = (int*)(red + 48);
    __shared__ int nzero;
    const long long row = blockIdx.x;
    const R w = tid < M ? w_in[row * M + tid] : (R)0;
    if (tid == 0) nzero = 0;
    block_cumsum<R>(w, c, red, tid, nw);
    const R U = uvw[row * 3], V = uvw[row * 3 + 1], W = uvw[row * 3 + 2];
    const R tmp = (R)N * w_in[row * M];
    const R fl = floor(tmp);
    R uni;
    if (tmp <= (R)1) {
        uni = tmp * U;
    } else {
        const R rem = tmp - fl;
        const R p_cond = rem * (fl + (R)1) / tmp;
        uni = V < p_cond ? rem * U : rem + ((R)1 - rem) * U;
    }
    int i = 0;
    if (tid < N) {
        const R pos = ((R)tid + uni) / (R)N;
        i = lower_bound<R>(c, M, pos);
        idx[tid] = i;
        if (i == 0) atomicAdd(&nzero, 1);
    }
    __syncthreads();
    if (tid < N) {
        const int nz = nzero;
        int o = i;
        if (nz != 1) {
            // idx is non-decreasing, so its zeros are the first nz positions: zero_loc[k] = k for k < nz, the fill value -1 otherwise
            const int roll_idx = (int)floor((R)nz * W);
            const int shift = roll_idx < nz ? roll_idx : -1;
            int src = (tid + shift) % N;
            if (src < 0) src += N;
            o = idx[src];
        }
        o = o < 0 ? 0 : (o > M - 1 ? M - 1 : o);
        out[row * N + tid] = o;
    }
}

// (the passes' LDS sizes, the workgroup classes and the kernel-pointer type -- fwd_lds / bwd_lds, nw_class, with_bool / with_nw, SweepKernel -- are csmc_host.h's:
// csmc_chain.hip launches the same passes on per-chain transitions)

// config C3's shape: the one instantiation with the model kinds folded at compile time (SP = 1, csmc_sweep.h)
template <typename R, int D> static bool c3_shape(const FkDev<R>& m, const CsmcArgs& a, int nw) {
    return D == 1 && sizeof(R) == 4 && nw == 16 && !m.Ft && !m.gradient && m.proposal == AUXSSM_PROP_AUX_INDEPENDENT && m.potential == AUXSSM_POT_SV &&
           m.transition == AUXSSM_TRANS_LINEAR && a.As == nullptr && a.noise_mode != AUXSSM_NOISE_EXPLICIT && !a.pregen;
}

// The forward pass of (model, sweep), nw = nw_class(N).  TV: time-varying transitions; GRAD: gradient-informed proposals; P = FkBuiltin<R, D, V>, V the variant of
// the model's potential (csmc_sweep.h::with_pot).
//   case                            k_csmc_fwd<R, D, ...>                    ("own variant": a coupled, the Poisson or the logistic potential, V != SEP)
//   own variant, guided             <false, GRAD, 0, 2, P>
//   own variant, otherwise          <TV, GRAD, 0, 0, P>                      the generic workgroup for every N
//   guided, separable potentials    <false, GRAD, nw == 16 ? 16 : 0, 2, P>   N = 512 takes the generic one
//   c3_shape                        <float, 1, false, false, 16, 1>
//   everything else                 <TV, GRAD, nw, 0, P>
template <typename R, int D> static SweepKernel<R> fwd_kernel(const FkDev<R>& m, const CsmcArgs& a, int nw) {
    const bool tv = m.Ft != nullptr, guided = m.proposal == AUXSSM_PROP_AUX_GUIDED;
    return with_bool(m.gradient != 0, [&](auto gr) {
        return with_pot(m.potential, [&](auto pv) -> SweepKernel<R> {
            constexpr bool GR = decltype(gr)::value, SEP = decltype(pv)::value == PotV::SEP;
            using P = FkBuiltin<R, D, decltype(pv)::value>;
            if (guided) {
                if constexpr (SEP) {
                    if (nw == 16) return k_csmc_fwd<R, D, false, GR, 16, 2, P>;
                }
                return k_csmc_fwd<R, D, false, GR, 0, 2, P>;
            }
            if constexpr (D == 1 && sizeof(R) == 4 && !GR && SEP) {
                if (c3_shape<R, D>(m, a, nw)) return k_csmc_fwd<R, D, false, false, 16, 1>;
            }
            return with_bool(tv, [&](auto tvc) -> SweepKernel<R> {
                constexpr bool TV = decltype(tvc)::value;
                if constexpr (!SEP) return k_csmc_fwd<R, D, TV, GR, 0, 0, P>;
                else return with_nw(nw, [&](auto n) -> SweepKernel<R> { return k_csmc_fwd<R, D, TV, GR, decltype(n)::value, 0, P>; });
            });
        });
    });
}
// The backward pass: k_csmc_bwd<R, D, TV, nw>, whatever the proposal and the potential.
template <typename R, int D> static SweepKernel<R> bwd_kernel(const FkDev<R>& m, int nw) {
    return with_bool(m.Ft != nullptr, [&](auto tvc) {
        return with_nw(nw, [&](auto n) -> SweepKernel<R> { return k_csmc_bwd<R, D, decltype(tvc)::value, decltype(n)::value>; });
    });
}

template <typename R, int D>
static int run_csmc(auxssm_ctx* h, const auxssm_fk_model* fk, CsmcArgs& a, void* ctt) {
    FkDev<R> m = fk_dev<R>(fk);
    int rc = csmc_prologue<R>(h, fk, a, ctt, m, false, [&] { return builtin_grad<R, D>(h, a, m); });
    if (rc) return rc;
    const int TB = (a.N + 63) / 64 * 64, nw = nw_class(a.N);
    // forward + backward pass, batch of chains by batch (CsmcArgs::c0; one batch unless the particle systems of all chains do not fit the device)
    const int cb = a.cb > 0 ? a.cb : a.C;
    for (int c0 = 0; c0 < a.C; c0 += cb) {
        const CsmcArgs ab = csmc_batch(a, c0, cb);
        {
            ProfScope ps(h, AUXSSM_K_CSMC_FWD);
            if ((rc = launch(h, fwd_kernel<R, D>(m, ab, nw), dim3(ab.C), dim3(TB), fwd_lds(TB, D, sizeof(R)), ab, m))) return rc;
        }
        {
            ProfScope ps(h, AUXSSM_K_CSMC_BWD);
            if ((rc = launch(h, bwd_kernel<R, D>(m, nw), dim3(ab.C), dim3(TB), bwd_lds(TB, D, sizeof(R)), ab, m))) return rc;
        }
    }
    AX_HIP(hipGetLastError());
    return AUXSSM_OK;
}

// run_csmc with a user-defined model (fk_program.hip): the same launches, the forward / backward passes, the potential's bound and the gradient from the
// program's module.  Time-invariant transitions; gradient proposals with a gradient program only (auxssm_csmc_sweep_program refuses the rest).
static int fk_launch(auxssm_ctx* h, hipFunction_t f, unsigned grid, unsigned block, size_t lds, void** args) {
    if (lds > 48 * 1024) {  // (module functions have no hipFuncSetAttribute: their limit is what the device grants, checked here)
        int mx = 0;
        AX_HIP(hipFuncGetAttribute(&mx, HIP_FUNC_ATTRIBUTE_MAX_DYNAMIC_SHARED_SIZE_BYTES, f));
        if ((size_t)mx < lds) {
            set_error("the user-model sweep needs %zu bytes of LDS, the device grants %d", lds, mx);
            return AUXSSM_ERR_UNSUPPORTED;
        }
    }
    AX_HIP(hipModuleLaunchKernel(f, grid, 1, 1, block, 1, 1, (unsigned)lds, h->stream, args, nullptr));
    return AUXSSM_OK;
}
// The program's passes for nw = nw_class(N), by their index in the module (fk_program.h: three of each kind, NW = 0 / 8 / 16):
//   forward   FK_FWD0 + nw / 8, with gradient proposals FK_FWDG0 + nw / 8
//   backward  FK_BWD0 + nw / 8
static int fk_fwd_index(int gradient, int nw) { return (gradient ? FK_FWDG0 : FK_FWD0) + nw / 8; }
static int fk_bwd_index(int nw) { return FK_BWD0 + nw / 8; }
template <typename R, int D>
static int run_csmc_program(auxssm_ctx* h, const auxssm_fk_program_s* prog, const auxssm_fk_model* fk, const auxssm_fk_user* user, CsmcArgs& a) {
    const hipFunction_t* fn = nullptr;
    int rc = fk_program_functions(h, prog, &fn);
    if (rc) return rc;
    FkDev<R> m = fk_dev<R>(fk);
    FkUser<R> u{(const R*)user->y, (const R*)user->theta_g, (const R*)user->theta_m, user->p};
    const bool user_bound = (prog->flags & AUXSSM_FK_USER_POTENTIAL) != 0;
    if (a.gb && user_bound) {
        int T = a.T;
        R* gb = (R*)a.gb;
        void* args[] = {&T, &u, &gb};
        if ((rc = fk_launch(h, fn[FK_BOUND], (unsigned)((a.T + 255) / 256), 256, 0, args))) return rc;
    }
    rc = csmc_prologue<R>(h, fk, a, nullptr, m, user_bound, [&] {
        void* args[] = {&a, &m, &u};
        return fk_launch(h, fn[FK_GRAD], (unsigned)(((long long)a.C * a.T + 255) / 256), 256, 0, args);
    });
    if (rc) return rc;
    const int TB = (a.N + 63) / 64 * 64, nw = nw_class(a.N);
    const int cb = a.cb > 0 ? a.cb : a.C;
    for (int c0 = 0; c0 < a.C; c0 += cb) {
        CsmcArgs ab = csmc_batch(a, c0, cb);
        void* args[] = {&ab, &m, &u};
        {
            ProfScope ps(h, AUXSSM_K_CSMC_FWD);
            if ((rc = fk_launch(h, fn[fk_fwd_index(m.gradient, nw)], (unsigned)ab.C, (unsigned)TB, fwd_lds(TB, D, sizeof(R)), args))) return rc;
        }
        {
            ProfScope ps(h, AUXSSM_K_CSMC_BWD);
            if ((rc = fk_launch(h, fn[fk_bwd_index(nw)], (unsigned)ab.C, (unsigned)TB, bwd_lds(TB, D, sizeof(R)), args))) return rc;
        }
    }
    AX_HIP(hipGetLastError());
    return AUXSSM_OK;
}

}  // namespace ax

namespace ax {
int run_csmc_wide(auxssm_ctx* h, int dtype, const auxssm_fk_model* fk, CsmcArgs& a, void* ctt);  // csmc_wide.hip
int run_csmc_chain(auxssm_ctx* h, int dtype, const auxssm_fk_model* fk, const auxssm_fk_chain_dynamics* dyn, CsmcArgs& a, void* ctt);  // csmc_chain.hip
}
using namespace ax;

extern "C" int auxssm_normalize_resample(auxssm_handle h, int dtype, int32_t rows, int32_t N, const void* log_weights,
                                         const void* weights, const void* uniforms, void* weights_out, int32_t* indices) {
    AX_NEED_H(h);
    if (int rc = check_dtype(dtype)) return rc;
    if (rows < 1 || N < 1 || N > 1024) {
        set_error("need rows >= 1 and 1 <= N <= 1024");
        return AUXSSM_ERR_ARG;
    }
    if ((!log_weights) == (!weights)) {
        set_error("give exactly one of log_weights / weights");
        return AUXSSM_ERR_ARG;
    }
    if (indices && !uniforms) {
        set_error("indices need uniforms");
        return AUXSSM_ERR_ARG;
    }
    const int TB = (N + 63) / 64 * 64;
    if (dtype == AUXSSM_F32)
        hipLaunchKernelGGL((k_normalize_resample<float>), dim3(rows), dim3(TB), (size_t)TB * 4 + 48 * 4 + 64, h->stream, N,
                           (const float*)log_weights, (const float*)weights, (const float*)uniforms, (float*)weights_out, indices);
    else
        hipLaunchKernelGGL((k_normalize_resample<double>), dim3(rows), dim3(TB), (size_t)TB * 8 + 48 * 8 + 64, h->stream, N,
                           (const double*)log_weights, (const double*)weights, (const double*)uniforms, (double*)weights_out, indices);
    AX_HIP(hipGetLastError());
    return AUXSSM_OK;
}

extern "C" int auxssm_systematic_resample(auxssm_handle h, int dtype, int32_t rows, int32_t M, int32_t N, const void* weights, const void* uvw,
                                          int32_t* indices) {
    AX_NEED_H(h);
    if (int rc = check_dtype(dtype)) return rc;
    if (rows < 1 || M < 1 || M > 1024 || N < 1 || N > 1024) {
        set_error("need rows >= 1, 1 <= M <= 1024 weights and 1 <= N <= 1024 draws");
        return AUXSSM_ERR_ARG;
    }
    if (!weights || !uvw || !indices) {
        set_error("weights/uvw/indices must be non-NULL");
        return AUXSSM_ERR_ARG;
    }
    const int TB = ((M > N ? M : N) + 63) / 64 * 64;
    const size_t sR = dtype == AUXSSM_F32 ? 4 : 8;
    const size_t lds = (size_t)TB * sR + 48 * sR + (size_t)TB * 4 + 64;
    if (dtype == AUXSSM_F32)
        hipLaunchKernelGGL((k_systematic<float>), dim3(rows), dim3(TB), lds, h->stream, M, N, (const float*)weights, (const float*)uvw, indices);
    else
        hipLaunchKernelGGL((k_systematic<double>), dim3(rows), dim3(TB), lds, h->stream, M, N, (const double*)weights, (const double*)uvw, indices);
    AX_HIP(hipGetLastError());
    return AUXSSM_OK;
}

// auxssm_csmc_sweep (prog == nullptr), auxssm_csmc_sweep_program and auxssm_csmc_sweep_chain_dynamics (dyn != nullptr: per-chain transitions, csmc_chain.hip):
// one validation, one workspace plan, one chain batching
static int csmc_sweep_impl(auxssm_handle h, int dtype, const auxssm_fk_model* fk, const auxssm_fk_program_s* prog, const auxssm_fk_user* user,
                           const auxssm_fk_chain_dynamics* dyn, int32_t C,
                           int32_t T, int32_t N, int32_t backward, const void* sqrt_half_delta, void* x, const auxssm_csmc_noise* noise, int32_t* ancestors,
                           void* xs_out, void* log_ws_out, int32_t* As_out) {
    AX_NEED_H(h);
    if (int rc = check_dtype(dtype)) return rc;
    if (!fk || !x || !noise || !ancestors) {
        set_error("model/x/noise/ancestors must be non-NULL");
        return AUXSSM_ERR_ARG;
    }
    if (C < 1 || T < 1 || N < 2 || N > 1024) {
        set_error("need C >= 1, T >= 1, 2 <= N <= 1024 (got C=%d T=%d N=%d)", C, T, N);
        return AUXSSM_ERR_ARG;
    }
    const int D = fk->dx;
    const bool wide = D > CS_MAXD;  // csmc_wide.hip: one wave per chain, particles' components in LDS rows
    const bool ug = prog && (prog->flags & AUXSSM_FK_USER_POTENTIAL), um = prog && (prog->flags & AUXSSM_FK_USER_MEAN);
    if (dyn) {  // per-chain transitions: the register kernels' independent and bootstrap proposals on linear, time-invariant dynamics
        if (!dyn->F || !dyn->b || !dyn->chol_Q) {
            set_error("dyn->%s is NULL: per-chain dynamics need the device arrays F (C,dx,dx), b (C,dx) and chol_Q (C,dx,dx)", !dyn->F ? "F" : (!dyn->b ? "b" : "chol_Q"));
            return AUXSSM_ERR_ARG;
        }
        if (D > CS_MAXD) {
            set_error("dx=%d: per-chain dynamics run the register sweep kernels, dx <= %d (the wide-state kernels read one shared transition)", D, CS_MAXD);
            return AUXSSM_ERR_UNSUPPORTED;
        }
        if (fk->proposal == AUXSSM_PROP_AUX_GUIDED) {
            set_error("guided proposals run chain-shared transitions: with per-chain dynamics their K_t / chol Lambda_t tables would be per chain and step");
            return AUXSSM_ERR_UNSUPPORTED;
        }
        if (fk->transition != AUXSSM_TRANS_LINEAR) {
            set_error("per-chain dynamics are linear-Gaussian (F, b, chol_Q): AUXSSM_TRANS_LORENZ63_EM has none to replace");
            return AUXSSM_ERR_UNSUPPORTED;
        }
        if (fk->F_t || fk->b_t || fk->chol_Q_t) {
            set_error("per-chain dynamics are time-invariant: F_t / b_t / chol_Q_t must be NULL (one transition per chain, not per chain and step)");
            return AUXSSM_ERR_UNSUPPORTED;
        }
    }
    if (prog) {
        if (!user) {
            set_error("user must be non-NULL");
            return AUXSSM_ERR_ARG;
        }
        if (prog->dtype != dtype || prog->dx != D) {
            set_error("the program was compiled for dtype %d, dx %d (sweep: dtype %d, dx %d)", prog->dtype, prog->dx, dtype, D);
            return AUXSSM_ERR_ARG;
        }
        if (fk->F_t || fk->b_t || fk->chol_Q_t) {
            set_error("user-defined models run time-invariant transitions");
            return AUXSSM_ERR_UNSUPPORTED;
        }
        if (fk->gradient != AUXSSM_GRAD_NONE && !(prog->flags & AUXSSM_FK_USER_GRADIENT)) {
            set_error("gradient proposals need a program compiled with AUXSSM_FK_USER_GRADIENT (the derivatives of the user-defined parts)");
            return AUXSSM_ERR_UNSUPPORTED;
        }
        if (um && fk->transition != AUXSSM_TRANS_LINEAR) {
            set_error("a user transition mean replaces the linear one (transition must be AUXSSM_TRANS_LINEAR)");
            return AUXSSM_ERR_ARG;
        }
        if (user->y && user->p < 1) {
            set_error("user observations need p >= 1 columns");
            return AUXSSM_ERR_ARG;
        }
    }
    if (D < 1 || D > 32) {
        set_error("dx=%d: the cSMC kernels cover 1 <= dx <= 32", D);
        return AUXSSM_ERR_UNSUPPORTED;
    }
    if (wide && (N > 64 || fk->transition != AUXSSM_TRANS_LINEAR)) {
        set_error("dx=%d runs the wide-state cSMC kernels: N <= 64 particles, linear-Gaussian transitions", D);
        return AUXSSM_ERR_UNSUPPORTED;
    }
    if (fk->proposal != AUXSSM_PROP_BOOTSTRAP_LG && fk->proposal != AUXSSM_PROP_AUX_INDEPENDENT && fk->proposal != AUXSSM_PROP_AUX_GUIDED) {
        set_error("unknown proposal kind %d", fk->proposal);
        return AUXSSM_ERR_ARG;
    }
    const bool guided = fk->proposal == AUXSSM_PROP_AUX_GUIDED, auxiliary = guided || fk->proposal == AUXSSM_PROP_AUX_INDEPENDENT;
    if (guided && prog) {
        set_error("guided proposals run the closed model family: they are not compiled into user-defined programs");
        return AUXSSM_ERR_UNSUPPORTED;
    }
    if (guided && (fk->F_t || fk->b_t || fk->chol_Q_t)) {
        set_error("guided proposals run time-invariant transitions");
        return AUXSSM_ERR_UNSUPPORTED;
    }
    if (int rc = check_fk_model(fk, noise, ug)) return rc;
    if (auxiliary && !sqrt_half_delta) {
        set_error("the auxiliary proposals need sqrt_half_delta (T)");
        return AUXSSM_ERR_ARG;
    }
    if (fk->gradient != AUXSSM_GRAD_NONE && !auxiliary) {
        set_error("gradient-informed proposals belong to AUXSSM_PROP_AUX_INDEPENDENT and AUXSSM_PROP_AUX_GUIDED");
        return AUXSSM_ERR_ARG;
    }
    if (guided && fk->gradient != AUXSSM_GRAD_NONE && fk->gradient != AUXSSM_GRAD_REFERENCE) {
        set_error("guided proposals take AUXSSM_GRAD_NONE or AUXSSM_GRAD_REFERENCE (the potential's gradient at u shifts the proposal mean; there is no other weighting)");
        return AUXSSM_ERR_ARG;
    }
    if (noise->mode == AUXSSM_NOISE_EXPLICIT && (!noise->eps_prop || !noise->u_bwd || (T > 1 && !noise->u_res) || (auxiliary && !noise->eps_aux))) {
        set_error("explicit noise needs eps_prop, u_res, u_bwd (and eps_aux for the auxiliary proposals)");
        return AUXSSM_ERR_ARG;
    }
    const size_t sR = dtype == AUXSSM_F32 ? 4 : 8;
    const size_t CT = (size_t)C * T;
    // the particle systems (xs, lws, As) dominate: T N (D + 1) reals per chain.  When those of all C chains do not fit what the device has free
    // (counting the handle's current workspace, which a larger reservation replaces), the sweep runs in batches of cb chains (CsmcArgs::c0)
    const size_t xs_rec = xs_out ? 0 : (size_t)T * N * D * sR, lws_rec = log_ws_out ? 0 : (size_t)T * N * sR;
    const size_t As_rec = (!backward && !As_out) ? (size_t)(T > 1 ? T - 1 : 1) * N * 4 : 0;
    const size_t big = xs_rec + lws_rec + As_rec;
    int cb = C;
    if (big) {
        const size_t small = 4096 + 8 * 256 + (size_t)C * N * sR + CT * sR + (size_t)T * (2 + D) * sR + 2 * CT * D * sR;
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) == hipSuccess) {
            const double budget = 0.8 * (double)(fr + h->ws_bytes);  // (ws_reserve adds an eighth)
            if ((double)small + (double)C * (double)big > budget) {
                const double fit = (budget - (double)small) / (double)big;
                if (fit < 1.0) {
                    set_error("one chain's particle system (%zu bytes) does not fit the device (%zu free)", big, fr + h->ws_bytes);
                    return AUXSSM_ERR_NOMEM;
                }
                if (fit < (double)cb) cb = (int)fit;
                if (cb > h->num_cu) cb -= cb % h->num_cu;  // one workgroup per chain and CU: whole rounds of the chip per batch
            }
        }
        if (const char* ev = getenv("AUXSSM_CSMC_BATCH")) {  // test hook: tests/test_gpu_csmc.py and tests/test_gpu_full_size.py force small batches
            const int v = atoi(ev);
            if (v >= 1 && v < cb) cb = v;
        }
    }
    const size_t CBT = (size_t)cb * T, T1 = (size_t)(T > 1 ? T - 1 : 1);
    CsmcArgs a{};
    a.C = C; a.T = T; a.N = N; a.backward = backward ? 1 : 0;
    a.y = fk->y;
    a.shd = sqrt_half_delta;
    a.x = x;
    a.cb = cb; a.xs_rec = xs_rec; a.lws_rec = lws_rec; a.As_rec = As_rec;
    a.xs = xs_out; a.lws = log_ws_out; a.As = As_out;
    a.anc = ancestors;
    a.noise_mode = noise->mode;
    a.key0 = noise->key0; a.key1 = noise->key1;
    a.eps_aux = noise->eps_aux; a.eps_prop = noise->eps_prop; a.u_res = noise->u_res; a.u_bwd = noise->u_bwd;
    // the workspace plan: the buffers this sweep owns
    WsPlan ws;
    void *ctt = nullptr, *ub = nullptr, *pe = nullptr, *pu = nullptr;
    ws.add(a.u, CT * D * sR);
    if (fk->gradient) ws.add(a.grad, CT * D * sR);
    if (fk->F_t) ws.add(ctt, (size_t)T * (1 + D) * sR);  // constants + reciprocal diagonals of the T - 1 transitions
    if (dyn) ws.add(ctt, (size_t)C * (1 + D) * sR);      // ... of the C per-chain transitions
    if (!xs_out) ws.add(a.xs, CBT * N * D * sR);
    if (!log_ws_out) ws.add(a.lws, CBT * N * sR);
    if (!As_out && !backward) ws.add(a.As, (size_t)cb * T1 * N * 4);
    ws.add(a.wT, (size_t)C * N * sR);
    ws.add(a.fmax, CT * sR);
    // (the guided weights are not bounded by gb + c_trans: no bound array, every step shifts by its exact maximum)
    // (nor do the wide kernels shift the multivariate-t potential's weights by its bound sup_x log g = 0: at dx > 4 the weights sit tens of nats below it -- (nu + dx) / 2
    // times a logarithm -- and fp32 weights exp(lw - bound) leave the normal range, which costs the resampling draws their precision long before every weight is zero)
    // (the linear-Gaussian observation potential likewise: its bound c_lin is attained only where Hw x = yw_t, and at dx > 4 the particles' residuals leave the weights
    // as far below it)
    const bool loose = wide && !ug && pot_kind(fk->potential).wide_no_bound;
    if (!guided && !loose && (ug ? prog->has_bound : (fk->potential == AUXSSM_POT_FLAT || fk->y != nullptr))) ws.add(a.gb, (size_t)T * sR);
    if (guided) ws.add(a.gtab, guided_tab_reals(T, D) * sR);  // K_t, chol Lambda_t and their constants, every step
    if (noise->mode == AUXSSM_NOISE_THREEFRY) ws.add(ub, CT * sR);  // the backward pass's uniforms, drawn once (csmc_sweep.h::k_csmc_ubwd)
    // fewer chains than CUs: the forward pass's draws are generated up front by the whole chip (csmc_sweep.h::k_csmc_pregen) when the two arrays fit
    bool pregen = noise->mode == AUXSSM_NOISE_THREEFRY && !wide && T > 1 && C < h->num_cu && cb == C &&
                  !getenv("AUXSSM_CSMC_NO_PREGEN");  // test hook: tests/test_gpu_csmc.py and tests/test_gpu_full_size.py force the in-pass draws
    if (pregen) {
        ws.add(pe, CT * N * D * sR);
        ws.add(pu, (size_t)C * T1 * N * sR);
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) != hipSuccess || (double)ws.total() > 0.7 * (double)(fr + h->ws_bytes)) {
            ws.drop(2);
            pregen = false;
        }
    }
    if (int rc = ws.reserve(h)) return rc;
    if (ub) {
        const long long n = (long long)CT;
        if (dtype == AUXSSM_F32) hipLaunchKernelGGL((k_csmc_ubwd<float>), dim3((unsigned)(((n + 1) / 2 + 255) / 256)), dim3(256), 0, h->stream, n, noise->key0, noise->key1, (float*)ub);
        else hipLaunchKernelGGL((k_csmc_ubwd<double>), dim3((unsigned)(((n + 1) / 2 + 255) / 256)), dim3(256), 0, h->stream, n, noise->key0, noise->key1, (double*)ub);
        a.u_bwd = ub;
    }
    if (pregen) {
        const int T2 = (T + 1) >> 1;
        const dim3 grid((unsigned)C * T2, (unsigned)((N * D + 255) / 256));
        ProfScope ps(h, AUXSSM_K_RNG);
        if (dtype == AUXSSM_F32) hipLaunchKernelGGL((k_csmc_pregen<float>), grid, dim3(256), 0, h->stream, T, N, D, noise->key0, noise->key1, (float*)pe, (float*)pu);
        else hipLaunchKernelGGL((k_csmc_pregen<double>), grid, dim3(256), 0, h->stream, T, N, D, noise->key0, noise->key1, (double*)pe, (double*)pu);
        a.pregen = 1;
        a.eps_prop = pe;
        a.u_res = pu;
    }
    if (dyn) return run_csmc_chain(h, dtype, fk, dyn, a, ctt);
    if (wide) return run_csmc_wide(h, dtype, fk, a, ctt);
    return csmc_dispatch(dtype, D, [&](auto r, auto d) {
        using R = decltype(r);
        constexpr int DD = decltype(d)::value;
        return prog ? run_csmc_program<R, DD>(h, prog, fk, user, a) : run_csmc<R, DD>(h, fk, a, ctt);
    });
}

extern "C" int auxssm_csmc_sweep(auxssm_handle h, int dtype, const auxssm_fk_model* fk, int32_t C, int32_t T, int32_t N,
                                 int32_t backward, const void* sqrt_half_delta, void* x, const auxssm_csmc_noise* noise,
                                 int32_t* ancestors, void* xs_out, void* log_ws_out, int32_t* As_out) {
    return csmc_sweep_impl(h, dtype, fk, nullptr, nullptr, nullptr, C, T, N, backward, sqrt_half_delta, x, noise, ancestors, xs_out, log_ws_out, As_out);
}

extern "C" int auxssm_csmc_sweep_program(auxssm_handle h, auxssm_fk_program prog, int dtype, const auxssm_fk_model* fk, const auxssm_fk_user* user,
                                         int32_t C, int32_t T, int32_t N, int32_t backward, const void* sqrt_half_delta, void* x,
                                         const auxssm_csmc_noise* noise, int32_t* ancestors, void* xs_out, void* log_ws_out, int32_t* As_out) {
    if (!prog) {
        set_error("program is NULL");
        return AUXSSM_ERR_ARG;
    }
    return csmc_sweep_impl(h, dtype, fk, prog, user, nullptr, C, T, N, backward, sqrt_half_delta, x, noise, ancestors, xs_out, log_ws_out, As_out);
}

extern "C" int auxssm_csmc_sweep_chain_dynamics(auxssm_handle h, int dtype, const auxssm_fk_model* fk, const auxssm_fk_chain_dynamics* dyn, int32_t C, int32_t T,
                                                int32_t N, int32_t backward, const void* sqrt_half_delta, void* x, const auxssm_csmc_noise* noise,
                                                int32_t* ancestors, void* xs_out, void* log_ws_out, int32_t* As_out) {
    if (!dyn) {
        set_error("dyn is NULL (the chain-shared sweep is auxssm_csmc_sweep)");
        return AUXSSM_ERR_ARG;
    }
    return csmc_sweep_impl(h, dtype, fk, nullptr, nullptr, dyn, C, T, N, backward, sqrt_half_delta, x, noise, ancestors, xs_out, log_ws_out, As_out);
}
