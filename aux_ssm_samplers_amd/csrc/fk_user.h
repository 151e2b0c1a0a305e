// fk_user.h -- the user-model policy of the sequential cSMC sweep.  Never compiled by hipcc: fk_program.hip hands hipRTC a program
//     #include "fk_user_pre.h"   <- the model contract (what user code may call, fallback declarations for detection)
//     <the user's source>
//     #include "fk_user.h"       <- this file: detection, the policy, the kernels to instantiate
// with -O3 -std=c++17 -ffp-contract=off for gfx950 (the flags of csmc.o) and AXFK_USER_G / AXFK_USER_M set to 0 / 1 by the caller: which of the
// potential and the transition mean the user's source supplies (the other one is the built-in closed family, read from FkDev as in csmc.hip).
// The derivatives of the user's parts (grad_log_g, mean_vjp) are only called by k_csmc_grad, which only a gradient program instantiates.
#pragma once

namespace ax {

template <typename A, typename B> struct fk_same { static constexpr bool value = false; };
template <typename A> struct fk_same<A, A> { static constexpr bool value = true; };
template <typename T> using fk_void = void;

// presence and signature of the user's functions (fk_user_pre.h declares fallbacks of another signature, so a missing name is not an error here)
template <typename R, int D, typename = void> struct fk_has_log_g { static constexpr bool value = false; };
template <typename R, int D>
struct fk_has_log_g<R, D, fk_void<decltype(::log_g<R, D>(0, (const R*)nullptr, (const R*)nullptr, (const R*)nullptr, (const R*)nullptr))>> {
    static constexpr bool value = fk_same<decltype(::log_g<R, D>(0, (const R*)nullptr, (const R*)nullptr, (const R*)nullptr, (const R*)nullptr)), R>::value;
};
template <typename R, int D, typename = void> struct fk_has_bound { static constexpr bool value = false; };
template <typename R, int D> struct fk_has_bound<R, D, fk_void<decltype(::log_g_bound<R, D>(0, (const R*)nullptr, (const R*)nullptr))>> {
    static constexpr bool value = fk_same<decltype(::log_g_bound<R, D>(0, (const R*)nullptr, (const R*)nullptr)), R>::value;
};
template <typename R, int D, typename = void> struct fk_has_mean { static constexpr bool value = false; };
template <typename R, int D> struct fk_has_mean<R, D, fk_void<decltype(::mean<R, D>(0, (const R*)nullptr, (const R*)nullptr, (R*)nullptr))>> {
    static constexpr bool value = true;
};

template <typename R, int D, typename = void> struct fk_has_grad_log_g { static constexpr bool value = false; };
template <typename R, int D>
struct fk_has_grad_log_g<R, D, fk_void<decltype(::grad_log_g<R, D>(0, (const R*)nullptr, (const R*)nullptr, (const R*)nullptr, (const R*)nullptr, (R*)nullptr, (R*)nullptr))>> {
    static constexpr bool value =
        fk_same<decltype(::grad_log_g<R, D>(0, (const R*)nullptr, (const R*)nullptr, (const R*)nullptr, (const R*)nullptr, (R*)nullptr, (R*)nullptr)), void>::value;
};
template <typename R, int D, typename = void> struct fk_has_mean_vjp { static constexpr bool value = false; };
template <typename R, int D>
struct fk_has_mean_vjp<R, D, fk_void<decltype(::mean_vjp<R, D>(0, (const R*)nullptr, (const R*)nullptr, (const R*)nullptr, (R*)nullptr))>> {
    static constexpr bool value = fk_same<decltype(::mean_vjp<R, D>(0, (const R*)nullptr, (const R*)nullptr, (const R*)nullptr, (R*)nullptr)), void>::value;
};

template <typename R, int D, bool UG, bool UM> struct FkUserPolicy {
    static_assert(!UG || fk_has_log_g<R, D>::value,
                  "the model source must define  template <typename R, int D> __device__ R log_g(int t, const R* x, const R* xprev, const R* y, const R* theta)");
    static_assert(!UM || fk_has_mean<R, D>::value,
                  "the dynamics source must define  template <typename R, int D> __device__ void mean(int t, const R* xprev, const R* theta, R* mu)");
    FkUser<R> u;
    // a program that keeps the built-in potential may meet the logistic one, whose sizes are plane 1 of CsmcArgs::y: a run-time question here (size_row_rt)
    static constexpr bool size_row = !UG;
    __device__ __forceinline__ void load_sizes(const FkDev<R>& m, const R* y, long long T, long long t, R* sz) const { size_row_rt<R, D>(m, y, T, t, sz); }
    __device__ __forceinline__ R log_g(const FkDev<R>& m, int t, const R* x, const R* xprev, const R* y, const R* sz = nullptr) const {
        if constexpr (UG) return ::log_g<R, D>(t, x, xprev, u.y ? u.y + (long long)t * u.p : nullptr, u.theta_g);
        else return potential_rt<R, D>(m, x, y, sz);
    }
    __device__ __forceinline__ void mean(const FkDev<R>& m, const TransT<R>& tr, int t, const R* xp, R* mu) const {
        if constexpr (UM) ::mean<R, D>(t, xp, u.theta_m, mu);
        else trans_mean_t<R, D>(m, tr, xp, mu);
    }
    // the derivatives (k_csmc_grad).  A user part without its derivative compiles to nothing here: fk_program.hip refuses such a gradient program
    // before any launch (k_fk_probe below)
    static constexpr bool grad_xprev = UG;
    __device__ __forceinline__ void grad_log_g(const FkDev<R>& m, int t, const R* x, const R* xprev, const R* y, R* gx, R* gxprev, const R* sz = nullptr) const {
        if constexpr (UG) {
            if constexpr (fk_has_grad_log_g<R, D>::value) ::grad_log_g<R, D>(t, x, xprev, u.y ? u.y + (long long)t * u.p : nullptr, u.theta_g, gx, gxprev);
        } else {
            potential_grad_rt<R, D>(m, x, y, gx, sz);
        }
    }
    __device__ __forceinline__ void mean_vjp(const FkDev<R>& m, const TransT<R>& tr, int t, const R* xp, const R* v, R* out) const {
        if constexpr (UM) {
            if constexpr (fk_has_mean_vjp<R, D>::value) ::mean_vjp<R, D>(t, xp, u.theta_m, v, out);
        } else {
            trans_mean_vjp_t<R, D>(m, tr, xp, v, out);
        }
    }
};

// presence probes of a gradient program: the host names k_fk_probe<R, D, W, fk_has_...<R, D>::value> and k_fk_probe<R, D, W, true> (W = 0: grad_log_g,
// 1: mean_vjp) and compares their lowered names, as for k_fk_bound below.  Never launched.
template <typename R, int D, int W, bool HAS> __global__ void k_fk_probe() {}

// gb[t] = sup_x log G_t(x) from the user's log_g_bound (the forward shift of the sweep contract, as k_csmc_potbound for the built-ins).  The host
// names both k_fk_bound<R, D, fk_has_bound<R, D>::value> and k_fk_bound<R, D, true>: the two are the same kernel exactly when the source defines
// log_g_bound (fk_program.hip compares their lowered names).  Without a bound the launcher passes gb = nullptr and runs neither; the body is empty then.
template <typename R, int D, bool HAS> __global__ void k_fk_bound(int T, FkUser<R> u, R* __restrict__ gb) {
    if constexpr (HAS && fk_has_bound<R, D>::value) {
        const int t = blockIdx.x * blockDim.x + threadIdx.x;
        if (t >= T) return;
        gb[t] = ::log_g_bound<R, D>(t, u.y ? u.y + (long long)t * u.p : nullptr, u.theta_g);
    }
}

}  // namespace ax
