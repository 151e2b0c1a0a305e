// pit_shared.h -- what the two units of the parallel-in-time cSMC sweep share (pit.hip: the register kernels of dx <= 4, the entry point and the trace;
// pit_wide.hip: the kernels of 4 < dx <= 32): the sweep's arguments, its noise accessors, the per-time-step normalisation of the leaf weights and the constants
// of the arithmetic contract (header of pit.hip).  Units including this are compiled with -ffp-contract=off.
#pragma once
#include "csmc_host.h"

namespace ax {

struct PitArgs {
    int C, T, N, K;
    const void* y;    // (T, D) or null
    const void* shd;  // (T)
    void* x;          // (C, T, D) reference trajectory in, new trajectory out
    void* xs;         // (C, T, N, D) leaf particles
    void* lw0;        // (C, N) normalised log-weights of the leaf at t = 0
    // gradient-informed proposals (csmc/independent.py:81-84: mt = N(u + delta/2 grad, delta/2 I), qt = N(u, delta/2 I); pit/csmc.py:83-88: the leaf
    // weights are qt.logpdf - mt.logpdf, per particle): u, grad (C, T, D) and the normalised leaf log-weights of EVERY time step, lwt (C, T, N); null otherwise
    const void* u;
    const void* grad;
    void* lwt;
    uint16_t* Ls;     // (C, tot, N) left slot of each stitched pair, nodes of all levels back to back (off[k] = first node of level k)
    uint16_t* Rs;     // (C, tot, N) right slot
    uint16_t* Fi;     // (C, tot, N) leaf particle index at the node's first time step
    uint16_t* La;     // (C, tot, N) leaf particle index at the node's last time step
    int32_t* anc;     // (C, T)
    long long tot;
    long long off[32];
    double neg_log_n;
    int noise_mode;
    uint32_t key0, key1;
    const void* eps_aux;   // (C, T, D)
    const void* eps_prop;  // (C, T, N, D)
    const void* u_res;     // (C, T, N): row t feeds the stitch at the boundary (t-1 | t); row 0 is never read
};

template <typename R> __device__ __forceinline__ R pit_normal(const PitArgs& a, const void* arr, uint32_t stream, long long idx) {
    if (a.noise_mode == 0) return ((const R*)arr)[idx];
    return stream_normal<R>(a.key0, a.key1, stream, (unsigned long long)idx);
}
template <typename R> __device__ __forceinline__ R pit_uniform(const PitArgs& a, const void* arr, uint32_t stream, long long idx) {
    if (a.noise_mode == 0) return ((const R*)arr)[idx];
    return stream_uniform<R>(a.key0, a.key1, stream, (unsigned long long)idx);
}

// log(w / sum w) of a block's log-weights, the reductions of block_normalize
template <typename R> __device__ __forceinline__ R block_lognormalize(R lw, R* red, int tid, int nw) {
    const int lane = tid & 63, wv = tid >> 6;
    R m = wave_max(lw);
    if (lane == 0) red[wv] = m;
    __syncthreads();
    R t[16];
    load16<R>(red, t);
    m = t[0];
#pragma unroll
    for (int k = 1; k < 16; ++k) m = (k < nw && t[k] > m) ? t[k] : m;
    if (!(m - m == 0)) m = 0;
    const R e = det_exp(lw - m);
    R s = wave_sum_tree(e);
    if (lane == 0) red[16 + wv] = s;
    __syncthreads();
    load16<R>(red + 16, t);
    s = t[0];
#pragma unroll
    for (int k = 1; k < 16; ++k) s = k < nw ? s + t[k] : s;
    return lw - (det_log(s) + m);
}

constexpr int PIT_MAXD = 32, PIT_WIDE_MAXN = 64;  // the widest state of the sweep; the most particles of a wide one (dx > CS_MAXD: pit_wide.hip)
constexpr int PIT_SC = 8;  // sub-chunks per chunk (arithmetic contract, see the header of pit.hip)
// chunks of a stitch = lanes of its workgroup (arithmetic contract)
inline int pit_nch(int N) { return N <= 32 ? 64 : (N <= 128 ? 256 : 1024); }

// the leaves and the up-sweep of a wide model (4 < dx <= 32, N <= 64: pit_wide.hip); auxssm_csmc_pit_sweep (pit.hip) reads the trajectory off the tree afterwards
int run_pit_wide(auxssm_ctx* h, int dtype, const auxssm_fk_model* fk, PitArgs& a, void* ctt);

}  // namespace ax
