// pit_wide.hip -- the parallel-in-time conditional-SMC sweep for WIDE states with FEW particles: 4 < dx <= 32, N <= 64 (the reference's stochastic-volatility
// experiment defaults to --parallel --D 30 --N 25: examples/stochastic_volatility/experiment.py:20-22, :40, :55).
//
// Same tree, same arithmetic contract (header of pit.hip) and the same oracle (oracle/csmc_ref.c::csmc_ref_pit_sweep, MAXD = 32) as the register kernels of pit.hip;
// what changes is where the model and a particle live.  The model travels as FkW<R> -- pointers into the device block csmc_wide.hip caches on the handle
// (cw_model) -- and is staged into LDS by every workgroup; particles sit in zero-padded LDS rows.
//   leaves   one workgroup per (t, chain): the N dx draws elementwise (natural flat indices of streams 1 and 2, as k_pit_leaves has them), then -- at t = 0, and at
//            every t with gradient proposals -- the weights in the half-wave form of csmc_wide.hip (a particle's components across the 32 lanes of a half-wave:
//            potential_half, gauss_half, grad_corr_half), normalised by block_lognormalize with one lane per particle.
//   stitch   one workgroup per tree node, lanes = chunks as in k_pit_stitch, whose index bookkeeping (Ls, Rs, Fi, La, passthrough resolution, root draw) is
//            carried over line for line.  The N transition means and the N potentials are formed in the half-wave form; the N^2 densities are evaluated one pair
//            per lane by a forward substitution unrolled to 32 rows, rows beyond dx skipped: the row-oriented order of csmc_sweep.h::gauss_chol_logpdf itself.
//   trace    pit.hip::k_pit_trace (run-time dx).
// Linear-Gaussian transitions (time-invariant, or time-varying: a stitch stages row mid - 1), the eight built-in potentials, gradient proposals (the per-particle
// correction in either AUXSSM_GRAD_* mode, as for dx <= 4), fp32 and fp64, explicit and Threefry noise.
#include "csmc_wide_shared.h"
#include "pit_shared.h"

namespace ax {

constexpr int PW_S = CSW_MAXD + 1;  // stride of a particle row and of the matrices a half-wave reads by rows (odd: lanes of a half-wave fall into 32 banks)
constexpr int PW_LS = CSW_MAXD;     // stride of chol Q as the per-lane substitution reads it (every lane the same address: rows aligned for wide reads)
constexpr int PW_MAXN = 64;

// ---- leaves ---------------------------------------------------------------------------------------------------------------------------------------
constexpr int PWL_NT = 512;  // eight waves: sixteen particles per pass of the weight section
template <typename R> struct PwLeafLds {
    R *xr, *lw, *red, *uu, *pm, *xref, *pot_mat;
    __device__ PwLeafLds(char* smem, int D) {
        xr = (R*)smem;                // [64][S] the particles, rows zero-padded
        lw = xr + PW_MAXN * PW_S;     // [64]
        red = lw + PW_MAXN;           // [48]
        uu = red + 48;                // [32] u_t
        pm = uu + CSW_MAXD;           // [32] the proposal mean
        xref = pm + CSW_MAXD;         // [32] the reference trajectory's x_t
        pot_mat = xref + CSW_MAXD;    // [D][S] coupled potentials, t = 0 only
    }
    static constexpr size_t bytes(int D, bool coupled) {
        return ((size_t)PW_MAXN * PW_S + PW_MAXN + 48 + 3 * CSW_MAXD + (coupled ? (size_t)D * PW_S : 0)) * sizeof(R) + 16;
    }
};

// u = x + s eps_aux (or the prologue's, with gradient proposals); particles ~ N(u_t [+ s_t^2 grad_t], s_t^2 I), slot 0 = x; weights as k_pit_leaves has them
template <typename R, PotV V> __global__ void __launch_bounds__(PWL_NT) k_pitw_leaves(PitArgs a, FkW<R> m) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int t = blockIdx.x, c = blockIdx.y, tid = threadIdx.x, N = a.N, T = a.T, D = m.D;
    constexpr bool coupled = pot_has_matrix(V);
    PwLeafLds<R> L(smem, D);
    const bool grad = a.lwt != nullptr;
    const long long ct = (long long)c * T + t;
    const R sh = ((const R*)a.shd)[t];
    if (tid < CSW_MAXD) {
        R xk = 0, uk = 0, pk = 0;
        if (tid < D) {
            xk = ((const R*)a.x)[ct * D + tid];
            if (grad) {
                uk = ((const R*)a.u)[ct * D + tid];
                pk = fma_(sh * sh, ((const R*)a.grad)[ct * D + tid], uk);
            } else {
                uk = fma_(sh, pit_normal<R>(a, a.eps_aux, STREAM_EPS_AUX, ct * D + tid), xk);
                pk = uk;
            }
        }
        L.xref[tid] = xk, L.uu[tid] = uk, L.pm[tid] = pk;
    }
    for (int i = tid; i < PW_MAXN * PW_S; i += PWL_NT) L.xr[i] = 0;
    if constexpr (coupled) {
        if (t == 0)
            for (int i = tid; i < D * PW_S; i += PWL_NT) {
                const int r = i / PW_S, q = i - r * PW_S;
                L.pot_mat[i] = q < D ? m.pot_mat[r * D + q] : (R)0;
            }
    }
    __syncthreads();
    const int ND = N * D;
    for (int e = tid; e < ND; e += PWL_NT) {
        const int n = e / D, k = e - n * D;
        const R eps = pit_normal<R>(a, a.eps_prop, STREAM_EPS_PROP, ct * ND + e);
        const R xv = n == 0 ? L.xref[k] : fma_(sh, eps, L.pm[k]);
        ((R*)a.xs)[ct * ND + e] = xv;
        L.xr[n * PW_S + k] = xv;
    }
    if (!grad && t != 0) return;  // (uniform per workgroup)
    __syncthreads();
    const int lane = tid & 63, wv = tid >> 6, k = lane & 31, kk = k < D ? k : 0;
    const bool hi = lane >= 32;
    constexpr int PP = PWL_NT / 32;  // particles per pass
    const R uk = L.uu[k], pmk = L.pm[k];
    const R* Mrow = coupled ? L.pot_mat + kk * PW_S : nullptr;
    for (int s = 0; s * PP < N; ++s) {
        const int i = s * PP + 2 * wv + (hi ? 1 : 0);
        const bool pl = i < N;  // (uniform per half-wave)
        const R xk = L.xr[(pl ? i : 0) * PW_S + k];
        R g = 0;
        if (grad) g = grad_corr_half<R>(D, k, xk, uk, pmk, sh);  // qt.logpdf(x) - mt.logpdf(x) (pit/csmc.py:84-85), slot 0 included
        if (t == 0) {
            const R yk = (a.y && k < D) ? ((const R*)a.y)[k] : (R)0;
            R g0;
            if constexpr (V == PotV::LOGI) g0 = logistic_half<R>(D, k, xk, yk, a.y, T, 0);
            else g0 = potential_half<R, V>(m, k, hi, xk, yk, Mrow);
            g0 = g0 + gauss_half<R>(D, k, hi, k < D ? xk - m.m0[k] : (R)0, m.LP0 + (long long)kk * D, k < D ? m.iLP0[k] : (R)0, m.c_init);  // AuxiliaryG0
            g = grad ? g + g0 : g0;  // log_wts.at[0].add(log_w0) (pit/csmc.py:90-91)
        }
        if (pl && k == 0) L.lw[i] = g;
    }
    __syncthreads();
    const bool live = tid < N;
    const R lw = block_lognormalize<R>(live ? L.lw[tid] : (R)-INFINITY, L.red, tid, 1);  // (N <= 64: the particles are wave 0's)
    if (live) {
        if (grad) ((R*)a.lwt)[ct * N + tid] = lw;
        else ((R*)a.lw0)[(long long)c * N + tid] = lw;
    }
}

// ---- stitch ---------------------------------------------------------------------------------------------------------------------------------------
template <typename R> struct PwStitchLds {
    R *F, *LQ, *b, *iL, *xb, *mu, *tmp, *pg, *hh, *cs, *red, *sub, *pot_mat;
    __device__ PwStitchLds(char* smem, int D, int N, int NCH) {
        LQ = (R*)smem;                 // [32][LS] chol Q, zero-padded (first: 16-byte aligned rows)
        F = LQ + CSW_MAXD * PW_LS;     // [D][S] rows zero-padded to 32 columns
        b = F + D * PW_S;              // [32]
        iL = b + CSW_MAXD;             // [32] reciprocal diagonal of chol Q
        xb = iL + CSW_MAXD;            // [N][S] first-step particles of the right block
        mu = xb + N * PW_S;            // [N][S] transition means of the last-step particles of the left block
        tmp = mu + N * PW_S;           // [NCH / 32][S] a half-wave's left particle while its mean is formed
        pg = tmp + (NCH / 32) * PW_S;  // [N] potential + lw_b
        hh = pg + N;                   // [N] lw_a
        cs = hh + N;                   // [NCH] cumsum of the chunk sums
        red = cs + NCH;                // [48]
        sub = red + 48;                // [PIT_SC][NCH] sub-chunk sums
        pot_mat = sub + PIT_SC * NCH;  // [D][S] coupled potentials only
    }
    static constexpr size_t bytes(int D, int N, int NCH, bool coupled) {
        return ((size_t)CSW_MAXD * PW_LS + (size_t)D * PW_S + 2 * CSW_MAXD + (size_t)2 * N * PW_S + (size_t)(NCH / 32) * PW_S + 2 * N + NCH + 48 +
                (size_t)PIT_SC * NCH + (coupled ? (size_t)D * PW_S : 0)) * sizeof(R) + 16;
    }
};
static_assert(PwStitchLds<double>::bytes(CSW_MAXD, PW_MAXN, 256, true) <= 160 * 1024, "the stitch's LDS plan must fit the 160 KB of LDS of a CU");

// log N(x; mu, L L^T) of one pair in one lane: csmc_sweep.h::gauss_chol_logpdf with a run-time dimension -- the 32 rows unrolled, rows beyond D skipped
// (uniform), so z stays in registers.  x, mu: LDS rows; L: stride PW_LS, the same address in every lane
template <typename R> __device__ __forceinline__ R gauss_lane(int D, const R* x, const R* mu, const R* L, const R* iL, R cst) {
    R z[CSW_MAXD];
    R q = 0;
#pragma unroll
    for (int k = 0; k < CSW_MAXD; ++k) {
        if (k < D) {
            R acc = x[k] - mu[k];
#pragma unroll
            for (int j = 0; j < k; ++j) acc = fma_(-L[k * PW_LS + j], z[j], acc);
            z[k] = acc * iL[k];
            q = fma_(z[k], z[k], q);
        }
    }
    return fma_((R)-0.5, q, cst);
}

// the stitch of node j at level k (header of pit.hip); grid (nodes of the level, chains), NCH lanes
template <typename R, PotV V> __global__ void __launch_bounds__(256) k_pitw_stitch(PitArgs a, FkW<R> m, int k) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int j = blockIdx.x, c = blockIdx.y, tid = threadIdx.x, N = a.N, T = a.T, D = m.D;
    const long long s0 = (long long)j << (k + 1), mid = s0 + (1ll << k);
    if (mid >= T) return;  // passthrough node (uniform per workgroup)
    constexpr bool coupled = pot_has_matrix(V);
    const int NCH = blockDim.x, nw = NCH >> 6;
    PwStitchLds<R> L(smem, D, N, NCH);
    R *cs = L.cs, *red = L.red, *sub = L.sub, *pg = L.pg, *hh = L.hh;
    const bool root = k == a.K - 1;
    const long long chain_nodes = (long long)c * a.tot;
    // children: left = (k-1, 2j), complete; right = (k-1, 2j+1), resolved through passthrough nodes down to a stitched node or a leaf
    int kb = k - 1;
    long long jb = 2ll * j + 1;
    while (kb >= 0 && (jb << (kb + 1)) + (1ll << kb) >= T) {
        jb <<= 1;
        --kb;
    }
    const uint16_t* la_left = k > 0 ? a.La + (chain_nodes + a.off[k - 1] + 2ll * j) * N : nullptr;
    const uint16_t* fi_left = k > 0 ? a.Fi + (chain_nodes + a.off[k - 1] + 2ll * j) * N : nullptr;
    const uint16_t* fi_right = kb >= 0 ? a.Fi + (chain_nodes + a.off[kb] + jb) * N : nullptr;
    const uint16_t* la_right = kb >= 0 ? a.La + (chain_nodes + a.off[kb] + jb) * N : nullptr;
    const R nln = (R)a.neg_log_n;
    // the transition across the boundary (time-varying: row mid - 1 of the device arrays) into LDS
    const bool tv = m.Ft != nullptr;
    const R* gF = tv ? m.Ft + (mid - 1) * D * D : m.F;
    const R* gLQ = tv ? m.LQt + (mid - 1) * D * D : m.LQ;
    const R* gb = tv ? m.bt + (mid - 1) * D : m.b;
    const R* giL = tv ? m.idt + (mid - 1) * D : m.iLQ;
    const R ctr = tv ? m.ctt[mid - 1] : m.c_trans;
    for (int i = tid; i < D * PW_S; i += NCH) {
        const int r = i / PW_S, q = i - r * PW_S;
        L.F[i] = q < D ? gF[r * D + q] : (R)0;
        if constexpr (coupled) L.pot_mat[i] = q < D ? m.pot_mat[r * D + q] : (R)0;
    }
    for (int i = tid; i < CSW_MAXD * PW_LS; i += NCH) {
        const int r = i / PW_LS, q = i - r * PW_LS;
        L.LQ[i] = (r < D && q < D) ? gLQ[r * D + q] : (R)0;
    }
    if (tid < CSW_MAXD) L.b[tid] = tid < D ? gb[tid] : (R)0, L.iL[tid] = tid < D ? giL[tid] : (R)0;
    for (int i = tid; i < 2 * N * PW_S; i += NCH) L.xb[i] = 0;  // (xb and mu are adjacent)
    __syncthreads();
    {   // the N right-hand particles, transition means, potentials and the log-weights the two blocks bring: a particle across the 32 lanes of a half-wave
        const int lane = tid & 63, wv = tid >> 6, q = lane & 31, qq = q < D ? q : 0;
        const bool hi = lane >= 32;
        const int PP = NCH / 32;  // particles per pass
        const R* Frow = L.F + qq * PW_S;
        const R* Mrow = coupled ? L.pot_mat + qq * PW_S : nullptr;
        R* xl = L.tmp + (2 * wv + (hi ? 1 : 0)) * PW_S;
        const R bq = L.b[q];
        const R yq = (a.y && q < D) ? ((const R*)a.y)[mid * D + q] : (R)0;
        for (int s = 0; s * PP < N; ++s) {
            const int i = s * PP + 2 * wv + (hi ? 1 : 0);
            const bool pl = i < N;  // (uniform per half-wave)
            const int ir = pl ? i : 0;
            const int ia = la_left ? la_left[ir] : ir;
            const int ib = fi_right ? fi_right[ir] : ir;
            const R xa = q < D ? ((const R*)a.xs)[(((long long)c * T + mid - 1) * N + ia) * D + q] : (R)0;
            const R xv = q < D ? ((const R*)a.xs)[(((long long)c * T + mid) * N + ib) * D + q] : (R)0;
            xl[q] = xa;  // (a half-wave reads back only its own row: ordered inside the wave)
            __builtin_amdgcn_wave_barrier();
            R mq = bq;
#pragma unroll
            for (int p = 0; p < CSW_MAXD; ++p) mq = fma_(Frow[p], xl[p], mq);  // (columns beyond D are zeros on both sides: fma(0, 0, mq) = mq)
            __builtin_amdgcn_wave_barrier();
            R g;
            if constexpr (V == PotV::LOGI) g = logistic_half<R>(D, q, xv, yq, a.y, T, mid);
            else g = potential_half<R, V>(m, q, hi, xv, yq, Mrow);
            if (pl && q < D) {
                L.mu[i * PW_S + q] = mq;
                L.xb[i * PW_S + q] = xv;
            }
            if (pl && q == 0) {
                // -log N once a block has been stitched (operator.py:106-108), the LEAF's own while it is a single time step -- the left block at level 0,
                // the right one when no level below stitched it (kb < 0)
                R wl = nln, wr = nln;
                if (a.lwt) {
                    if (k == 0) wl = ((const R*)a.lwt)[((long long)c * T + mid - 1) * N + ia];
                    if (kb < 0) wr = ((const R*)a.lwt)[((long long)c * T + mid) * N + ib];
                } else if (mid == 1) {
                    wl = ((const R*)a.lw0)[(long long)c * N + ia];
                }
                pg[i] = g + wr;
                hh[i] = wl;
            }
        }
    }
    __syncthreads();
    const long long NN = (long long)N * N;
    const int Lc = (int)((NN + NCH - 1) / NCH);
    const long long p0 = (long long)tid * Lc;
    const long long p1 = p0 + Lc < NN ? p0 + Lc : NN;
    auto value = [&](int i, int jj) -> R { return (gauss_lane<R>(D, L.xb + jj * PW_S, L.mu + i * PW_S, L.LQ, L.iL, ctr) + pg[jj]) + hh[i]; };
    // pass 1: max
    R vmax = -INFINITY;
    {
        int i = (int)(p0 / N), jj = (int)(p0 - (long long)i * N);
#pragma unroll 1
        for (long long p = p0; p < p1; ++p) {
            const R v = value(i, jj);
            vmax = v > vmax ? v : vmax;
            if (++jj == N) jj = 0, ++i;
        }
    }
    {
        const int lane = tid & 63, wv = tid >> 6;
        const R wm = wave_max(vmax);
        if (lane == 0) red[wv] = wm;
        __syncthreads();
        R t16[16];
        load16<R>(red, t16);
        vmax = t16[0];
#pragma unroll
        for (int q = 1; q < 16; ++q) vmax = (q < nw && t16[q] > vmax) ? t16[q] : vmax;
        if (!(vmax - vmax == 0)) vmax = 0;
    }
    // pass 2: sub-chunk sums of exp(v - M), chunk sums, block cumsum
    const int Ls = (Lc + PIT_SC - 1) / PIT_SC;
    R s = 0;
    {
        int i = (int)(p0 / N), jj = (int)(p0 - (long long)i * N);
        long long p = p0;
#pragma unroll 1
        for (int b = 0; b < PIT_SC; ++b) {
            const long long pe = p0 + (long long)(b + 1) * Ls < p1 ? p0 + (long long)(b + 1) * Ls : p1;
            R sb = 0;
#pragma unroll 1
            for (; p < pe; ++p) {
                sb = sb + det_exp(value(i, jj) - vmax);
                if (++jj == N) jj = 0, ++i;
            }
            sub[b * NCH + tid] = sb;
            s = s + sb;
        }
    }
    block_cumsum<R>(s, cs, red, tid, nw);
    // pass 3: the draws
    uint16_t* Lo = a.Ls + (chain_nodes + a.off[k] + j) * N;
    uint16_t* Ro = a.Rs + (chain_nodes + a.off[k] + j) * N;
    uint16_t* Fo = a.Fi + (chain_nodes + a.off[k] + j) * N;
    uint16_t* Ao = a.La + (chain_nodes + a.off[k] + j) * N;
    if (tid < N && (!root || tid == 0)) {
        int il = 0, jr = 0;
        if (root || tid > 0) {
            const R un = pit_uniform<R>(a, a.u_res, STREAM_U_RES, ((long long)c * T + mid) * N + tid);
            const R r = cs[NCH - 1] * ((R)1 - un);
            int ts = lower_bound<R>(cs, NCH, r);
            const int last_chunk = (int)((NN - 1) / Lc);
            ts = ts < last_chunk ? ts : last_chunk;
            const R pre = ts > 0 ? cs[ts - 1] : (R)0;
            const long long c0 = (long long)ts * Lc;
            const long long c1 = c0 + Lc < NN ? c0 + Lc : NN;
            // the sub-chunk: first b whose running sum reaches r, else the last non-empty one
            const int nsub = (int)((c1 - c0 + Ls - 1) / Ls);
            int bsel = nsub - 1;
            R acc = 0;
            for (int b = 0; b < nsub; ++b) {
                const R nacc = acc + sub[b * NCH + ts];
                const R cvb = ts > 0 ? pre + nacc : nacc;
                if (cvb >= r || b == nsub - 1) {
                    bsel = b;
                    break;
                }
                acc = nacc;
            }
            const long long q0 = c0 + (long long)bsel * Ls;
            const long long q1 = q0 + Ls < c1 ? q0 + Ls : c1;
            long long psel = q1 - 1;
            int i = (int)(q0 / N), jj = (int)(q0 - (long long)i * N);
#pragma unroll 1
            for (long long p = q0; p < q1; ++p) {
                acc = acc + det_exp(value(i, jj) - vmax);
                const R cv = ts > 0 ? pre + acc : acc;
                if (cv >= r) {
                    psel = p;
                    break;
                }
                if (++jj == N) jj = 0, ++i;
            }
            il = (int)(psel / N);
            jr = (int)(psel - (long long)il * N);
        }
        Lo[tid] = (uint16_t)il;
        Ro[tid] = (uint16_t)jr;
        Fo[tid] = fi_left ? fi_left[il] : (uint16_t)il;
        Ao[tid] = la_right ? la_right[jr] : (uint16_t)jr;
    }
}

// the leaves and the up-sweep; the model block is csmc_wide.hip's (cw_model: uploaded only when it changed), the gradient its prologue kernel (k_cw_grad)
template <typename R> static int run_pw(auxssm_ctx* h, const auxssm_fk_model* fk, PitArgs& a, void* ctt) {
    FkW<R> m;
    if (int rc = cw_model<R>(h, fk, m)) return rc;
    const int D = m.D;
    const bool coupled = pot_has_matrix(pot_variant(m.potential));
    CsmcArgs ca{};
    ca.C = a.C; ca.T = a.T; ca.N = a.N;
    ca.y = a.y; ca.shd = a.shd; ca.x = a.x; ca.u = const_cast<void*>(a.u); ca.grad = const_cast<void*>(a.grad);
    ca.noise_mode = a.noise_mode; ca.key0 = a.key0; ca.key1 = a.key1; ca.eps_aux = a.eps_aux;
    int rc = csmc_prologue<R, false>(h, fk, ca, ctt, m, false, [&] {
        cw_grad_launch<R>(h, ca, m);
        return AUXSSM_OK;
    });
    if (rc) return rc;
    rc = with_pot(m.potential, [&](auto pv) {
        constexpr PotV V = decltype(pv)::value;
        return launch(h, k_pitw_leaves<R, V>, dim3(a.T, a.C), dim3(PWL_NT), PwLeafLds<R>::bytes(D, coupled), a, m);
    });
    if (rc) return rc;
    const int NCH = pit_nch(a.N);  // part of the arithmetic contract (header of pit.hip)
    const size_t lds = PwStitchLds<R>::bytes(D, a.N, NCH, coupled);
    ProfScope ps(h, AUXSSM_K_PIT_STITCH);
    for (int k = 0; k < a.K; ++k) {
        const long long nodes = ((long long)a.T + (2ll << k) - 1) >> (k + 1);
        rc = with_pot(m.potential, [&](auto pv) {
            constexpr PotV V = decltype(pv)::value;
            return launch(h, k_pitw_stitch<R, V>, dim3((unsigned)nodes, a.C), dim3(NCH), lds, a, m, k);
        });
        if (rc) return rc;
    }
    return AUXSSM_OK;
}

int run_pit_wide(auxssm_ctx* h, int dtype, const auxssm_fk_model* fk, PitArgs& a, void* ctt) {
    if (dtype == AUXSSM_F32) return run_pw<float>(h, fk, a, ctt);
    return run_pw<double>(h, fk, a, ctt);
}

}  // namespace ax
