// fs_chunk.h -- the chunk rule of the fused sweep (fused_shared.h): integer bookkeeping that holds no device type.
// Plain C++ (any host compiler reads it: tests/hostsim_chunk/chunk_check.cpp tabulates it); included inside namespace ax by fused_shared.h.
#pragma once

#if defined(__HIPCC__)
#define FS_PURE __host__ __device__ inline
#else
#define FS_PURE inline
#endif

constexpr int FS_RULE_TILE = 64;  // chains per workgroup of the affine passes the first clause was sized on (kernels.hip.h: TB_CM)

// The chunk length of the fused sweep: time steps per (chain tile, chunk) workgroup of the two chain passes.  A function of the device's compute units, the chain count
// and T only: the workspace (fused_ws) and the launch (run_fused_shared) both come here, so they always agree.
FS_PURE int fs_chunk_rule(int num_cu, int C, int T) {
    constexpr int waves = 10;
    const long long stiles = (C + FS_RULE_TILE - 1) / FS_RULE_TILE;
    long long want = (long long)num_cu * 4 * waves / stiles;
    if (want < 1) want = 1;
    long long E = (T + want - 1) / want;
    if (E < 16) E = 16;
    if (E > 32) E = 32;
    // measured at T = 65536, d = 4, fp64 once pass C stopped walking the innovations (rows of 88 / 84 / 68 reals: 64 steps = 45 KB of LDS at most): 64 chains 16 (81k
    // sweeps/s; 32: 76k), 96 chains 32 (100k; 16: 96k), 128 chains 32 (125k; 16: 118k), 256 chains 32 or 64 (175k; 24: 172k), 1024 chains 64 (228k; 32: 220k)
    // with u out of memory (pass AC's rows 82 reals, pass E's 84 + the normal tables) 64 steps at 256 chains measured 278.2k-282.6k sweeps/s against 269.3k-273.8k
    // for 32 (profiles/r19_tuning_variants_bench.txt).
    // From 256 chains on the plain mapping's workgroup is 256 chains wide, and what a chunk costs beyond its steps (its prologue in both passes, its records in
    // k_fs_mid, its partial sums in k_fs_accept) is paid ceil(T / E) ceil(C / 256) times.  64 steps halve that count, and are taken while the grid still gives every
    // compute unit the four workgroups pass AC's registers admit: ceil(T / 64) ceil(C / 256) >= 4 num_cu.  Below that a 64-step grid leaves slots empty and 32 stands
    // (256 x 32768 on 256 compute units, every short T).  Measured (profiles/r21_parent_vs_chunk64_bench.txt): 256 x 65536, 512 x 32768 and 512 x 65536, d = 4, fp64.
    // A 64-step block of pass AC's rows is 50 KB of LDS, three workgroups per compute unit where the registers admit four; staging it in windows of 32 rows gave the
    // fourth back and LOST (two barriers per window inside the time loop: DESIGN.md has the figures), so both passes stage the whole chunk.
    // The chunk length sets the association of the two aggregate scans, so where the clause applies x agrees with the 32-step sweep to rounding, not bit for bit
    // ("64-step chunks from 256 chains").
    const long long tiles256 = (C + 255) / 256, chunks64 = ((long long)T + 63) / 64;
    if (C >= 1024) E = 64;
    else if (C >= 256 && chunks64 * tiles256 >= (long long)4 * num_cu) E = 64;
    else if (C >= 96) E = 32;
    if (E > T) E = T > 2 ? T : 2;
    return (int)E;
}
