// TEST INFRASTRUCTURE ONLY (plain g++, no GPU): the chunk rule of the fused sweep in csrc/fs_chunk.h.
// fs_chunk_rule against the mirror tests/fused_cases.py::chunk_len (64 from 1024 chains, 32 from 96, else 16, at T <= 130 on 256 compute units), the shapes at
// which the clause for 256 <= C < 1024 does and does not select 64, and 1 <= E <= max(T, 2) everywhere.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "../../aux_ssm_samplers_amd/csrc/fs_chunk.h"

static int fails = 0;
#define CHECK(cond, ...)                      \
    do {                                      \
        if (!(cond)) {                        \
            ++fails;                          \
            if (fails < 20) {                 \
                std::printf("FAILED: ");      \
                std::printf(__VA_ARGS__);     \
                std::printf("\n");            \
            }                                 \
        }                                     \
    } while (0)

static int mirror(int C) { return C >= 1024 ? 64 : C >= 96 ? 32 : 16; }  // tests/fused_cases.py::chunk_len

static void rule_table() {
    const int before = fails;
    // (a)
    const int Ts[] = {64, 70, 97, 130};
    for (int C = 1; C <= 1100; ++C)
        for (int T : Ts) CHECK(fs_chunk_rule(256, C, T) == mirror(C), "(a) rule(256, %d, %d) = %d, mirror %d", C, T, fs_chunk_rule(256, C, T), mirror(C));
    // (b)
    CHECK(fs_chunk_rule(256, 256, 65536) == 64, "(b) 256 x 65536");
    CHECK(fs_chunk_rule(256, 256, 65473) == 64, "(b) 256 x 65473");
    CHECK(fs_chunk_rule(256, 512, 32768) == 64, "(b) 512 x 32768");
    for (int T = 64; T <= 70000; T += (T < 300 ? 1 : 997))
        for (int C : {1024, 1025, 1026, 2048, 4096}) CHECK(fs_chunk_rule(256, C, T) == 64, "(b) %d x %d", C, T);
    // (c)
    CHECK(fs_chunk_rule(256, 256, 65472) == 32, "(c) 256 x 65472");
    CHECK(fs_chunk_rule(256, 256, 32768) == 32, "(c) 256 x 32768");
    CHECK(fs_chunk_rule(256, 130, 3001) == 32, "(c) 130 x 3001");
    CHECK(fs_chunk_rule(256, 255, 65536) == 32, "(c) 255 x 65536");
    // (d)
    for (int cu : {1, 4, 32, 64, 256, 304})
        for (int C : {1, 2, 63, 64, 95, 96, 128, 255, 256, 257, 511, 512, 1023, 1024, 5000})
            for (int T = 1; T <= 200000; T += (T < 300 ? 1 : 4999)) {
                const int E = fs_chunk_rule(cu, C, T);
                CHECK(E >= 1 && (T + E - 1) / E >= 1 && E <= (T > 2 ? T : 2), "(d) rule(%d, %d, %d) = %d", cu, C, T, E);
            }
    std::printf("rule table %s\n", fails == before ? "ok" : "WRONG");
}

int main() {
    rule_table();
    std::printf("%s\n", fails ? "DIFFERENT" : "all equal");
    return fails ? 1 : 0;
}
