// What the wide-state drivers (csrc/wide.hip) reserve, as their entry tables say it, for the shapes of profiles/r15_wide_workspace.txt.
// Host only: the size functions read the handle's CU count and nothing else, so no device is opened.
//   hipcc -std=c++17 tools/wide_ws_report.cpp -Laux_ssm_samplers_amd -lauxssm -Wl,-rpath,$PWD/aux_ssm_samplers_amd -o /tmp/wide_ws_report && /tmp/wide_ws_report [num_cu]
#include <cstdio>
#include <cstdlib>

#include "../aux_ssm_samplers_amd/csrc/ctx.h"

int main(int argc, char** argv) {
    auxssm_ctx h;
    h.num_cu = argc > 1 ? atoi(argv[1]) : 256;  // MI355X
    const int filt[][4] = {{1, 1, 5, 3}, {1, 9, 5, 3}, {1, 41, 8, 8}, {3, 40, 5, 2}, {16, 130, 16, 5}, {70, 300, 6, 11}, {16, 8192, 64, 64}};
    const int sweep[][4] = {{2, 25, 20, 50}, {5, 80, 8, 8}, {16, 8192, 64, 64}};
    for (int dtype : {AUXSSM_F32, AUXSSM_F64})
        for (int parallel : {1, 0}) {
            const char* tag = dtype == AUXSSM_F32 ? "fp32" : "fp64";
            for (const auto& s : filt) {
                const ax::KDims kd{s[0], s[1], 1};
                printf("filter  %s parallel=%d S=%d T=%d d=%d p=%d  %zu\n", tag, parallel, s[0], s[1], s[2], s[3],
                       ax::wide_kalman_entry(dtype)->filter_ws(&h, kd, parallel, s[2], s[3]));
                printf("sample  %s parallel=%d S=%d T=%d d=%d  %zu\n", tag, parallel, s[0], s[1], s[2], ax::wide_sample_entry(dtype)->sample_ws(&h, kd, parallel, s[2]));
                printf("logpdf  %s parallel=%d S=%d T=%d d=%d p=%d  %zu\n", tag, parallel, s[0], s[1], s[2], s[3],
                       ax::wide_kalman_entry(dtype)->logpdf_ws(&h, kd, s[2], s[3]));
            }
            for (const auto& s : sweep) {
                const ax::KDims kd{s[0], s[1], 1};
                printf("sweep-logpdf  %s parallel=%d C=%d T=%d d=%d po=%d  %zu\n", tag, parallel, s[0], s[1], s[2], s[3],
                       ax::wide_sweep_logpdf_entry(dtype)->ws(&h, kd, s[2], s[3]));
            }
            if (parallel) printf("gain-tab  %s T=8192 d=64 p=64  %zu\n", tag, ax::wide_gain_tab_bytes(dtype, 8192, 64, 64));
        }
    return 0;
}
