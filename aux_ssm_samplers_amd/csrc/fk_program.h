// fk_program.h -- a compiled user-defined Feynman-Kac model (fk_program.hip) as the sweep launcher (csmc.hip) sees it.
#pragma once
#include <string>
#include <vector>

#include "ctx.h"
#include "csmc_sweep.h"

namespace ax {

// the program's kernels: forward / backward pass with NW = 0 / 8 / 16 (csmc.hip::nw_class; fk_fwd_index / fk_bwd_index pick among them), and the user potential's bound; a gradient program
// (AUXSSM_FK_USER_GRADIENT) adds the GRAD = true forward passes and the gradient kernel k_csmc_grad
enum { FK_FWD0 = 0, FK_BWD0 = 3, FK_BOUND = 6, FK_NFUNC_PLAIN = 7, FK_FWDG0 = 7, FK_GRAD = 10, FK_NFUNC = 11 };
// (name expressions that are not launched functions: k_fk_bound<R, D, true>, whose lowered name equals FK_BOUND's iff the source defines log_g_bound, and
// the presence probes of a gradient program's derivatives, fk_user.h::k_fk_probe, each with its `true` twin)
enum { FK_BOUND_TRUE = FK_NFUNC, FK_PROBE_G, FK_PROBE_G_TRUE, FK_PROBE_M, FK_PROBE_M_TRUE, FK_NNAMES };

// the module's functions on handle h (loaded on first use)
int fk_program_functions(auxssm_ctx* h, const auxssm_fk_program_s* p, const hipFunction_t** out);

}  // namespace ax

struct auxssm_fk_program_s {
    unsigned long long id = 0;  // (never reused: the handles' module caches key on it)
    int dtype = 0, dx = 0, flags = 0;
    int nfunc = 0;           // the kernels of lowered[] it holds: FK_NFUNC_PLAIN, or FK_NFUNC for a gradient program
    bool has_bound = false;  // the source defines log_g_bound
    std::vector<char> code;  // the gfx950 code object
    std::string lowered[ax::FK_NFUNC];
};
