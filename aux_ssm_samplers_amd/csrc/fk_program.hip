// fk_program.hip -- user-defined Feynman-Kac models for the sequential cSMC sweep: the program (hipRTC: the user's source between fk_user_pre.h and
// fk_user.h, every instantiation of the sweep kernels the launcher may pick) and its modules (hipModuleLoadData, once per handle).  The sweep itself
// is csmc.hip::auxssm_csmc_sweep_program: the validation, workspace and chain batching of auxssm_csmc_sweep, with module launches.
#include <hip/hiprtc.h>

#include <atomic>
#include <cstring>
#include <string>
#include <vector>

#include "fk_program.h"

namespace ax {

static std::atomic<unsigned long long> g_fk_next_id{1};

// the modules of one handle: one per program it has swept with (a program freed later leaves its module here until the handle goes)
struct FkModules {
    struct Entry {
        unsigned long long id;
        hipModule_t mod;
        hipFunction_t f[FK_NFUNC];
    };
    std::vector<Entry> v;
};

void fk_modules_release(auxssm_ctx* h) {
    auto* ms = static_cast<FkModules*>(h->fk_modules);
    if (!ms) return;
    for (auto& e : ms->v) (void)hipModuleUnload(e.mod);
    delete ms;
    h->fk_modules = nullptr;
}

int fk_program_functions(auxssm_ctx* h, const auxssm_fk_program_s* p, const hipFunction_t** out) {
    auto* ms = static_cast<FkModules*>(h->fk_modules);
    if (!ms) h->fk_modules = ms = new FkModules();
    for (auto& e : ms->v)
        if (e.id == p->id) {
            *out = e.f;
            return AUXSSM_OK;
        }
    FkModules::Entry e{};
    e.id = p->id;
    AX_HIP(hipModuleLoadData(&e.mod, p->code.data()));
    for (int i = 0; i < p->nfunc; ++i) {
        const hipError_t rc = hipModuleGetFunction(&e.f[i], e.mod, p->lowered[i].c_str());
        if (rc != hipSuccess) {
            (void)hipModuleUnload(e.mod);
            set_error("hipModuleGetFunction(%s): %s", p->lowered[i].c_str(), hipGetErrorString(rc));
            return AUXSSM_ERR_HIP;
        }
    }
    ms->v.push_back(e);
    *out = ms->v.back().f;
    return AUXSSM_OK;
}

}  // namespace ax

using namespace ax;

static void copy_log(char* log, size_t log_len, const std::string& s) {
    if (!log || !log_len) return;
    const size_t n = s.size() < log_len - 1 ? s.size() : log_len - 1;
    memcpy(log, s.data(), n);
    log[n] = 0;
}

extern "C" int auxssm_fk_program_compile(const char* source, const char* include_dir, int dtype, int32_t dx, int32_t flags, char* log, size_t log_len,
                                         auxssm_fk_program* out) {
    copy_log(log, log_len, "");
    if (!source || !include_dir || !out) {
        set_error("source/include_dir/out must be non-NULL");
        return AUXSSM_ERR_ARG;
    }
    *out = nullptr;
    if (dtype != AUXSSM_F32 && dtype != AUXSSM_F64) {
        set_error("dtype must be 0 (f32) or 1 (f64)");
        return AUXSSM_ERR_ARG;
    }
    if (dx < 1 || dx > CS_MAXD) {
        set_error("dx=%d: user-defined models run the sequential kernels of 1 <= dx <= %d", dx, CS_MAXD);
        return AUXSSM_ERR_UNSUPPORTED;
    }
    if (flags & ~(AUXSSM_FK_USER_POTENTIAL | AUXSSM_FK_USER_MEAN | AUXSSM_FK_USER_GRADIENT) || !(flags & (AUXSSM_FK_USER_POTENTIAL | AUXSSM_FK_USER_MEAN))) {
        set_error("flags must be a non-empty set of AUXSSM_FK_USER_POTENTIAL | AUXSSM_FK_USER_MEAN, optionally | AUXSSM_FK_USER_GRADIENT (got %d)", flags);
        return AUXSSM_ERR_ARG;
    }
    const bool ug = flags & AUXSSM_FK_USER_POTENTIAL, um = flags & AUXSSM_FK_USER_MEAN, gr = flags & AUXSSM_FK_USER_GRADIENT;
    // #line: hipRTC's diagnostics count the lines of the user's source
    const std::string src = std::string("#include \"fk_user_pre.h\"\n#line 1 \"model.hip\"\n") + source + "\n#include \"fk_user.h\"\n";
    const std::string R = dtype == AUXSSM_F32 ? "float" : "double", Ds = std::to_string(dx);
    const std::string P = "ax::FkUserPolicy<" + R + ", " + Ds + ", " + (ug ? "true" : "false") + ", " + (um ? "true" : "false") + ">";
    const std::string U = "ax::FkUser<" + R + ">";
    std::string names[FK_NNAMES];
    const int nws[3] = {0, 8, 16};
    for (int i = 0; i < 3; ++i) {
        names[FK_FWD0 + i] = "ax::k_csmc_fwd<" + R + ", " + Ds + ", false, false, " + std::to_string(nws[i]) + ", 0, " + P + ", " + U + ">";
        names[FK_BWD0 + i] = "ax::k_csmc_bwd<" + R + ", " + Ds + ", false, " + std::to_string(nws[i]) + ", " + P + ", " + U + ">";
        if (gr) names[FK_FWDG0 + i] = "ax::k_csmc_fwd<" + R + ", " + Ds + ", false, true, " + std::to_string(nws[i]) + ", 0, " + P + ", " + U + ">";
    }
    names[FK_BOUND] = "ax::k_fk_bound<" + R + ", " + Ds + ", " + (ug ? "ax::fk_has_bound<" + R + ", " + Ds + ">::value" : std::string("false")) + ">";
    names[FK_BOUND_TRUE] = "ax::k_fk_bound<" + R + ", " + Ds + ", true>";
    if (gr) {
        names[FK_GRAD] = "ax::k_csmc_grad<" + R + ", " + Ds + ", " + P + ", " + U + ">";
        names[FK_PROBE_G] = "ax::k_fk_probe<" + R + ", " + Ds + ", 0, ax::fk_has_grad_log_g<" + R + ", " + Ds + ">::value>";
        names[FK_PROBE_G_TRUE] = "ax::k_fk_probe<" + R + ", " + Ds + ", 0, true>";
        names[FK_PROBE_M] = "ax::k_fk_probe<" + R + ", " + Ds + ", 1, ax::fk_has_mean_vjp<" + R + ", " + Ds + ">::value>";
        names[FK_PROBE_M_TRUE] = "ax::k_fk_probe<" + R + ", " + Ds + ", 1, true>";
    }

    hiprtcProgram prog;
    if (hiprtcCreateProgram(&prog, src.c_str(), "fk_program.hip", 0, nullptr, nullptr) != HIPRTC_SUCCESS) {
        set_error("hiprtcCreateProgram failed");
        return AUXSSM_ERR_HIP;
    }
    for (auto& n : names)
        if (!n.empty()) hiprtcAddNameExpression(prog, n.c_str());  // (a program without AUXSSM_FK_USER_GRADIENT: the kernels of the plain sweep only)
    const std::string inc = std::string("-I") + include_dir;
    const std::string dg = std::string("-DAXFK_USER_G=") + (ug ? "1" : "0"), dm = std::string("-DAXFK_USER_M=") + (um ? "1" : "0");
    const char* opts[] = {"--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", inc.c_str(), dg.c_str(), dm.c_str()};
    const hiprtcResult rc = hiprtcCompileProgram(prog, (int)(sizeof(opts) / sizeof(opts[0])), opts);
    if (rc != HIPRTC_SUCCESS) {
        size_t n = 0;
        std::string lg;
        if (hiprtcGetProgramLogSize(prog, &n) == HIPRTC_SUCCESS && n) {
            lg.resize(n);
            hiprtcGetProgramLog(prog, &lg[0]);
        }
        copy_log(log, log_len, lg);
        hiprtcDestroyProgram(&prog);
        set_error("hipRTC could not compile the model source: %s", hiprtcGetErrorString(rc));
        return AUXSSM_ERR_ARG;
    }
    auto* p = new auxssm_fk_program_s();
    p->id = g_fk_next_id++;
    p->dtype = dtype;
    p->dx = dx;
    p->flags = flags;
    p->nfunc = gr ? FK_NFUNC : FK_NFUNC_PLAIN;
    std::string lowered[FK_NNAMES];
    for (int i = 0; i < FK_NNAMES; ++i) {
        if (names[i].empty()) continue;
        const char* low = nullptr;
        if (hiprtcGetLoweredName(prog, names[i].c_str(), &low) != HIPRTC_SUCCESS || !low) {
            hiprtcDestroyProgram(&prog);
            delete p;
            set_error("hiprtcGetLoweredName(%s) failed", names[i].c_str());
            return AUXSSM_ERR_HIP;
        }
        lowered[i] = low;
        if (i < FK_NFUNC) p->lowered[i] = low;
    }
    // k_fk_bound<R, D, fk_has_bound<R, D>::value> IS k_fk_bound<R, D, true> exactly when the source defines log_g_bound (a user potential only)
    p->has_bound = ug && lowered[FK_BOUND] == lowered[FK_BOUND_TRUE];
    // a gradient program needs the derivative of every user-defined part (the same comparison: the probe with the detected value IS its `true` twin)
    std::string missing;
    if (gr && ug && lowered[FK_PROBE_G] != lowered[FK_PROBE_G_TRUE])
        missing += "  template <typename R, int D> __device__ void grad_log_g(int t, const R* x, const R* xprev, const R* y, const R* theta, R* gx, R* gxprev)";
    if (gr && um && lowered[FK_PROBE_M] != lowered[FK_PROBE_M_TRUE])
        missing += "  template <typename R, int D> __device__ void mean_vjp(int t, const R* xprev, const R* theta, const R* v, R* out)";
    if (!missing.empty()) {
        hiprtcDestroyProgram(&prog);
        delete p;
        set_error("gradient-informed proposals differentiate the user-defined model parts; the source must define (it lacks them, or has another signature):%s",
                  missing.c_str());
        return AUXSSM_ERR_UNSUPPORTED;
    }
    size_t cs = 0;
    if (hiprtcGetCodeSize(prog, &cs) != HIPRTC_SUCCESS || !cs) {
        hiprtcDestroyProgram(&prog);
        delete p;
        set_error("hiprtcGetCodeSize failed");
        return AUXSSM_ERR_HIP;
    }
    p->code.resize(cs);
    const hiprtcResult rg = hiprtcGetCode(prog, p->code.data());
    hiprtcDestroyProgram(&prog);
    if (rg != HIPRTC_SUCCESS) {
        delete p;
        set_error("hiprtcGetCode failed: %s", hiprtcGetErrorString(rg));
        return AUXSSM_ERR_HIP;
    }
    *out = p;
    return AUXSSM_OK;
}

extern "C" int auxssm_fk_program_info(auxssm_fk_program prog, int32_t* dtype, int32_t* dx, int32_t* flags, int32_t* has_bound) {
    if (!prog) {
        set_error("program is NULL");
        return AUXSSM_ERR_ARG;
    }
    if (dtype) *dtype = prog->dtype;
    if (dx) *dx = prog->dx;
    if (flags) *flags = prog->flags;
    if (has_bound) *has_bound = prog->has_bound ? 1 : 0;
    return AUXSSM_OK;
}

extern "C" int auxssm_fk_program_free(auxssm_fk_program prog) {
    delete prog;
    return AUXSSM_OK;
}
