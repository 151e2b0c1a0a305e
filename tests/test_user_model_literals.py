"""CPU checks of the multi-dimensional user-model tests' references and inputs (tests/user_models.py; the GPU comparisons are tests/test_gpu_user_model_multidim.py).

1. Every device source compiles (hipRTC needs no device) for fp32 and fp64 at its state dimension, with and without the gradient kernels, and reports the
   log_g_bound it defines.
2. The sources themselves, compiled for the host: values equal the literal's, derivatives agree with central differences of the literal log-densities.
3. The exact comparison of ancestors with the fp64 literal is well posed for every case of user_models.CASES: no resampling or backward draw within 1e-8 of a
   cumulative-weight boundary, the particle systems neither degenerate nor stuck on the reference path, and the tightened inputs do underflow.
4. NumPy's own fp32 resampling stays under the tie-rate cap the GPU test applies to the device."""
import numpy as np
import pytest

from oracle import csmc_np as L
from tests import user_models as M


def _sources():
    return [pytest.param(*s, id=f"{s[0]}-d{s[2]}") for s in M.sources()]


@pytest.mark.parametrize("name,source,dx,flags,has_bound", _sources())
def test_sources_compile_and_report_their_bound(name, source, dx, flags, has_bound):
    from aux_ssm_samplers_amd import _lib
    from aux_ssm_samplers_amd.csmc import _device
    for dtype in (np.float32, np.float64):
        for grad in (0, _lib.FK_USER_GRADIENT):
            info = _device.program_info(_device.compile_program(source, dtype, dx, flags | grad))
            assert info["dx"] == dx and info["flags"] == flags | grad and info["dtype"] == _lib.dtype_code(dtype)
            assert bool(info["has_bound"]) == has_bound


def test_case_list_is_complete():
    """the gaps the GPU file is there for are all in the shared case list"""
    ids = [c.id for c in M.CASES]
    assert len(set(ids)) == len(ids)
    specs = {c.spec for c in M.CASES}
    assert {(s.dx, s.p) for s in specs if s.model == "range"} >= {(2, 1), (2, 3), (4, 3), (4, 6)}          # p < dx, p > dx, p == dx - 1
    assert {s.parts for s in specs if s.model == "lorenz"} == {"user", "potential", "mean"}
    assert {c.N for c in M.cases("N")} == {2, 3, 65, 512, 1000, 1024} and {c.spec.T for c in M.cases("T")} == {1, 2}
    assert {(c.spec.bound, c.spec.tight) for c in M.cases("bound")} == {(b, t) for b in M.BOUNDS for t in (False, True)}
    for model in ("range", "lorenz", "increments", "growth_nd"):
        cs = [c for c in M.CASES if c.spec.model == model]
        assert {(c.proposal, c.backward) for c in cs if c.gradient is None} >= {(p, b) for p in ("independent", "bootstrap") for b in (True, False)}
        assert {c.gradient for c in cs} == {None, True, "exact"}


# ---- the device sources themselves, compiled for the host -------------------------------------------------------------------------------------------
_HOST = r"""
#include <cmath>
#define __device__
using namespace std;
%s
extern "C" {
%s
}
"""
_WRAP = dict(
    log_g="double h_log_g(int t, const double* x, const double* xp, const double* y, const double* th) { return log_g<double, DX>(t, x, xp, y, th); }",
    log_g_bound="double h_log_g_bound(int t, const double* y, const double* th) { return log_g_bound<double, DX>(t, y, th); }",
    grad_log_g="void h_grad_log_g(int t, const double* x, const double* xp, const double* y, const double* th, double* gx, double* gxp) "
               "{ grad_log_g<double, DX>(t, x, xp, y, th, gx, gxp); }",
    mean="void h_mean(int t, const double* xp, const double* th, double* mu) { mean<double, DX>(t, xp, th, mu); }",
    mean_vjp="void h_mean_vjp(int t, const double* xp, const double* th, const double* v, double* out) { mean_vjp<double, DX>(t, xp, th, v, out); }")


class _HostSource:
    """the functions of a device source (which uses nothing of the device but its math library) instantiated for double at D = dx by the host compiler:
    the very text hipRTC compiles, evaluated on the CPU"""

    def __init__(self, source, dx, workdir):
        import ctypes
        import subprocess
        names = [n for n in _WRAP if f" {n}(" in source]
        cpp = workdir / "model.cpp"
        cpp.write_text(_HOST % (source, "\n".join(_WRAP[n] for n in names)))
        so = workdir / "model.so"
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", f"-DDX={dx}", str(cpp), "-o", str(so)])
        self.lib, self.dx, self.c = ctypes.CDLL(str(so)), dx, ctypes
        for n in ("log_g", "log_g_bound"):
            if n in names:
                getattr(self.lib, "h_" + n).restype = ctypes.c_double

    def _p(self, a):
        return None if a is None else np.ascontiguousarray(a, np.float64).ctypes.data_as(self.c.POINTER(self.c.c_double))

    def log_g(self, t, x, xp, y, th):
        return self.lib.h_log_g(int(t), self._p(x), self._p(xp), self._p(y), self._p(th))

    def log_g_bound(self, t, y, th):
        return self.lib.h_log_g_bound(int(t), self._p(y), self._p(th))

    def grad_log_g(self, t, x, xp, y, th):
        gx, gxp = np.zeros(self.dx), np.zeros(self.dx)   # (zero-filled by the caller: the contract of csrc/fk_user_pre.h)
        self.lib.h_grad_log_g(int(t), self._p(x), self._p(xp), self._p(y), self._p(th), self._p(gx), self._p(gxp) if xp is not None else None)
        return gx, gxp

    def mean(self, t, xp, th):
        mu = np.zeros(self.dx)
        self.lib.h_mean(int(t), self._p(xp), self._p(th), self._p(mu))
        return mu

    def mean_vjp(self, t, xp, th, v):
        out = np.zeros(self.dx)
        self.lib.h_mean_vjp(int(t), self._p(xp), self._p(th), self._p(v), self._p(out))
        return out


def _rel(got, want):
    return float(np.max(np.abs(got - want)) / max(1.0, np.max(np.abs(want))))


def _fd_accuracy():
    """the error of csmc_np.grad_fd on a log-density whose gradient is known in closed form: Gaussian observations, d/dx = (y - x) / sig^2"""
    rng = np.random.default_rng(0)
    worst = 0.0
    for _ in range(100):
        d = int(rng.integers(1, 5))
        x, y, sig = 3 * rng.standard_normal(d), 3 * rng.standard_normal(d), float(0.3 + rng.random())
        pot = L.ObsPotential("gauss", y, sig, first=True)
        worst = max(worst, _rel(L.grad_fd(lambda v: float(pot(v)), x), (y - x) / (sig * sig)))
    return worst


_DERIV_SPECS = [M.Spec("range", 2, 3), M.Spec("range", 4, 6), M.Spec("lorenz", 3, 3), M.Spec("increments", 2, 2), M.Spec("growth_nd", 4, 1)]


@pytest.mark.parametrize("spec", _DERIV_SPECS, ids=[s.name for s in _DERIV_SPECS])
def test_device_sources_on_the_host_agree_with_the_literal_and_its_finite_differences(spec, tmp_path):
    """The device source of each model, compiled for the host, at 100 random points (time step, state and previous state near the simulated path, cotangent):
    log_g, mean and log_g_bound equal the literal's potential, mean and supremum to 1e-12 (relative to max(1, |value|)); grad_log_g (gx and gxprev) and mean_vjp
    agree with csmc_np.grad_fd of the LITERAL potential and of v . mean(x).  The allowance for the derivatives is 10 times grad_fd's own error on the Gaussian
    observation density, whose gradient is known in closed form, both relative to max(1, |gradient|_inf).  Measured: grad_fd's error 9.6e-11 (allowance 9.6e-10);
    the sources' largest deviation: range 2.3e-10, lorenz 1.7e-10, increments 1.2e-10, growth_nd 6.5e-10.  A sweep mismatch on the GPU therefore points at the
    kernels, not at the calculus of the test's own sources."""
    allow = 10 * _fd_accuracy()
    rng = np.random.default_rng(1)
    d = M.data(spec)
    dev = M.device(spec)
    H = _HostSource(dev[3].source, spec.dx, tmp_path)
    th_g, th_m = np.asarray(dev[3].theta, np.float64), np.asarray(dev[2].theta, np.float64)
    _, G0, Mt, Gt = M.literal(spec)
    worst_value = worst_grad = 0.0
    for _ in range(100):
        t = int(rng.integers(1, spec.T))
        x, xp, v = d["x"][t] + 0.5 * rng.standard_normal(spec.dx), d["x"][t - 1] + 0.5 * rng.standard_normal(spec.dx), rng.standard_normal(spec.dx)
        y, gp, mp = d["y"][t], L._tree_index(Gt.params, t - 1), L._tree_index(Mt.params, t - 1)
        lit_g = lambda a, b: float(Gt(a, b, gp))
        lit_mean = lambda a: Mt.mean(a, mp) if isinstance(Mt.params, tuple) else Mt.mean(a, t)
        gx, gxp = H.grad_log_g(t, x, xp, y, th_g)
        worst_value = max(worst_value, _rel(np.array(H.log_g(t, x, xp, y, th_g)), np.array(lit_g(x, xp))), _rel(H.mean(t, xp, th_m), lit_mean(xp)),
                          _rel(np.array(H.log_g_bound(t, y, th_g)), M.exact_bound(spec)[t]),
                          _rel(np.array(H.log_g(0, x, None, d["y"][0], th_g)), np.array(float(G0(x)))))
        worst_grad = max(worst_grad, _rel(gx, L.grad_fd(lambda a: lit_g(a, xp), x)), _rel(gxp, L.grad_fd(lambda a: lit_g(x, a), xp)),
                         _rel(H.mean_vjp(t, xp, th_m, v), L.grad_fd(lambda a: float(v @ lit_mean(a)), xp)))
    print(f"{spec.name}: values' worst {worst_value:.2e}; grad_fd accuracy x 10 = {allow:.2e}, derivatives' worst = {worst_grad:.2e}")
    assert worst_value <= 1e-12
    assert worst_grad <= allow


# ---- well-posedness of the exact comparison ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", M.CASES, ids=[c.id for c in M.CASES])
def test_exact_ancestor_comparison_is_well_posed(case):
    """The GPU tests demand EQUAL ancestors of the device and the fp64 literal while their log-weights agree to 1e-10: fair only if no draw r = c[-1] (1 - u) lies
    within rounding of a cumulative-weight boundary c[j].  Per case, from the literal sweep: (a) the smallest |r - c[j]| over all resampling and backward draws is
    >= 1e-8 (two orders above what a 1e-10 log-weight error moves a boundary); (b) N >= 64: the smallest effective sample size over t is >= 2 and the new path
    leaves the reference particle at more than 10 % of the steps; (c) the tightened inputs: at one step or more every weight shifted by the exact bound is zero
    in fp32 and in fp64, so the sweep's fallback to the exact maximum is reached in both precisions.  Measured over the list: smallest gap 1.3e-8 (range,
    N = 1000); smallest ESS 2.5 (the tightened growth inputs, 3.2 otherwise); the new path leaves the reference particle at 42 % of the steps or more; the
    tightened cases underflow in fp32 at 19 (range) and 13 (growth) of 22 steps, in fp64 at 3 and 2 of them."""
    w = M.wellposedness(case)
    print(case.id, w)
    assert w["gap"] >= 1e-8
    if case.N >= 64:
        assert w["ess"] >= 2 and w["moved"] > 0.1
    if case.spec.T > 2 and case.gradient != "exact":
        assert w["bound_excess"] <= 1e-9    # the exact bound is one (the exact-gradient correction is unbounded: the sweep uses no bound there)
    if case.spec.tight:
        assert w["underflow32"] >= 1 and w["underflow64"] >= 1


_TIGHT = [c for c in M.cases("bound") if c.spec.tight and c.spec.bound == "exact"]   # (the four bounds share their inputs and their literal)


@pytest.mark.parametrize("case", _TIGHT, ids=[c.id for c in _TIGHT])
def test_fp32_chains_of_the_tightened_inputs_underflow(case):
    """the four chains of the GPU file's fp32 bound test (teacher-forced, so no boundary condition): each reaches the fallback"""
    for c in M.fp32_bound_chains(case):
        assert M.wellposedness(c)["underflow32"] >= 1


# ---- fp32 resampling by NumPy itself -----------------------------------------------------------------------------------------------------------------------
_FP32_CHAINS = [(s.name, M.fp32_chains(s)) for s in M.FP32_SPECS]


@pytest.mark.parametrize("chains", [c for _, c in _FP32_CHAINS], ids=[n for n, _ in _FP32_CHAINS])
def test_numpy_fp32_resampling_stays_under_the_tie_rate_cap(chains):
    """the cap the GPU tests apply to the device (2e-4 of the resampling draws may land on another particle than the literal fp32 order picks) is a condition
    NumPy's own fp32 arithmetic meets on the inputs of the N = 1024 fp32 sweeps: normalise -> cumsum -> searchsorted in fp32 against the same in fp64, on the
    literal sweeps' log-weights.  Measured: range 28, lorenz 27 of 241 428 draws differ (1.2e-4, 1.1e-4).  (Not a condition on the tightened bound inputs, whose
    log-weights reach -2e3: storing those in fp32 alone moves 6 of 23 460 draws against fp64.  The GPU file compares them, like these, with the fp32 order
    redone from the device's own stored fp32 log-weights, never with fp64 ancestors.)"""
    miss = total = 0
    for case in chains:
        _, _, h = M.literal_sweep(case)
        _, _, nz = M.inputs(case)
        for t in range(case.spec.T - 1):
            a64 = L.multinomial(nz["u_res"][t], L.normalize(h["log_ws"][t]))
            a32 = L.multinomial(nz["u_res"][t].astype(np.float32), L.normalize(h["log_ws"][t].astype(np.float32)))
            miss += int(np.sum(a64 != a32))
            total += case.N - 1
    print(chains[0].spec.name, miss, total)
    assert miss / total <= 2e-4, (miss, total)
