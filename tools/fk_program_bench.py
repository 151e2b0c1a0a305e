"""User-defined Feynman-Kac models (csrc/fk_program.hip): what compiling costs and what the compiled sweep runs at.

  compile   hipRTC time of one program (the sweep's seven kernels), f32 / f64 x dx = 1 / 4, a potential + mean source; no device needed
  sweep     C3's shape (SV d = 1, N = 1024, fp32, 256 chains, independent auxiliary proposals, backward sampling, Threefry noise) in sweeps/s:
              builtin        the closed family -- C3's special SP = 1 instantiation of k_csmc_fwd (csmc.hip::fwd_kernel, c3_shape)
              builtin_trace  the closed family with the ancestor trace stored (As_out), which the SP = 1 path excludes: the generic NW = 16 kernel
              user           the same potential and bound as user source (csmc/device_models.py::BUILTIN_SV): the program's NW = 16 kernel
              user_trace     the same with the ancestor trace stored (like for like with builtin_trace)
  gradient  hipRTC time of one gradient program (AUXSSM_FK_USER_GRADIENT: 11 kernels), then C3's shape with gradient="exact" in sweeps/s:
              builtin        the closed family's gradient sweep (k_csmc_grad + the generic GRAD = true NW = 16 forward kernel)
              user           the same model as user source with its derivative (csmc/device_models.py::BUILTIN_SV_GRAD): the program's kernels
Prints one JSON line per measurement.  Usage: python tools/fk_program_bench.py [compile] [sweep] [gradient] [--T 65536] [--steps 3] [--warmup 1]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from aux_ssm_samplers_amd import _lib, random as R  # noqa: E402
from aux_ssm_samplers_amd.csmc import _device  # noqa: E402
from aux_ssm_samplers_amd.csmc import device_models as U  # noqa: E402


def compile_times(reps=3, gradient=False):
    src = U.BUILTIN_SV_GRAD + U.BUILTIN_LINEAR_MEAN_VJP if gradient else U.BUILTIN_SV + U.BUILTIN_LINEAR_MEAN
    flags = _lib.FK_USER_POTENTIAL | _lib.FK_USER_MEAN | (_lib.FK_USER_GRADIENT if gradient else 0)
    what = "hipRTC compile, one gradient program (11 kernels)" if gradient else "hipRTC compile, one program (7 kernels)"
    for dt in (np.float32, np.float64):
        for dx in (1, 4):
            ts = []
            for r in range(reps):
                t0 = time.perf_counter()
                _device.compile_program(src + f"\n// rep {r}\n", dt, dx, flags)  # (a new source: no cache hit)
                ts.append(time.perf_counter() - t0)
            print(json.dumps(dict(measure=what, dtype=np.dtype(dt).name, dx=dx, seconds_min=round(min(ts), 3),
                                  seconds_median=round(float(np.median(ts)), 3), reps=reps)), flush=True)


def sweep_rates(T, N, Cn, steps, warmup, gradient=False):
    from aux_ssm_samplers_amd.csmc import GaussianInit, LinearGaussianDynamics, SVPotential, DevicePotential
    h = _lib.default_handle()
    phi, q = 0.9, 2.0 / (1.0 - 0.9 ** 2)
    rng = np.random.default_rng(0)
    x = np.zeros((T, 1))
    for t in range(1, T):
        x[t] = phi * x[t - 1] + np.sqrt(q) * rng.standard_normal(1)
    y = np.exp(0.5 * x) * rng.standard_normal((T, 1))
    M0, Mt = GaussianInit(m0=[0.0], P0=[[q]]), LinearGaussianDynamics(F=[[phi]], b=[0.0], Q=[[q]])
    gmode, src = (_lib.GRAD_EXACT, U.BUILTIN_SV_GRAD) if gradient else (_lib.GRAD_NONE, U.BUILTIN_SV)
    fks = dict(builtin=_device.describe_independent(M0, SVPotential(y=y[0]), Mt, SVPotential(params=y[1:]), Mt, gmode),
               user=_device.describe_independent(M0, DevicePotential(src, y=y[0]), Mt, DevicePotential(src, params=y[1:]), Mt, gmode))
    dtype = np.float32
    x0 = (x[None] + 0.1 * rng.standard_normal((Cn, T, 1))).astype(dtype)
    shd = h.to_device(np.full(T, 0.5), dtype)
    As = h.zeros((Cn, T - 1, N), np.int32)
    keys = R.split(R.PRNGKey(77), steps + warmup)
    out = {}
    measure = "C3 shape sweep, gradient=exact" if gradient else "C3 shape sweep"
    for name in ("builtin", "user") if gradient else ("builtin", "builtin_trace", "user", "user_trace"):
        fk = fks[name.split("_")[0]]
        trace = name.endswith("trace")
        xd = h.to_device(x0)
        anc = h.zeros((Cn, T), np.int32)
        m = fk.struct(h, dtype, T)

        def step(k):
            nz = _lib.CsmcNoise()
            nz.mode, nz.key0, nz.key1 = _lib.NOISE_THREEFRY, int(keys[k][0]), int(keys[k][1])
            _device._csmc_call(h, fk, dtype, m, Cn, T, N, True, shd, xd, nz, anc, None, None, As if trace else None)

        for k in range(warmup):
            step(k)
        h.sync()
        t0 = time.perf_counter()
        for k in range(warmup, warmup + steps):
            step(k)
        h.sync()
        el = time.perf_counter() - t0
        out[name] = xd.to_host()
        print(json.dumps(dict(measure=measure, path=name, T=T, N=N, chains=Cn, dtype="f32", steps=steps, sweeps_per_s=round(Cn * steps / el, 2),
                              ms_per_sweep=round(el / steps * 1e3, 2), updated_fraction=round(float((anc.to_host() != 0).mean()), 4))), flush=True)
    same = all(np.array_equal(out[k], out["user" + k[7:]]) for k in out if k.startswith("builtin"))
    print(json.dumps(dict(measure=measure, user_equals_builtin_bitwise=bool(same))), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["compile", "sweep"])
    ap.add_argument("--T", type=int, default=65536)
    ap.add_argument("--N", type=int, default=1024)
    ap.add_argument("--chains", type=int, default=256)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    if "compile" in a.what:
        compile_times()
    if "sweep" in a.what:
        sweep_rates(a.T, a.N, a.chains, a.steps, a.warmup)
    if "gradient" in a.what:
        compile_times(gradient=True)
        sweep_rates(a.T, a.N, a.chains, a.steps, a.warmup, gradient=True)
