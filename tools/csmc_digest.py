#!/usr/bin/env python3
"""One SHA-256 per case over the bytes of (x, ancestors, xs, log_ws, As) of one conditional-SMC sweep with its history, for a fixed list of small problems: every
built-in potential kind on every path a cSMC driver can take (csrc/csmc.hip: the register kernels, dx <= 4; csrc/csmc_wide.hip: the wide-state kernels, with few chains and with more chains than the device has CUs -- the two sides of
csmc_wide.hip::run_cw's choice between sixteen and eight waves per chain in fp32; csrc/pit.hip: the parallel-in-time sweep), every proposal style and gradient mode, with and without backward sampling, in both dtypes, once on explicit noise arrays and once on
Threefry keys.  For comparing two builds of the library bit for bit:   AUXSSM_LIB=/path/to/libauxssm.so python tools/csmc_digest.py out.json   once per build, then
compare the files.  A case that raises is recorded with the error's text."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aux_ssm_samplers_amd import _lib, random as R  # noqa: E402
from aux_ssm_samplers_amd.csmc import _device, FlatPotential, MaskedGaussianObsPotential  # noqa: E402
from tests import guided_np as G, lingauss_np as LG, mvt_np as MV  # noqa: E402

KINDS = ("flat", "gauss", "masked", "sv", "mvt", "lingauss")
NAN_ROWS = (0, 2)  # time steps with a NaN observation component (not the flat potential, not the SV cases)
# (style, gradient): the describe_* call and its gradient mode
STYLES = [("bootstrap", _lib.GRAD_NONE), ("independent", _lib.GRAD_NONE), ("independent", _lib.GRAD_REFERENCE), ("independent", _lib.GRAD_EXACT),
          ("guided", _lib.GRAD_NONE), ("guided", _lib.GRAD_REFERENCE)]
# (name, dx, N, T, kinds): the register path at dx = 2 and 4; its sixteen-wave instantiations (and, with in-pass draws, config C3's shape); the wide path with a
# partial slot and at its widest state
SHAPES = [("reg2", 2, 20, 5, KINDS), ("reg4", 4, 20, 5, KINDS), ("reg1_n1024", 1, 1024, 4, ("sv",)), ("wide5", 5, 7, 5, KINDS), ("wide32", 32, 64, 5, KINDS)]
CHAINS = 2
# more chains than CUs on the wide path (fp32: the eight-wave kernels; the count is CUs + 3, so the digests belong to one device model): (style, gradient, backward, noise)
MANY_SHAPE = ("wide30_more_chains_than_cus", 30, 25, 4)
MANY_STYLES = [("bootstrap", _lib.GRAD_NONE, False, "explicit"), ("independent", _lib.GRAD_NONE, True, "keyed"), ("independent", _lib.GRAD_EXACT, True, "explicit"),
               ("guided", _lib.GRAD_REFERENCE, True, "explicit")]


def many_chains():
    """CUs + 3: the library compares the chain count with hipDeviceProp_t::multiProcessorCount of the handle's device (read by torch in a child process: torch
    ships a HIP runtime of its own, which stays out of this process)"""
    code = f"import torch; print(torch.cuda.get_device_properties({_lib.default_handle().device}).multi_processor_count)"
    return int(subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, check=True).stdout.split()[-1]) + 3


def model(kind, d, T):
    """(device objects (M0, G0, Mt, Gt), a trajectory (T, d), delta (T,)) of one potential kind"""
    rng = np.random.default_rng(1000 * d + KINDS.index(kind))
    if kind == "mvt":
        dev, _, x, delta = MV.case(d, T, rng, nan_rows=NAN_ROWS)
    elif kind == "lingauss":
        dev, _, x, delta = LG.case(d, max(d - 1, 1), T, rng, nan_rows=NAN_ROWS)  # (dy < dx wherever dx > 1)
    elif kind == "sv":
        dev, _, x, delta = G.sv_case(d, T, rng)
    else:
        (M0, G0, Mt, Gt), _, x, delta = G.sv_case(d, T, rng, potential="gauss")
        y = np.concatenate([np.reshape(G0.y, (1, d)), np.reshape(Gt.params, (-1, d))])
        for i, t in enumerate(NAN_ROWS):
            y[t, i % d] = np.nan
        if kind == "flat":
            G0, Gt = FlatPotential(), FlatPotential()
        elif kind == "masked":
            G0, Gt = MaskedGaussianObsPotential(sig=G0.sig, y=y[0]), MaskedGaussianObsPotential(sig=Gt.sig, params=y[1:])
        else:
            G0, Gt = type(G0)(sig=G0.sig, y=y[0]), type(Gt)(sig=Gt.sig, params=y[1:])
        dev, delta = (M0, G0, Mt, Gt), delta / d
    return dev, x, delta


def describe(style, gradient, dev, parallel=False):
    M0, G0, Mt, Gt = dev
    if style == "bootstrap":
        return _device.describe_bootstrap(M0, G0, Mt, Gt, Mt)
    if style == "guided":
        return _device.describe_guided(M0, G0, Mt, Gt, Mt, gradient)
    return _device.describe_independent(M0, G0, Mt, Gt, Mt, gradient, parallel)


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def start(x, dtype, chains=CHAINS):
    return np.stack([x + 0.1 * (c % 7) + 0.01 * (c // 7) for c in range(chains)]).astype(dtype)


def noise_kw(how, T, N, d, seed, chains=CHAINS):
    """the sweep's noise: explicit arrays of `chains` chains, or a Threefry key"""
    if how == "keyed":
        return dict(key=R.PRNGKey(seed))
    per = [G.noise(T, N, d, np.random.default_rng(seed + c)) for c in range(chains)]
    return dict(noise={k: np.stack([p[k] for p in per]) for k in per[0]})


def sweep_digest(fk, x, delta, N, backward, dtype, how, chains=CHAINS):
    T, d = x.shape
    xo, anc, hist = _device.sweep(fk, start(x, dtype, chains), N, backward, delta=delta, want_history=True, **noise_kw(how, T, N, d, 77, chains))
    return sha(xo, anc, hist["xs"], hist["log_ws"], hist["As"])


def pit_digest(fk, x, delta, N, dtype, how):
    T, d = x.shape
    kw = noise_kw(how, T, N, d, 78)
    if how == "explicit":  # (the parallel-in-time sweep draws one uniform per time step and particle, T rows, and has no backward pass of its own)
        rng = np.random.default_rng(79)
        kw["noise"] = dict(eps_aux=kw["noise"]["eps_aux"], eps_prop=kw["noise"]["eps_prop"], u_res=rng.random((CHAINS, T, N)))
    xo, anc = _device.pit_sweep(fk, start(x, dtype), N, delta=delta, **kw)
    return sha(xo, anc)


def cases():
    """(name, thunk) of every case"""
    for dtype in (np.float32, np.float64):
        dn = np.dtype(dtype).name
        for shape, d, N, T, kinds in SHAPES:
            for kind in kinds:
                dev, x, delta = model(kind, d, T)
                for style, gradient in STYLES:
                    for backward in (False, True):
                        for how in ("explicit", "keyed"):
                            yield (f"{shape}:{kind}:{style}:grad{gradient}:bw{int(backward)}:{dn}:{how}",
                                   lambda a=(style, gradient, dev, x, delta, N, backward, dtype, how): sweep_digest(describe(*a[:3]), *a[3:]))
        if dtype == np.float32:  # (fp64 runs eight waves at every chain count: the cases above)
            shape, d, N, T = MANY_SHAPE
            Cn = many_chains()
            for kind in KINDS:
                dev, x, delta = model(kind, d, T)
                for style, gradient, backward, how in MANY_STYLES:
                    yield (f"{shape}:C{Cn}:{kind}:{style}:grad{gradient}:bw{int(backward)}:{dn}:{how}",
                           lambda a=(style, gradient, dev, x, delta, N, backward, dtype, how, Cn): sweep_digest(describe(*a[:3]), *a[3:]))
        # config C3's shape (csrc/csmc.hip::c3_shape) runs with the draws made inside the forward pass
        dev, x, delta = model("sv", 1, 4)

        def c3(dev=dev, x=x, delta=delta, dtype=dtype):
            os.environ["AUXSSM_CSMC_NO_PREGEN"] = "1"
            try:
                return sweep_digest(describe("independent", _lib.GRAD_NONE, dev), x, delta, 1024, True, dtype, "keyed")
            finally:
                del os.environ["AUXSSM_CSMC_NO_PREGEN"]
        yield f"reg1_n1024:sv:independent:grad0:bw1:{dn}:keyed_in_pass_draws", c3
        for kind in ("gauss", "mvt", "lingauss"):
            dev, x, delta = model(kind, 2, 8)
            for gradient in (_lib.GRAD_NONE, _lib.GRAD_REFERENCE):
                for how in ("explicit", "keyed"):
                    yield (f"pit2:{kind}:grad{gradient}:{dn}:{how}",
                           lambda a=(gradient, dev, x, delta, dtype, how): pit_digest(describe("independent", a[0], a[1], True), a[2], a[3], 8, a[4], a[5]))


if __name__ == "__main__":
    out = {}
    for name, run in cases():
        try:
            out[name] = run()
        except Exception as e:  # noqa: BLE001 -- part of the record: both builds must fail alike
            out[name] = f"{type(e).__name__}: {e}"
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    bad = [k for k, v in out.items() if len(v) != 64]
    print(f"{len(out)} cases ({len(bad)} raised) -> {sys.argv[1]}")
    for k in bad[:20]:
        print(" ", k, out[k])
