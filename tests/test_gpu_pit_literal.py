"""The parallel-in-time cSMC sweep ON THE GPU (auxssm_csmc_pit_sweep through `_device.pit_sweep`, csrc/pit.hip) next to `oracle/pit_np.py`, the LITERAL NumPy
restatement of the reference's tree (padding to 2^K, whole-block gathers, passthrough of padded right children, normalised weights, plain cumsum,
`searchsorted`), with no contract oracle in between: the kernels keep boundary leaf indices and slot pairs and walk them down from the root, the literal
does what the reference does.  fp64 on identical explicit noise: `anc` identical to the literal's origins, `x` within rtol = atol = 1e-12
(the bar of tests/test_oracle_csmc_literal.py / tests/test_gpu_csmc_literal.py for the same comparison of the sequential sweep).

1. The closed family: the cells and seeds of tests/test_oracle_pit_literal.py (tests/pit_cases.py) -- every N class of the stitch, passthrough trees, gradient
   proposals, time-varying transitions, the Lorenz-63 transition, a whole missing step on the top-level stitch boundary.
2. The multivariate Student-t potential, which csmc_ref.c does not restate (the literal is its only oracle): d in {1, 3, 4}, N in {32, 33, 100}, T in {9, 25, 33},
   nu = 4 and 1, a dense non-diagonal precision matrix, flat steps (NaN in y_t) at t = 0, on the top-level stitch boundary and at the last step, gradient off / on.
3. Three chains in one launch, each with its own reference trajectory and noise, each against its own literal run (chain strides of the tree workspace).
   The step sizes are per time step and shared by the chains: the entry point takes one sqrt_half_delta (T) per launch.
4. The keyed path: `pit_sweep(key=...)` against the literal on the arrays `rng_normal` / `rng_uniform` fill from that key at streams 1, 2, 3 -- the
   stream-to-array map of the keyed sweep tied to the reference's key tree (oracle/pit_np.py, "PRNG").

Every case first asserts the margin condition of tests/test_oracle_pit_literal.py ("Ties") on the literal: smallest draw margin >= 2 N^2 eps, so an index
mismatch is a defect, never a tie.  fp32 stays with the bit-exact tests against the contract oracle (tests/test_gpu_pit.py): the kernel exposes no per-stitch
state to teacher-force a tie rate from."""
import numpy as np
import numpy.testing as npt
import pytest

from tests import pit_cases as PC

pytestmark = pytest.mark.gpu


def _check(c, literal, x, anc, what):
    xl, origins, hist = literal
    threshold = PC.margin_threshold(c.N)
    err = float(np.max(np.abs(x - xl)))
    print(f"{what}: smallest draw margin {hist['min_margin']:.2e} (threshold {threshold:.2e}); device: {int((anc != origins).sum())} of {c.T} origins differ, "
          f"max |x - literal| = {err:.1e}, {int((origins != 0).sum())} steps updated")
    assert hist["min_margin"] >= threshold
    npt.assert_array_equal(anc, origins)
    npt.assert_allclose(x, xl, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("cell", PC.CELLS, ids=PC.cell_id)
def test_hip_pit_sweep_fp64_equals_the_literal_tree(cell):
    from aux_ssm_samplers_amd.csmc import _device
    c = PC.case(cell)
    x, anc = _device.pit_sweep(c.device_model(), c.x0, c.N, noise={k: v[None] for k, v in c.noise.items()}, delta=c.delta)
    assert x.dtype == np.float64
    _check(c, PC.literal(cell), x, anc, PC.cell_id(cell))


@pytest.mark.parametrize("cell", PC.MVT_CELLS, ids=PC.mvt_cell_id)
def test_hip_pit_sweep_student_t_fp64_equals_the_literal_tree(cell):
    from aux_ssm_samplers_amd.csmc import _device
    c = PC.mvt_case(cell)
    fk = c.device_model()
    assert fk.potential == 4 and fk.user is None and np.all(np.isnan(c.m.y[[0, PC.top_boundary(c.T), c.T - 1]]).any(axis=1))
    x, anc = _device.pit_sweep(fk, c.x0, c.N, noise={k: v[None] for k, v in c.noise.items()}, delta=c.delta)
    _check(c, PC.mvt_literal(cell), x, anc, PC.mvt_cell_id(cell))
    assert (anc != 0).any()


@pytest.mark.parametrize("kind,cell,seed", PC.CHAIN_CELLS, ids=[k for k, _, _ in PC.CHAIN_CELLS])
def test_three_chains_in_one_launch_each_equal_their_own_literal(kind, cell, seed):
    from aux_ssm_samplers_amd.csmc import _device
    c = PC.any_case(kind, cell)
    x0, noise = c.chains(3, seed)
    x, anc = _device.pit_sweep(c.device_model(), x0, c.N, noise=noise, delta=c.delta)
    assert x.shape == x0.shape and anc.shape == x0.shape[:2]
    for k in range(3):
        _check(c, c.literal_sweep({n: v[k] for n, v in noise.items()}, x0[k]), x[k], anc[k], f"{kind} chain {k}")
    assert not np.array_equal(anc[0], anc[1]) and not np.array_equal(anc[1], anc[2])


@pytest.mark.parametrize("kind,cell,seed", PC.KEYED_CELLS, ids=[k for k, _, _ in PC.KEYED_CELLS])
def test_keyed_sweep_equals_the_literal_on_the_arrays_of_its_streams(kind, cell, seed):
    from aux_ssm_samplers_amd import _lib, random as R
    from aux_ssm_samplers_amd.csmc import _device
    c = PC.any_case(kind, cell)
    h, key = _lib.default_handle(), R.PRNGKey(seed)
    x0, _ = c.chains(3, seed)
    noise = PC.keyed_noise(lambda s, shp: h.rng_normal(key, s, shp, np.float64).to_host(), lambda s, shp: h.rng_uniform(key, s, shp, np.float64).to_host(),
                           3, c.T, c.N, c.d)
    x, anc = _device.pit_sweep(c.device_model(), x0, c.N, key=key, delta=c.delta)
    for k in range(3):
        _check(c, c.literal_sweep({n: v[k] for n, v in noise.items()}, x0[k]), x[k], anc[k], f"{kind} keyed chain {k}")
