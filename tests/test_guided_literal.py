"""The literal guided sampler (tests/guided_np.py on oracle/csmc_np.py::get_generic_kernel), checked against itself before the HIP kernels are checked
against it (tests/test_gpu_guided.py).  CPU only.

* Closed form: without gradient the guided weight is log g_t(x) + log N(u_t; pred, P + s_t^2 I) -- an identity with no K or Lambda in it.
* Stability: the sweep with tables built by solve + cholesky and by the eigen-decomposition of P picks identical ancestors and backward indices on every
  case of the GPU test, and its outputs differ by rounding only.  That difference is the rounding floor of the problem (printed): the GPU bars
  (1e-12 on particles, 1e-10 on log-weights) sit more than a hundred times above it.
* Every limit of csmc.get_guided_kernel raises NotImplementedError naming it (no GPU needed: the description is refused before anything is launched)."""
import numpy as np
import numpy.testing as npt
import pytest

from oracle import csmc_np as L
from tests import guided_np as G


@pytest.mark.parametrize("d", [1, 3, 30])
def test_guided_weight_without_gradient_is_the_closed_form(d):
    rng = np.random.default_rng(5 + d)
    T, N = 6, 40
    _, m, xtrue, delta = G.sv_case(d, T, rng)
    scale = np.sqrt(0.5 * delta)
    u = xtrue + scale[:, None] * rng.standard_normal((T, d))
    m0, g0, mt, gt = G.factory(m)(u, scale)
    worst = 0.0
    for t in range(T):
        x, xp = xtrue[t] + rng.standard_normal((N, d)), xtrue[max(t - 1, 0)] + rng.standard_normal((N, d))
        got = g0(x) if t == 0 else gt(x, xp, L._tree_index(gt.params, t - 1))
        want = G.closed_form(m, t, x, xp, u[t], scale[t])
        worst = max(worst, float(np.max(np.abs(got - want))))
    print(f"d = {d}: max |guided weight - closed form| = {worst:.1e}")
    assert worst < (1e-12 if d < 30 else 1e-11)  # (measured 6e-15 at d = 1, 2e-13 at d = 30: sums of d terms of magnitude ~ 10 d in fp64)


_floor = {"xs": 0.0, "log_ws": 0.0}


@pytest.mark.parametrize("backward", [False, True])
@pytest.mark.parametrize("gradient", [False, True])
@pytest.mark.parametrize("d,N,T", G.CASES)
def test_literal_sweep_is_stable_under_the_route_to_its_tables(d, N, T, gradient, backward):
    rng = np.random.default_rng(1000 * d + 10 * gradient + backward)
    _, m, xtrue, delta = G.sv_case(d, T, rng)
    x0 = xtrue + 0.3 * rng.standard_normal((T, d))
    nz = L.Noise(**G.noise(T, N, d, rng))
    out = [G.get_kernel(m, N, backward, gradient, how)[1](nz, x0, delta) for how in ("solve", "eig")]
    (xa, Ba, ha), (xb, Bb, hb) = out
    npt.assert_array_equal(ha["As"], hb["As"])
    npt.assert_array_equal(Ba, Bb)
    ex, el = float(np.max(np.abs(ha["xs"] - hb["xs"]))), float(np.max(np.abs(ha["log_ws"] - hb["log_ws"])))
    _floor["xs"], _floor["log_ws"] = max(_floor["xs"], ex), max(_floor["log_ws"], el)
    print(f"d={d} N={N} T={T} gradient={gradient} backward={backward}: xs {ex:.1e} log_ws {el:.1e}; floor so far xs {_floor['xs']:.1e} log_ws {_floor['log_ws']:.1e}; "
          f"updated {int((Ba != 0).sum())} of {T}")
    assert ex <= 1e-13 and el <= 1e-11  # (measured 7e-15 and 1.5e-13; a tenth of the GPU test's bars at the very most)
    npt.assert_allclose(xa, xb, rtol=0, atol=1e-13)
    assert np.all(ha["As"][:, 0] == 0) and np.array_equal(ha["xs"][:, 0], x0)


def test_python_refusals_name_their_limit():
    from aux_ssm_samplers_amd.csmc import (get_guided_kernel, get_generic_kernel, GaussianInit, LinearGaussianDynamics, FlatPotential, DevicePotential,
                                           DeviceGaussianDynamics, device_models as U)
    from aux_ssm_samplers_amd.csmc.guided import GuidedFactory
    T, d = 5, 1
    M0, Mt, G = GaussianInit(m0=[0.0], P0=[[1.0]]), LinearGaussianDynamics(F=[[0.9]], b=[0.0], Q=[[0.5]]), FlatPotential()
    with pytest.raises(NotImplementedError, match="user-defined models"):
        get_guided_kernel(M0, DevicePotential(U.BUILTIN_SV, y=np.zeros(1)), Mt, DevicePotential(U.BUILTIN_SV, params=np.zeros((T - 1, 1))), 8)
    with pytest.raises(NotImplementedError, match="user-defined models"):
        get_guided_kernel(M0, G, DeviceGaussianDynamics(U.BUILTIN_LINEAR_MEAN, Q=[[0.5]], theta=[0.9, 0.0]), G, 8)
    Mtv = LinearGaussianDynamics(F=np.full((T - 1, 1, 1), 0.9), b=np.zeros((T - 1, 1)), Q=np.full((T - 1, 1, 1), 0.5))
    with pytest.raises(NotImplementedError, match="time-invariant transitions"):
        get_guided_kernel(M0, G, Mtv, G, 8)
    with pytest.raises(NotImplementedError, match="Pt must be the model dynamics Mt"):
        get_guided_kernel(M0, G, Mt, G, 8, backward=True, Pt=LinearGaussianDynamics(F=[[0.9]], b=[0.0], Q=[[0.5]]))
    with pytest.raises(NotImplementedError, match="exact"):
        get_guided_kernel(M0, G, Mt, G, 8, gradient="exact")
    with pytest.raises(NotImplementedError, match="parallel"):
        get_guided_kernel(M0, G, Mt, G, 8, parallel=True)
    init, kern = get_generic_kernel(GuidedFactory(M0, G, Mt, G, Mt), 8, backward=True, Pt=Mt)  # the generic entry accepts the descriptor
    assert init(np.zeros((T, d))).x.shape == (T, d)
    from aux_samplers.csmc.guided import get_kernel as through_the_shim
    assert through_the_shim is get_guided_kernel
