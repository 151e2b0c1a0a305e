"""Auxiliary particle Gibbs with guided (locally optimal) proposals: the proposal of x_t is conditioned on the auxiliary variable u_t AND on the
parent particle (reference: the `csmc-guided` sampler style of the examples, examples/stochastic_volatility/auxiliary_guided_csmc.py on
aux_samplers/csmc/generic.py).

get_kernel(M0, G0, Mt, Gt, N, backward=False, Pt=None, gradient=False) -> (init, kernel); kernel(key, state, delta) -> CSMCState, on host states
and on resident `CsmcChains`.

With s_t = sqrt(delta_t / 2), u_t = x*_t + s_t eps, pred = m0 (P = P0) at t = 0 and the transition mean of the parent (P = Q) after:
    K_t = P (P + s_t^2 I)^-1,  Lambda_t = P - K_t P,  x_t ~ N(pred + K_t (u~_t - pred), Lambda_t),
    log w = log g_t(x) + log N(x; pred, P) + sum_k log N(x_k; u_{t,k}, s_t^2) - log N(x; pred + K_t (u~_t - pred), Lambda_t)
u~ = u, or with gradient=True u + s_t^2 grad log g_t(u_t): the gradient of the potential alone, not of the joint density the independent
kernel's gradient=True differentiates.  The tables K_t, chol Lambda_t are built on the device at every sweep (csrc/csmc_sweep.h::k_csmc_gtab).

Limits, each raising NotImplementedError: the closed model family only (no DevicePotential / DeviceGaussianDynamics), time-invariant
transitions, Pt = Mt, gradient False or True (no "exact"), the sequential sweep (no parallel=True: the reference has no parallel guided sampler)."""
from . import _device
from .generic import get_kernel as get_base_kernel


class GuidedFactory:
    """The factory of the reference's guided samplers in device-describable form (like generic.IndependentFactory)."""

    def __init__(self, M0, G0, Mt, Gt, Pt, gradient=False):
        from .. import _lib
        if gradient not in (False, True, 0, 1, "reference"):
            raise NotImplementedError('guided proposals take gradient=False or True (the potential\'s gradient at u, as the reference has it): '
                                      f"gradient={gradient!r} is a weighting of the independent proposals")
        self.fk = _device.describe_guided(M0, G0, Mt, Gt, Pt, _lib.GRAD_REFERENCE if gradient else _lib.GRAD_NONE)

    def __call__(self, u, scale):
        raise NotImplementedError("the auxiliary model is evaluated inside the HIP kernel; this factory is a descriptor")


def get_kernel(M0, G0, Mt, Gt, N, backward=False, Pt=None, gradient=False, parallel=False):
    if parallel:
        raise NotImplementedError("guided proposals depend on the parent particle, so they run the sequential sweep only: there is no parallel-in-time "
                                  "guided sampler (parallel=True)")
    if backward and Pt is None:
        Pt = Mt
    return get_base_kernel(GuidedFactory(M0, G0, Mt, Gt, Pt, gradient), N, backward, Pt)
