"""The cells that tests/test_oracle_pit_literal.py (contract oracle, CPU) and tests/test_gpu_pit_literal.py (HIP kernels) share: one model of the closed
family per cell, written three times -- the dict oracle/csmc.py takes, the protocol objects of oracle/csmc_np.py, the device objects of
aux_ssm_samplers_amd.csmc -- with its explicit noise, and the literal parallel-in-time sweep (oracle/pit_np.py) of it, computed once per process.
Test infrastructure only.

A cell is (d, N, T, potential, gradient, tv, seed); d = "lorenz" is the Euler-Maruyama Lorenz-63 transition at d = 3.  The sizes are the smallest at which
each thing can go wrong:  N over the three chunk classes of csrc/pit.hip (N <= 32: 64 chunks, N <= 128: 256, above: 1024), with ragged and empty chunks and
sub-chunks (2, 16, 32, 33, 100, 128, 129, 256; 1024 at T = 2, the root draw alone, and T = 3);  T = 2 (root only), 3 and 5 (passthrough nodes), 8 (a full
tree), 9 (one leaf beyond a power of two: almost every upper node passes through), 33 and 37.  The masked potential has, besides scattered missing
components, one WHOLE missing step on the stitch boundary of the top level (t = 2^(K-1)).  Every value of N, T, d and the potential appears with gradient
proposals off and on and with time-varying transitions off and on (test_cells_cover_every_value_with_gradient_and_time_varying_off_and_on).

The seed of a cell is the smallest of 0..31 at which the literal's smallest draw margin is >= 2 N^2 eps (tests/test_oracle_pit_literal.py, "Ties"); it was found
on the CPU by running exactly `literal(cell)` and is asserted again by every test."""
import functools

import numpy as np

from oracle import csmc as O
from oracle import csmc_np as L
from oracle import pit_np as P
from tests import guided_np as G

EPS = float(np.finfo(np.float64).eps)
FLAT, GAUSS, SV, MASKED = O.POT_FLAT, O.POT_GAUSS_OBS, O.POT_SV, O.POT_GAUSS_OBS_MASKED
SIG_Y = 0.7

#        d         N     T   potential gradient tv seed
CELLS = [
    (1,        2,    2,  FLAT,   0, 1, 0),
    (2,        2,    9,  GAUSS,  1, 0, 0),
    (2,        16,   3,  SV,     0, 1, 0),
    (3,        16,   33, MASKED, 1, 0, 0),
    (3,        32,   5,  GAUSS,  0, 1, 0),
    (4,        32,   37, FLAT,   1, 0, 0),
    (4,        33,   8,  MASKED, 0, 1, 0),
    (1,        33,   2,  SV,     1, 0, 0),
    (1,        100,  9,  SV,     0, 0, 0),
    (2,        100,  3,  MASKED, 1, 1, 0),
    (2,        128,  33, FLAT,   0, 0, 0),
    (3,        128,  5,  GAUSS,  1, 1, 0),
    (3,        129,  37, MASKED, 0, 0, 0),
    (4,        129,  8,  SV,     1, 1, 0),
    (4,        256,  2,  GAUSS,  0, 0, 0),
    (1,        256,  9,  FLAT,   1, 1, 0),
    (1,        1024, 2,  GAUSS,  0, 1, 0),
    (1,        1024, 3,  SV,     1, 0, 0),
    (2,        1024, 2,  SV,     1, 0, 0),
    (1,        1024, 3,  GAUSS,  0, 1, 3),
    ("lorenz", 100,  9,  MASKED, 0, 0, 0),
    ("lorenz", 33,   5,  GAUSS,  1, 0, 0),
    ("lorenz", 32,   33, MASKED, 1, 0, 0),
    ("lorenz", 128,  8,  GAUSS,  0, 0, 0),
    (1,        33,   33, GAUSS,  0, 1, 0),
    (2,        100,  37, SV,     1, 1, 0),
    (1,        16,   37, MASKED, 0, 1, 0),
    (3,        2,    37, SV,     0, 0, 0),
    (2,        256,  33, MASKED, 1, 0, 0),
    (1,        129,  3,  FLAT,   0, 1, 0),
    (4,        128,  9,  MASKED, 1, 1, 0),
    (2,        32,   8,  SV,     1, 1, 0),
    (4,        16,   5,  GAUSS,  1, 0, 0),
    (3,        100,  8,  FLAT,   0, 1, 0),
    (3,        33,   9,  FLAT,   1, 1, 0),
    (3,        256,  5,  SV,     0, 1, 0),
    (2,        129,  9,  GAUSS,  1, 0, 0),
    (4,        2,    3,  MASKED, 1, 1, 0),
    (1,        2,    5,  GAUSS,  0, 0, 0),
    (3,        16,   2,  FLAT,   1, 1, 0),
]

_POT_NAME = {FLAT: "flat", GAUSS: "gauss", SV: "sv", MASKED: "masked"}


def cell_id(cell):
    d, N, T, pot, gradient, tv, seed = cell
    return f"d{d}-N{N}-T{T}-{_POT_NAME[pot]}-g{gradient}-tv{tv}-s{seed}"


def margin_threshold(N):
    """2 N^2 eps: N^2 eps bounds the difference between any two orders of summing N^2 non-negative terms of total 1; the factor 2 covers the per-term
    rounding of exp and of the normalisation"""
    return 2.0 * N * N * EPS


def top_boundary(T):
    """the time step on the right of the root's stitch: 2^(K-1), 2^K the padded length"""
    return P.next_power_of_2(T) // 2


LORENZ_CENTRE = np.array([1.5, -1.5, 25.0])


class _Sides:
    """what the tests need of a case, whatever its model: N, T, d, gradient, x0 (T, d), delta (T,), noise; literal_objects(), joint_grad(u), device_objects()"""

    def literal_kernel(self, closed_form=True):
        M0, G0, Mt, Gt = self.literal_objects()
        return P.get_independent_parallel_kernel(M0, G0, Mt, Gt, self.N, gradient=self.gradient, grad=self.joint_grad if closed_form else None)[1]

    def literal_sweep(self, noise=None, x0=None):
        """(x, origins, history) of oracle/pit_np.py on this case's reference trajectory and noise (or the ones given)"""
        return self.literal_kernel()(L.Noise(u_bwd=None, **(self.noise if noise is None else noise)), self.x0 if x0 is None else x0, self.delta)

    def device_model(self):
        from aux_ssm_samplers_amd import _lib
        from aux_ssm_samplers_amd.csmc import _device
        M0, G0, Mt, Gt = self.device_objects()
        return _device.describe_independent(M0, G0, Mt, Gt, None, _lib.GRAD_EXACT if self.gradient else _lib.GRAD_NONE, parallel=True)

    def chains(self, Cn, seed):
        """Cn chains of this model: reference trajectories (Cn, T, d) around x0 and noise arrays with a leading chain axis, all different per chain.  (The
        step sizes delta (T,) are per time step and shared: auxssm_csmc_pit_sweep takes one sqrt_half_delta (T) for all chains of a launch.)"""
        rng = np.random.default_rng([seed, Cn, self.N, self.T, self.d])
        x0 = self.x0[None] + 0.3 * rng.standard_normal((Cn, self.T, self.d))
        return x0, dict(eps_aux=rng.standard_normal((Cn, self.T, self.d)), eps_prop=rng.standard_normal((Cn, self.T, self.N, self.d)),
                        u_res=rng.random((Cn, self.T, self.N)))


def keyed_noise(rng_normal, rng_uniform, Cn, T, N, d):
    """the explicit arrays of a Threefry-keyed sweep (include/auxssm.h: streams 1, 2, 3 at the flat indices of the explicit arrays), from fills
    rng_normal(stream, shape) / rng_uniform(stream, shape): the device's (handle.rng_normal / rng_uniform) or oracle/rng_np.py's"""
    return dict(eps_aux=rng_normal(1, (Cn, T, d)), eps_prop=rng_normal(2, (Cn, T, N, d)), u_res=rng_uniform(3, (Cn, T, N)))


class Case(_Sides):
    """one cell's model on all three sides, its reference trajectory, step sizes and noise"""

    def __init__(self, cell, seed=None):
        d, N, T, pot, gradient, tv, cell_seed = cell
        self.cell, self.N, self.T, self.pot, self.gradient, self.tv = cell, N, T, pot, bool(gradient), bool(tv)
        self.lorenz = d == "lorenz"
        d = self.d = 3 if self.lorenz else d
        seed = cell_seed if seed is None else seed
        rng = np.random.default_rng([seed, d, N, T, pot, gradient, tv, int(self.lorenz)])
        A = rng.standard_normal((d, d))
        Q = A @ A.T / d + 0.5 * np.eye(d)
        F = 0.9 * np.eye(d) + 0.05 * rng.standard_normal((d, d))
        b = 0.1 * rng.standard_normal(d)
        self.m0, self.P0 = 0.1 * rng.standard_normal(d), 2.0 * np.eye(d)
        self.theta, self.dt, self.sigma_x = np.array([10.0, 28.0, 8.0 / 3.0]), 0.01, 3.0
        y = rng.standard_normal((T, d))
        x0 = rng.standard_normal((T, d))
        if self.lorenz:
            assert not tv
            self.m0 = LORENZ_CENTRE.copy()
            self.F = self.b = None
            self.Q = self.sigma_x ** 2 * self.dt * np.eye(3)
            self.LQ = self.sigma_x * np.sqrt(self.dt) * np.eye(3)
            x0[0] += LORENZ_CENTRE  # a path of the model itself, observed with noise SIG_Y
            for t in range(1, T):
                x0[t] = self._lorenz_mean(x0[t - 1])[0] + self.LQ @ x0[t]
            y = x0 + SIG_Y * y
        else:
            if tv:
                F = F[None] + 0.05 * rng.standard_normal((T - 1, d, d))
                b = b[None] + 0.1 * rng.standard_normal((T - 1, d))
                Q = np.stack([Q * (0.5 + rng.random()) for _ in range(T - 1)])
            self.F, self.b, self.Q, self.LQ = F, b, Q, np.linalg.cholesky(Q)
        if pot == MASKED:
            y[rng.random((T, d)) < 0.3] = np.nan
            y[top_boundary(T)] = np.nan  # a whole missing step ON the stitch boundary of the top level
        self.y = None if pot == FLAT else y
        self.x0 = x0
        # gradient proposals: step sizes the shifted proposals do not overshoot with (tests/test_csmc_gradient_timevarying.py)
        self.delta = (0.05 + 0.1 * rng.random(T)) if (gradient or self.lorenz) else (0.5 + rng.random(T))
        self.noise = dict(eps_aux=rng.standard_normal((T, d)), eps_prop=rng.standard_normal((T, N, d)), u_res=rng.random((T, N)))

    def _lorenz_mean(self, xp):
        """(mean, Jacobian) of the Euler-Maruyama step at xp (examples/lorenz/model.py:10-25)"""
        th = self.theta
        f = np.array([th[0] * (xp[1] - xp[0]), th[1] * xp[0] - xp[1] - xp[0] * xp[2], xp[0] * xp[1] - th[2] * xp[2]])
        J = np.eye(3) + self.dt * np.array([[-th[0], th[0], 0.0], [th[1] - xp[2], -1.0, -xp[0]], [xp[1], xp[0], -th[2]]])
        return xp + self.dt * f, J

    # ---- the contract oracle's description (oracle/csmc.py) ----
    def oracle_model(self):
        od = dict(proposal=O.AUX_INDEPENDENT, potential=self.pot, m0=self.m0, chol_P0=np.linalg.cholesky(self.P0), sig_y=SIG_Y,
                  gradient=O.GRAD_EXACT if self.gradient else O.GRAD_NONE)
        if self.lorenz:
            Fl = np.zeros((3, 3))
            Fl[0] = self.theta
            od.update(F=Fl, b=[self.dt, 0, 0], chol_Q=self.LQ, transition=O.TRANS_LORENZ63_EM)
        elif self.tv:
            od.update(F=self.F[0], b=self.b[0], chol_Q=self.LQ[0], F_t=self.F, b_t=self.b, chol_Q_t=self.LQ)
        else:
            od.update(F=self.F, b=self.b, chol_Q=self.LQ)
        return od

    def oracle_sweep(self, dtype=np.float64):
        return O.pit_sweep(self.oracle_model(), self.x0, self.N, y=self.y, sqrt_half_delta=np.sqrt(0.5 * self.delta), dtype=dtype, **self.noise)

    # ---- the literal's protocol objects (oracle/csmc_np.py) ----
    def literal_objects(self):
        T = self.T
        M0 = L.GaussianInit(self.m0, np.linalg.cholesky(self.P0))
        Mt = L.Lorenz63EM(self.theta, self.dt, self.LQ, T) if self.lorenz else L.LinearGaussianDynamics(self.F, self.b, self.LQ, T)
        if self.pot == FLAT:
            return M0, L.FlatUnivariatePotential(), Mt, L.FlatPotential()
        kind = _POT_NAME[self.pot]
        return M0, L.ObsPotential(kind, self.y[0], SIG_Y, first=True), Mt, L.ObsPotential(kind, self.y[1:], SIG_Y)

    def joint_grad(self, u):
        """the gradient at u (T, d) of csmc_np._log_pdf (csmc/independent.py:121-134) in closed form; held against csmc_np.grad_fd by
        tests/test_oracle_pit_literal.py::test_closed_form_joint_gradient_equals_central_differences"""
        T, d = u.shape
        kind = None if self.pot == FLAT else _POT_NAME[self.pot]
        g = np.stack([G.grad_potential(kind, u[t], None if kind is None else self.y[t], SIG_Y) for t in range(T)])
        g[0] -= np.linalg.solve(self.P0, u[0] - self.m0)
        for t in range(1, T):
            xp = u[t - 1]
            if self.lorenz:
                (mean, J), Qt = self._lorenz_mean(xp), self.Q
            else:
                Ft, bt, Qt = (self.F[t - 1], self.b[t - 1], self.Q[t - 1]) if self.tv else (self.F, self.b, self.Q)
                mean, J = Ft @ xp + bt, Ft
            w = np.linalg.solve(Qt, u[t] - mean)
            g[t] -= w
            g[t - 1] += J.T @ w
        return g

    # ---- the device's objects (aux_ssm_samplers_amd.csmc) ----
    def device_objects(self):
        from aux_ssm_samplers_amd.csmc import (GaussianInit, LinearGaussianDynamics, Lorenz63Dynamics, FlatPotential, GaussianObsPotential,
                                               SVPotential, MaskedGaussianObsPotential)
        M0 = GaussianInit(m0=self.m0, P0=self.P0)
        if self.lorenz:
            Mt = Lorenz63Dynamics(theta=self.theta, sigma_x=self.sigma_x, dt=self.dt)
        else:
            Mt = LinearGaussianDynamics(F=self.F, b=self.b, Q=self.Q)
        y = self.y
        if self.pot == FLAT:
            G0, Gt = FlatPotential(), FlatPotential()
        elif self.pot == GAUSS:
            G0, Gt = GaussianObsPotential(sig=SIG_Y, y=y[0]), GaussianObsPotential(sig=SIG_Y, params=y[1:])
        elif self.pot == SV:
            G0, Gt = SVPotential(y=y[0]), SVPotential(params=y[1:])
        else:
            G0, Gt = MaskedGaussianObsPotential(sig=SIG_Y, y=y[0]), MaskedGaussianObsPotential(sig=SIG_Y, params=y[1:])
        return M0, G0, Mt, Gt


@functools.lru_cache(maxsize=None)
def case(cell):
    return Case(cell)


@functools.lru_cache(maxsize=None)
def literal(cell):
    """the literal sweep of a cell, computed once per process and shared: (x, origins, history); never modified by a test"""
    out = case(cell).literal_sweep()
    for a in (out[0], out[1], out[2]["xs"], out[2]["log_ws"]):
        a.setflags(write=False)
    return out


# ---- the multivariate Student-t potential (tests/mvt_np.py): no contract oracle restates it, the literal is its only oracle ------------------------------------
#            d  N    T   nu   gradient seed
MVT_CELLS = [
    (1, 32,  9,  4.0, 0, 0),
    (1, 33,  25, 1.0, 1, 0),
    (3, 100, 33, 4.0, 0, 0),
    (3, 32,  25, 1.0, 1, 0),
    (4, 33,  33, 4.0, 1, 0),
    (4, 100, 9,  1.0, 0, 0),
    (3, 33,  9,  4.0, 1, 0),
    (1, 100, 25, 4.0, 1, 0),
    (4, 32,  33, 1.0, 0, 0),
    (3, 33,  25, 1.0, 0, 0),
]


def mvt_cell_id(cell):
    d, N, T, nu, gradient, seed = cell
    return f"d{d}-N{N}-T{T}-nu{nu:g}-g{gradient}-s{seed}"


class MvtCase(_Sides):
    """tests/mvt_np.py::case: linear-Gaussian dynamics, a dense non-diagonal precision matrix, and flat steps (a NaN component in y_t) at t = 0, on the
    stitch boundary of the top level and at the last step"""

    def __init__(self, cell, seed=None):
        from tests import mvt_np as MV
        d, N, T, nu, gradient, cell_seed = cell
        self.cell, self.d, self.N, self.T, self.gradient = cell, d, N, T, bool(gradient)
        rng = np.random.default_rng([cell_seed if seed is None else seed, d, N, T, int(nu), gradient, 4])
        self.dev, self.m, xtrue, self.delta = MV.case(d, T, rng, nu=nu, nan_rows=(0, top_boundary(T), T - 1))
        assert np.max(np.abs(self.m.prec - np.diag(np.diag(self.m.prec)))) > 0.05 or d == 1
        self.x0 = xtrue + 0.3 * rng.standard_normal((T, d))
        self.noise = dict(eps_aux=rng.standard_normal((T, d)), eps_prop=rng.standard_normal((T, N, d)), u_res=rng.random((T, N)))

    def literal_objects(self):
        return self.m.literal()

    def joint_grad(self, u):
        from tests import potential_np
        return potential_np.joint_grad(self.m, u)

    def device_objects(self):
        return self.dev


@functools.lru_cache(maxsize=None)
def mvt_case(cell):
    return MvtCase(cell)


@functools.lru_cache(maxsize=None)
def mvt_literal(cell):
    out = mvt_case(cell).literal_sweep()
    for a in (out[0], out[1], out[2]["xs"], out[2]["log_ws"]):
        a.setflags(write=False)
    return out


# three chains in one launch, and the keyed path: one Gaussian and one Student-t cell each (cell, seed of the chains' inputs / the key's seed)
CHAIN_CELLS = [("gauss", (2, 33, 9, GAUSS, 1, 1, 0), 0), ("mvt", (3, 33, 25, 4.0, 1, 0), 0)]
KEYED_CELLS = [("gauss", (2, 100, 9, GAUSS, 0, 1, 0), 0), ("mvt", (3, 33, 25, 1.0, 0, 0), 0)]


def any_case(kind, cell):
    return case(cell) if kind == "gauss" else mvt_case(cell)
