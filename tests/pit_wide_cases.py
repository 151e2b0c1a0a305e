"""The wide-state cells (4 < d <= 32, N <= 64: csrc/pit_wide.hip) of the parallel-in-time cSMC sweep that tests/test_pit_wide_cells.py (contract oracle
against the literal tree, CPU) and tests/test_gpu_pit_wide.py (HIP kernels) share, in the format of tests/pit_cases.py (`PC.case(cell)`, `PC.literal(cell)`),
and the cases of the two coupled potentials, which no contract oracle restates.  Test infrastructure only.

The sizes: d in {5, 8, 16, 17, 30, 32} (one and two 4 x 4 blocks short of a full half-wave, odd, the stochastic-volatility protocol's 30, full), N in
{2, 25, 32, 33, 64} (32 | 33 is the edge between 64 and 256 chunks of a stitch, 64 the most a wide sweep takes), T in {2, 3, 5, 8, 9, 33, 37} (root only,
passthrough nodes, a full tree, one leaf beyond a power of two).  Each of the four separable potentials appears with gradient proposals off and on and with
time-varying transitions off and on.  Every seed is 0: at seed 0 each cell's smallest draw margin is >= 2 N^2 eps and each cell with N >= 25 moves at least
one time step off the reference trajectory (asserted by tests/test_pit_wide_cells.py)."""
import functools

import numpy as np

from tests import pit_cases as PC

FLAT, GAUSS, SV, MASKED = PC.FLAT, PC.GAUSS, PC.SV, PC.MASKED

#        d   N   T   potential gradient tv seed
WIDE_CELLS = [
    (5,  25, 9,  SV,     0, 0, 0),
    (8,  33, 5,  MASKED, 1, 0, 0),
    (30, 25, 33, SV,     0, 0, 0),
    (32, 64, 8,  GAUSS,  1, 1, 0),
    (30, 25, 9,  SV,     1, 0, 0),
    (16, 2,  37, FLAT,   0, 1, 0),
    (17, 32, 3,  FLAT,   1, 0, 0),
    (17, 33, 2,  GAUSS,  0, 0, 0),
    (5,  64, 5,  MASKED, 0, 1, 0),
    (8,  32, 9,  SV,     1, 1, 0),
    (32, 2,  3,  MASKED, 1, 1, 0),
    (5,  33, 33, FLAT,   0, 0, 0),
]

# ---- the coupled potentials (tests/mvt_np.py, tests/lingauss_np.py): the literal tree is their only oracle ------------------------------------------------
#                 kind   d   N   T  gradient seed (the smallest of 0..31 that meets the margin condition and moves a time step off the reference trajectory)
COUPLED_CELLS = [(kind, d, N, T, g, 0) for kind in ("mvt", "lin") for d, N, T in ((5, 33, 9), (9, 25, 5), (25, 25, 9)) for g in (0, 1)]


def coupled_cell_id(cell):
    kind, d, N, T, g, seed = cell
    return f"{kind}-d{d}-N{N}-T{T}-g{g}-s{seed}"


class CoupledCase(PC._Sides):
    """linear-Gaussian dynamics under the multivariate Student-t potential (d = 25: the precision matrix of the 5 x 5 spatial grid) or the linear-Gaussian
    observation potential (dy = ceil(d / 3)), with a flat step -- the whole observation row NaN -- at t = 0, on the stitch boundary of the top level and at T - 1"""

    def __init__(self, cell):
        from tests import mvt_np as MV, lingauss_np as LG, potential_np
        from aux_ssm_samplers_amd import workloads
        kind, d, N, T, gradient, seed = cell
        self.cell, self.kind, self.d, self.N, self.T, self.gradient = cell, kind, d, N, T, bool(gradient)
        rng = np.random.default_rng([seed, d, N, T, gradient, kind == "lin"])
        self.flat_rows = sorted({0, PC.top_boundary(T), T - 1})
        if kind == "mvt":
            from aux_ssm_samplers_amd.csmc import MultivariateTPotential
            prec = workloads.spatial_precision(5) if d == 25 else None
            dev, m, xtrue, self.delta = MV.case(d, T, rng, nu=4.0, prec=prec)
            y = m.y.copy()
            y[self.flat_rows] = np.nan
            self.dev = (dev[0], MultivariateTPotential(nu=m.nu, prec=m.prec, y=y[0]), dev[2], MultivariateTPotential(nu=m.nu, prec=m.prec, params=y[1:]))
            self.m = MV.model(m.m0, m.P0, m.dyn, m.Q, m.nu, m.prec, y)
        else:
            _, m, xtrue, self.delta = LG.case(d, (d + 2) // 3, T, rng)
            y = m.y.copy()
            y[self.flat_rows] = np.nan
            self.dev, self.m = LG.build(m.m0, m.P0, m.F, m.b, m.Q, m.H, m.R, m.c, y)
        self._grad = potential_np.joint_grad
        self.x0 = xtrue + 0.3 * rng.standard_normal((T, d))
        self.noise = dict(eps_aux=rng.standard_normal((T, d)), eps_prop=rng.standard_normal((T, N, d)), u_res=rng.random((T, N)))

    def literal_objects(self):
        return self.m.literal()

    def joint_grad(self, u):
        return self._grad(self.m, u)

    def device_objects(self):
        return self.dev


@functools.lru_cache(maxsize=None)
def coupled_case(cell):
    return CoupledCase(cell)


@functools.lru_cache(maxsize=None)
def coupled_literal(cell):
    """the literal sweep of a coupled cell, computed once per process and shared; never modified by a test"""
    out = coupled_case(cell).literal_sweep()
    for a in (out[0], out[1], out[2]["xs"], out[2]["log_ws"]):
        a.setflags(write=False)
    return out
