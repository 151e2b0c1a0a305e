#!/usr/bin/env python3
"""Ground truth of tests/test_gpu_observation_theta.py::test_gibbs_over_state_and_observation_model_matches_quadrature: the posterior means of
(H, c, log R, x_0, x_5) of a scalar LGConcatModel (dx = dy = 1, T = 6; F, b, Q, m0, P0 fixed) under an ObsMNIWPrior, by a midpoint rule on an n^3 grid over
(H, c, log R) with the state integrated out by a NumPy Kalman filter (the weight is prior x marginal likelihood) and a backward smoother (the conditional means
of the states).  The model is sign-symmetric in (H, x) when m0 = b = 0; here m0 = 2, b = 0.5, F = 0.8 and the prior is centred at H = 1 with K0 informative,
and the script checks that the quadrature's mass at H < 0 is below 1e-6 and that halving the grid moves the five means by less than 1e-8.

    python tests/golden/make_observation_theta_quadrature.py            writes tests/golden/observation_theta_quadrature.json
    python tests/golden/make_observation_theta_quadrature.py --check    recomputes and compares with the file (1e-12)
"""
import json
import os
import sys

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "observation_theta_quadrature.json")
N_FINE = 160
RANGES = dict(H=(-0.6, 2.6), c=(-3.2, 3.2), s=(-5.0, 4.0))


def joint_model(T=6):
    """the model's ingredients, the data and the prior"""
    rng = np.random.default_rng(2025)
    m0, P0, F, b, Q = 2.0, 0.5, 0.8, 0.5, 0.25
    H, c, R = 1.1, -0.2, 0.3
    x = np.zeros(T)
    x[0] = m0 + np.sqrt(P0) * rng.standard_normal()
    for t in range(T - 1):
        x[t + 1] = F * x[t] + b + np.sqrt(Q) * rng.standard_normal()
    y = H * x + c + np.sqrt(R) * rng.standard_normal(T)
    return dict(T=T, y=y, m0=m0, P0=P0, F=F, b=b, Q=Q, H=H, c=c, R=R, M0=np.array([[1.0, 0.0]]), K0=np.array([[30.0, 2.0], [2.0, 8.0]]), nu0=20.0,
                Psi0=np.array([[5.4]]))


def quadrature(j, n):
    """-> (means of H, c, log R, x_0, x_{T-1}; the posterior mass at H < 0)"""
    T, y = j["T"], j["y"]
    M0, K0, nu0, Psi0 = j["M0"][0], j["K0"], j["nu0"], j["Psi0"][0, 0]

    def mid(lo, hi):
        h = (hi - lo) / n
        return lo + h * (np.arange(n) + 0.5)

    Hg, cg, sg = np.meshgrid(mid(*RANGES["H"]), mid(*RANGES["c"]), mid(*RANGES["s"]), indexing="ij")
    R = np.exp(sg)
    d0, d1 = Hg - M0[0], cg - M0[1]
    quad = K0[0, 0] * d0 * d0 + 2 * K0[0, 1] * d0 * d1 + K0[1, 1] * d1 * d1
    # log prior in (H, c, s = log R): IW(nu0, Psi0) in R (dy = 1) x the Jacobian R, MN(M0, R, K0^-1) in A = [H c] (n = 2 columns: R^-1)
    lp = -0.5 * (nu0 + 2.0) * sg - 0.5 * Psi0 / R + sg - 1.0 * sg - 0.5 * quad / R
    m, P = np.full(Hg.shape, j["m0"]), np.full(Hg.shape, j["P0"])
    ms, Ps, mp, Pp = [], [], [], []
    ll = np.zeros(Hg.shape)
    for t in range(T):
        if t > 0:
            m, P = j["F"] * m + j["b"], j["F"] ** 2 * P + j["Q"]
        mp.append(m), Pp.append(P)
        S = Hg * Hg * P + R
        e = y[t] - Hg * m - cg
        ll += -0.5 * np.log(2 * np.pi * S) - 0.5 * e * e / S
        K = P * Hg / S
        m, P = m + K * e, (1.0 - K * Hg) * P
        ms.append(m), Ps.append(P)
    sm = ms[-1]
    xT = sm
    for t in range(T - 2, -1, -1):
        G = Ps[t] * j["F"] / Pp[t + 1]
        sm = ms[t] + G * (sm - mp[t + 1])
    lw = lp + ll
    w = np.exp(lw - lw.max())
    w /= w.sum()
    return np.array([np.sum(w * Hg), np.sum(w * cg), np.sum(w * sg), np.sum(w * sm), np.sum(w * xT)]), float(np.sum(w[Hg < 0]))


def compute():
    j = joint_model()
    fine, neg = quadrature(j, N_FINE)
    coarse, _ = quadrature(j, N_FINE // 2)
    move = float(np.max(np.abs(fine - coarse)))
    assert neg < 1e-6, f"posterior mass at H < 0: {neg}"
    assert move < 1e-8, f"halving the grid moves the means by {move}"
    return dict(names=["H", "c", "log R", "x_0", "x_5"], means=[float(v) for v in fine], grid=N_FINE, mass_H_negative=neg, grid_halving_moves=move)


if __name__ == "__main__":
    out = compute()
    if len(sys.argv) > 1 and sys.argv[1] == "--check":
        want = json.load(open(PATH))
        err = float(np.max(np.abs(np.array(out["means"]) - np.array(want["means"]))))
        print(f"recomputed means differ from {os.path.basename(PATH)} by {err:.2e}")
        sys.exit(0 if err <= 1e-12 else 1)
    with open(PATH, "w") as f:
        json.dump(out, f, indent=1)
    print(out)
