// fk_user_pre.h -- what a user-defined Feynman-Kac model sees (fk_program.hip puts it in front of the user's source; hipRTC, gfx950, -ffp-contract=off).
// The contract of the user's functions, all at global scope (R = float / double, D = the state dimension, 1..4):
//   required              template <typename R, int D> __device__ R log_g(int t, const R* x, const R* xprev, const R* y, const R* theta);
//                           log G_t(x_t); t = the time index of x (0 for G0); xprev = x_{t-1} (nullptr at t = 0); y = row t of the (T, p) observations
//                           (nullptr without); theta = the potential's constant parameters (nullptr without)
//   optional              template <typename R, int D> __device__ R log_g_bound(int t, const R* y, const R* theta);
//                           sup_x log G_t (or +inf): the forward pass shifts its weights by it as by k_csmc_potbound's bound; absent -> exact maxima
//   optional (dynamics)   template <typename R, int D> __device__ void mean(int t, const R* xprev, const R* theta, R* mu);
//                           the mean of x_t | x_{t-1}; the noise stays N(0, chol_Q chol_Q^T)
// Derivatives, read only by a program compiled for gradient-informed proposals (AUXSSM_FK_USER_GRADIENT), which needs the one of each user-defined part
// (the built-in part keeps its own derivative):
//   gradient (potential)  template <typename R, int D> __device__ void grad_log_g(int t, const R* x, const R* xprev, const R* y, const R* theta, R* gx, R* gxprev);
//                           the partial derivatives of log_g(t, x, xprev, y, theta): gx (D) w.r.t. x, gxprev (D) w.r.t. xprev (nullptr at t = 0); the
//                           caller zero-fills both, so a potential that does not read xprev leaves gxprev alone
//   gradient (dynamics)   template <typename R, int D> __device__ void mean_vjp(int t, const R* xprev, const R* theta, const R* v, R* out);
//                           out = J^T v, J = d mean(t, xprev) / d xprev (the vector-Jacobian product of the transition mean)
// Available: fma_, det_exp, det_log (det_math.h: the bit-reproducible exp / log of the built-in potentials) and hipRTC's device math (exp, log, lgamma, ...).
#pragma once
#include "csmc_sweep.h"

using ax::det_exp;
using ax::det_log;
using ax::fma_;

// fallbacks of a signature no user function has: the names always exist, so fk_user.h can detect which of them the source defines
struct fk_absent {};
template <typename R, int D> __device__ fk_absent log_g(fk_absent);
template <typename R, int D> __device__ fk_absent log_g_bound(fk_absent);
template <typename R, int D> __device__ fk_absent mean(fk_absent);
template <typename R, int D> __device__ fk_absent grad_log_g(fk_absent);
template <typename R, int D> __device__ fk_absent mean_vjp(fk_absent);
