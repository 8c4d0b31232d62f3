"""numpy float64 restatement of the adr kind's Robin points (pinn_set_robin, include/pinn_hip.h): adr_ref's loss plus

    r_j = alpha_j u(x_j, t_j) + beta_j u_x(x_j, t_j) - g_j,      mse_w = (1 / N_w) sum_j r_j^2

through the same Taylor-mode forward / reverse sweeps of oracle.mlp.  Hand-derived seeds at a Robin point:
    u_bar = 2 r_j alpha_j / N_w,   u_x_bar = 2 r_j beta_j / N_w,   u_t_bar = u_xx_bar = 0
The device adds mse_w to the boundary part of the loss: terms[2] = mse_b + mse_w.  tests/test_adr_robin_host.py pins this
module against torch autograd; with no Robin points it returns adr_ref's values bit for bit."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adr_ref  # noqa: E402
from adr_ref import mlp  # noqa: E402


def robin_residual(w, layers, lb, ub, X_w, alpha, beta, g):
    """r at the points X_w [n, 2] -> [n]"""
    lb, ub = np.asarray(lb, dtype=np.float64), np.asarray(ub, dtype=np.float64)
    (h, p, _, _), _ = mlp.taylor_forward(mlp.unpack(w, layers), np.asarray(X_w, dtype=np.float64), lb, ub)
    col = lambda v: np.broadcast_to(np.asarray(v, dtype=np.float64).reshape(-1, 1), h.shape)    # noqa: E731
    return (col(alpha) * h + col(beta) * p - col(g)).ravel()


def robin_loss_grad(w, layers, lb, ub, X_f, X_u, u, X_lo, X_hi, coeffs, X_w=None, alpha=None, beta=None, g=None,
                    n_f_total=None, n_u_total=None, n_b_total=None, n_w_total=None, base=None):
    """-> (loss, flat gradient, adr_ref's extras + {"mse_w", "r"}); X_w may be None or empty.  base: what
    adr_ref.adr_loss_grad returned for the same weights and sets (a test that varies only the Robin points computes it once)"""
    loss, grad, ex = base if base is not None else adr_ref.adr_loss_grad(
        w, layers, lb, ub, X_f, X_u, u, X_lo, X_hi, coeffs, n_f_total=n_f_total, n_u_total=n_u_total, n_b_total=n_b_total)
    ex = dict(ex, mse_w=0.0, r=np.zeros(0))
    if X_w is None or len(X_w) == 0:
        return loss, grad, ex
    lb, ub = np.asarray(lb, dtype=np.float64), np.asarray(ub, dtype=np.float64)
    X_w = np.asarray(X_w, dtype=np.float64)
    n = X_w.shape[0]
    N_w = n if n_w_total is None else n_w_total
    col = lambda v: np.broadcast_to(np.asarray(v, dtype=np.float64).reshape(-1, 1), (n, 1))    # noqa: E731
    al, be, gg = col(alpha), col(beta), col(g)
    params = mlp.unpack(w, layers)
    (h, p, _, _), cache = mlp.taylor_forward(params, X_w, lb, ub)
    r = al * h + be * p - gg
    mse_w = np.sum(r * r) / N_w
    z = np.zeros_like(r)
    gw = mlp.taylor_backward(params, cache, 2.0 * r * al / N_w, 2.0 * r * be / N_w, z, z)
    grad = grad + mlp.pack(gw)
    ex["mse_w"], ex["r"] = mse_w, r.ravel()
    return loss + mse_w, grad, ex
