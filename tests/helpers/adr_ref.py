"""numpy float64 restatement of the advection-diffusion-reaction residual kind (PINN_PDE_ADR, include/pinn_hip.h):

    f = u_t + (a0 + a1 u) u_x - nu u_xx + r1 u + r2 u^2 + r3 u^3                 coeffs = [a0, a1, nu, r1, r2, r3]
    L = mean_f f^2 + mean_u (u - u*)^2 + mean_b [(u(lo) - u(hi))^2 + (u_x(lo) - u_x(hi))^2]

built from oracle.mlp's Taylor-mode forward / reverse sweeps the way oracle/pde.py builds Burgers.  Hand-derived seeds:
    dF/du = a1 u_x + r1 + 2 r2 u + 3 r3 u^2,  dF/du_x = a0 + a1 u,  dF/du_t = 1,  dF/du_xx = -nu
tests/test_adr_host.py pins it against torch autograd and against the reference-made Burgers fixture."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from oracle import mlp  # noqa: E402

BURGERS = lambda nu=0.01 / np.pi: [0.0, 1.0, nu, 0.0, 0.0, 0.0]      # noqa: E731
ALLEN_CAHN = [0.0, 0.0, 1e-4, -5.0, 0.0, 5.0]
FISHER_KPP = [0.0, 0.0, 0.01, -2.0, 2.0, 0.0]
ADVECTION_DIFFUSION = [0.7, 0.0, 0.05, 0.0, 0.0, 0.0]
ALL_NONZERO = [0.3, -0.8, 0.02, 0.6, -0.4, 1.5]
COEFF_SETS = {"burgers": BURGERS(), "allen_cahn": ALLEN_CAHN, "fisher_kpp": FISHER_KPP,
              "advection_diffusion": ADVECTION_DIFFUSION, "all_nonzero": ALL_NONZERO}


def residual(w, layers, lb, ub, X, coeffs):
    """f at the points X [n, 2] -> [n, 1]"""
    a0, a1, nu, r1, r2, r3 = (float(v) for v in coeffs)
    lb, ub = np.asarray(lb, dtype=np.float64), np.asarray(ub, dtype=np.float64)
    (u, u_x, u_t, u_xx), _ = mlp.taylor_forward(mlp.unpack(w, layers), X, lb, ub)
    return u_t + (a0 + a1 * u) * u_x - nu * u_xx + r1 * u + r2 * u * u + r3 * u * u * u


def adr_loss_grad(w, layers, lb, ub, X_f, X_u, u, X_lo, X_hi, coeffs, n_f_total=None, n_u_total=None, n_b_total=None):
    """-> (loss, flat gradient, {"f", "mse_f", "mse_u", "mse_b"}); X_u / X_lo may be None or empty"""
    a0, a1, nu, r1, r2, r3 = (float(v) for v in coeffs)
    lb, ub = np.asarray(lb, dtype=np.float64), np.asarray(ub, dtype=np.float64)
    params = mlp.unpack(w, layers)
    N_f = X_f.shape[0] if n_f_total is None else n_f_total
    (h, p, q, r), cache = mlp.taylor_forward(params, X_f, lb, ub)
    f = q + (a0 + a1 * h) * p - nu * r + r1 * h + r2 * h * h + r3 * h * h * h
    mse_f = np.sum(f * f) / N_f
    fb = 2.0 * f / N_f
    grads = mlp.taylor_backward(params, cache, fb * (a1 * p + r1 + 2.0 * r2 * h + 3.0 * r3 * h * h), fb * (a0 + a1 * h),
                                fb, -nu * fb)
    mse_u = mse_b = 0.0
    if X_u is not None and len(X_u):
        N_u = X_u.shape[0] if n_u_total is None else n_u_total
        d = mlp.forward_value(params, X_u, lb, ub) - np.asarray(u, dtype=np.float64).reshape(-1, 1)
        mse_u = np.sum(d * d) / N_u
        grads = mlp.add_grads(grads, mlp.value_backward(params, X_u, lb, ub, 2.0 * d / N_u))
    if X_lo is not None and len(X_lo):
        N_b = X_lo.shape[0] if n_b_total is None else n_b_total
        (hl, pl, _, _), cl = mlp.taylor_forward(params, X_lo, lb, ub)
        (hu, pu, _, _), cu = mlp.taylor_forward(params, X_hi, lb, ub)
        dh, dp = hl - hu, pl - pu
        mse_b = (np.sum(dh * dh) + np.sum(dp * dp)) / N_b
        z = np.zeros_like(dh)
        grads = mlp.add_grads(grads, mlp.taylor_backward(params, cl, 2.0 * dh / N_b, 2.0 * dp / N_b, z, z))
        grads = mlp.add_grads(grads, mlp.taylor_backward(params, cu, -2.0 * dh / N_b, -2.0 * dp / N_b, z, z))
    return mse_f + mse_u + mse_b, mlp.pack(grads), {"f": f, "mse_f": mse_f, "mse_u": mse_u, "mse_b": mse_b}
