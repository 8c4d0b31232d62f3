"""numpy float64 restatement of the adr kind with per-point coefficient fields (pinn_set_coef_fields, include/pinn_hip.h):
adr_src_ref.src_loss_grad with a row of six coefficients per collocation point,

    f_i = u_t + (a0_i + a1_i u) u_x - nu_i u_xx + r1_i u + r2_i u^2 + r3_i u^3 - s_i,

through the same Taylor-mode forward / reverse sweeps of oracle.mlp, plus Robin points via adr_robin_ref.  The seeds are
adr_ref's with the point's own row where the constants stand.  Every statement is adr_src_ref's, in its order, with a column
[N_f, 1] where it has a scalar: numpy applies the same IEEE operation per element, so a table whose every row is the
constant set returns adr_src_ref's values bit for bit.  tests/test_adr_var_host.py pins this module against torch autograd."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adr_ref  # noqa: E402,F401
import adr_robin_ref  # noqa: E402
import adr_src_ref  # noqa: E402,F401
from adr_ref import mlp  # noqa: E402


def constant_rows(coeffs, n):
    """the table of a constant medium: n rows, each the constant set"""
    return np.tile(np.asarray(coeffs, dtype=np.float64).reshape(1, 6), (n, 1))


def _columns(K, n):
    K = np.asarray(K, dtype=np.float64)
    if K.shape != (n, 6):
        raise ValueError("K must hold one row of six coefficients per collocation point (%d), got shape %s" % (n, K.shape))
    return [np.ascontiguousarray(K[:, j]).reshape(-1, 1) for j in range(6)]


def residual(w, layers, lb, ub, X, K, s=None):
    """f at the points X [n, 2] with the rows K [n, 6] -> [n, 1]; s [n] or None"""
    lb, ub = np.asarray(lb, dtype=np.float64), np.asarray(ub, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64)
    a0, a1, nu, r1, r2, r3 = _columns(K, X.shape[0])
    (h, p, q, r), _ = mlp.taylor_forward(mlp.unpack(w, layers), X, lb, ub)
    f = q + (a0 + a1 * h) * p - nu * r + r1 * h + r2 * h * h + r3 * h * h * h
    return f if s is None else f - np.asarray(s, dtype=np.float64).reshape(-1, 1)


def var_loss_grad(w, layers, lb, ub, X_f, X_u, u, X_lo, X_hi, K, s=None, X_w=None, alpha=None, beta=None, g=None,
                  n_f_total=None, n_u_total=None, n_b_total=None, n_w_total=None):
    """-> (loss, flat gradient, {"f", "mse_f", "mse_u", "mse_b", "mse_w", "r"}); K [N_f, 6], s [N_f] or None (no source),
    X_u / X_lo / X_w may be None or empty"""
    lb, ub = np.asarray(lb, dtype=np.float64), np.asarray(ub, dtype=np.float64)
    a0, a1, nu, r1, r2, r3 = _columns(K, X_f.shape[0])
    params = mlp.unpack(w, layers)
    N_f = X_f.shape[0] if n_f_total is None else n_f_total
    (h, p, q, r), cache = mlp.taylor_forward(params, X_f, lb, ub)
    f = q + (a0 + a1 * h) * p - nu * r + r1 * h + r2 * h * h + r3 * h * h * h
    if s is not None:
        s = np.asarray(s, dtype=np.float64).reshape(-1, 1)
        if s.shape != f.shape:
            raise ValueError("s must hold one value per collocation point (%d), got %d" % (f.shape[0], s.size))
        f = f - s
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
    base = (mse_f + mse_u + mse_b, mlp.pack(grads), {"f": f, "mse_f": mse_f, "mse_u": mse_u, "mse_b": mse_b})
    # Robin points carry no coefficients: adr_robin_ref adds its part to whatever the base gives
    return adr_robin_ref.robin_loss_grad(w, layers, lb, ub, X_f, X_u, u, X_lo, X_hi, None, X_w, alpha, beta, g,
                                         n_w_total=n_w_total, base=base)
