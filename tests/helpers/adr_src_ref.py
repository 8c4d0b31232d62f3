"""numpy float64 restatement of the adr kind with a source term (pinn_set_source, include/pinn_hip.h): adr_ref.adr_loss_grad
with the residual

    f_i = u_t + (a0 + a1 u) u_x - nu u_xx + r1 u + r2 u^2 + r3 u^3 - s_i

at collocation point i, through the same Taylor-mode forward / reverse sweeps of oracle.mlp, plus Robin points via
adr_robin_ref.  The seeds are adr_ref's with this f: dF/d(u, u_x, u_t, u_xx) do not depend on s.  The subtraction is an
operation of its own behind adr_ref's expression for f, so a source of zeros returns adr_ref's values bit for bit.
tests/test_adr_source_host.py pins this module against torch autograd."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adr_ref  # noqa: E402
import adr_robin_ref  # noqa: E402
from adr_ref import mlp  # noqa: E402


def residual(w, layers, lb, ub, X, coeffs, s=None):
    """f at the points X [n, 2] -> [n, 1]; s [n] or None (the operator part N[u])"""
    f = adr_ref.residual(w, layers, lb, ub, X, coeffs)
    return f if s is None else f - np.asarray(s, dtype=np.float64).reshape(-1, 1)


def src_loss_grad(w, layers, lb, ub, X_f, X_u, u, X_lo, X_hi, coeffs, s=None, X_w=None, alpha=None, beta=None, g=None,
                  n_f_total=None, n_u_total=None, n_b_total=None, n_w_total=None):
    """-> (loss, flat gradient, {"f", "mse_f", "mse_u", "mse_b", "mse_w", "r"}); s [N_f] or None (no source), X_u / X_lo /
    X_w may be None or empty.  The statements are adr_ref.adr_loss_grad's, in its order, with f - s where it has f."""
    a0, a1, nu, r1, r2, r3 = (float(v) for v in coeffs)
    lb, ub = np.asarray(lb, dtype=np.float64), np.asarray(ub, dtype=np.float64)
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
    # Robin points: adr_robin_ref adds its part to whatever the base gives
    return adr_robin_ref.robin_loss_grad(w, layers, lb, ub, X_f, X_u, u, X_lo, X_hi, coeffs, X_w, alpha, beta, g,
                                         n_w_total=n_w_total, base=base)
