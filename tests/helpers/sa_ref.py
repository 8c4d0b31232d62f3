"""numpy restatement of self-adaptive point weights (include/pinn_hip.h pinn_sa_*, the SAW variants of
pinns-tf2.0_amd/csrc/kernels_fused20d.h) for Burgers inference:

    L(theta, lam) = (1/N_f) sum_i lam_f,i^2 f_i^2 + (1/N_u) sum_j lam_u,j^2 (u_j - u*_j)^2

its gradient in theta, its gradient in lam (dL/dlam = 2 lam r^2 / N), and Adam steps that descend in theta and ascend in lam
from one evaluation, in the TF form k_reduce_adam uses (m += (1-b1)(g-m), v += (1-b2)(g^2-v), step alpha m / (sqrt(v)+eps),
alpha = lr sqrt(1-b2^t) / (1-b1^t))."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from oracle import mlp, pde  # noqa: E402


def loss_grad(w, layers, lb, ub, X_f, X_u, u_data, nu, lam_u, lam_f):
    """-> (loss, grad_theta, terms = (mse_f, mse_u), dL/dlam_u, dL/dlam_f)"""
    lb, ub = np.asarray(lb, dtype=np.float64), np.asarray(ub, dtype=np.float64)
    lam_u = np.asarray(lam_u, dtype=np.float64).reshape(-1, 1)
    lam_f = np.asarray(lam_f, dtype=np.float64).reshape(-1, 1)
    params = mlp.unpack(w, layers)
    N_f, N_u = X_f.shape[0], X_u.shape[0]
    f, (u, u_x, u_t, u_xx), cache = pde.burgers_residual(params, X_f, lb, ub, 1.0, nu)
    f = f.reshape(-1, 1)
    mf = lam_f * lam_f
    mse_f = np.sum(mf * f * f) / N_f
    fb = 2.0 * mf * f / N_f
    grads = mlp.taylor_backward(params, cache, (fb * u_x.reshape(-1, 1)).reshape(u_x.shape),
                                (fb * u.reshape(-1, 1)).reshape(u.shape), fb.reshape(u.shape), (-nu * fb).reshape(u.shape))
    u_pred = mlp.forward_value(params, X_u, lb, ub).reshape(-1, 1)
    d = u_pred - np.asarray(u_data, dtype=np.float64).reshape(-1, 1)
    mu = lam_u * lam_u
    mse_u = np.sum(mu * d * d) / N_u
    grads = mlp.add_grads(grads, mlp.value_backward(params, X_u, lb, ub, 2.0 * mu * d / N_u))
    dlam_f = (2.0 * lam_f * f * f / N_f).ravel()
    dlam_u = (2.0 * lam_u * d * d / N_u).ravel()
    return mse_f + mse_u, mlp.pack(grads), (mse_f, mse_u), dlam_u, dlam_f


def loss_only(w, layers, lb, ub, X_f, X_u, u_data, nu, lam_u, lam_f):
    return loss_grad(w, layers, lb, ub, X_f, X_u, u_data, nu, lam_u, lam_f)[0]


def adam(w, lam_u, lam_f, n_steps, layers, lb, ub, X_f, X_u, u_data, nu, lr, lr_lam, b1=0.9, b2=0.999, eps=1e-7):
    """n_steps Adam steps from zero moments (step counter from 1): theta descends, lam ascends; -> (w, lam_u, lam_f, losses)"""
    w = np.array(w, dtype=np.float64)
    lam = [np.array(lam_u, dtype=np.float64), np.array(lam_f, dtype=np.float64)]
    m, v = np.zeros_like(w), np.zeros_like(w)
    ml, vl = [np.zeros_like(x) for x in lam], [np.zeros_like(x) for x in lam]
    losses = []
    for t in range(1, n_steps + 1):
        loss, g, _, gu, gf = loss_grad(w, layers, lb, ub, X_f, X_u, u_data, nu, lam[0], lam[1])
        losses.append(loss)
        scale = np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
        m += (1.0 - b1) * (g - m)
        v += (1.0 - b2) * (g * g - v)
        w = w - (lr * scale) * m / (np.sqrt(v) + eps)
        if lr_lam > 0:
            for k, gl in enumerate((gu, gf)):
                ml[k] += (1.0 - b1) * (gl - ml[k])
                vl[k] += (1.0 - b2) * (gl * gl - vl[k])
                lam[k] = lam[k] + (lr_lam * scale) * ml[k] / (np.sqrt(vl[k]) + eps)
    return w, lam[0], lam[1], np.array(losses)
