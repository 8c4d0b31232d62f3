"""numpy restatement of the advection-diffusion-reaction kind with TRAINABLE coefficients (PINN_PDE_ADR_IDE, pde="adr_ide"):

    theta = [net weights | a0, a1, log nu, r1, r2, r3]                      nu = exp(log nu)
    f = u_t + (a0 + a1 u) u_x - nu u_xx + r1 u + r2 u^2 + r3 u^3            on the collocation points
    L = mean_f f^2 + mean_u (u - u*)^2 + mean_b [(u(lo) - u(hi))^2 + (u_x(lo) - u_x(hi))^2]

The net entries of the gradient are those of adr_ref at the current coefficients; the six tail entries, with fb = 2 f / N_f:
    a0: sum fb u_x,  a1: sum fb u u_x,  log nu: -sum fb nu u_xx,  r1: sum fb u,  r2: sum fb u^2,  r3: sum fb u^3
and the entry of a coefficient that is not in `mask` is exactly 0.0.  The sweeps are those of tests/helpers/grad_entries.py
(oracle.mlp's in any dtype), so the same code gives the float64 oracle, the float32 / longdouble runs that the entrywise
bounds need, and the scale A_k = sum |fb df/dp_k| of every tail entry.  tests/test_adr_ide_host.py pins it against torch
autograd and against the reference-made identification fixture."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_entries as ge  # noqa: E402

NAMES = ("a0", "a1", "nu", "r1", "r2", "r3")
ALL = 63


def mask_of(names):
    """names from NAMES (or an int) -> bit mask, bit k = NAMES[k]"""
    if isinstance(names, (int, np.integer)):
        return int(names)
    return sum(1 << NAMES.index(n) for n in names)


def n_net(layers):
    return sum(a * b + b for a, b in zip(layers[:-1], layers[1:]))


def pack(w, coeffs):
    """net weights + raw [a0, a1, nu, r1, r2, r3] -> theta (log nu in the nu slot)"""
    tail = np.array(coeffs, dtype=np.float64)
    tail[2] = np.log(tail[2])
    return np.concatenate([np.asarray(w, dtype=np.float64).ravel(), tail])


def raw_coeffs(theta):
    tail = np.array(theta[-6:], dtype=np.float64)
    tail[2] = np.exp(tail[2])
    return tail


def restate(theta, layers, lb, ub, X_f, X_u, u, X_lo, X_hi, mask=ALL, dtype=np.float64, n_f_total=None, n_u_total=None,
            n_b_total=None):
    """-> (loss, flat gradient [n_net + 6], A, extras) with all arithmetic in `dtype`; A is the entrywise rounding scale
    of grad_entries (tail: sum |fb df/dp_k|, 0 where frozen); extras: f, mse_f, mse_u, mse_b.  n_*_total: the denominator
    of a class whose rows are a block of a larger set (a rank's shard), or that has lost rows (mutants)"""
    dt = np.dtype(dtype).type
    wide = np.longdouble if dt is np.longdouble else np.float64
    lbd = np.asarray(lb, dtype=wide)
    s = (2 / (np.asarray(ub, dtype=wide) - lbd)).astype(dt)
    lbd = lbd.astype(dt)
    theta = np.asarray(theta, dtype=np.float64)
    cast = lambda x: np.asarray(x, dtype=np.float64).astype(dt)
    nn = n_net(layers)
    assert theta.size == nn + 6, (theta.size, nn)
    params = ge._unpack(theta[:nn], layers, dt)
    G = [[np.zeros(W.shape, dt), np.zeros(b.shape, dt)] for W, b in params]
    A = [[np.zeros(W.shape), np.zeros(b.shape)] for W, b in params]
    a0, a1, lnu, r1, r2, r3 = (dt(v) for v in theta[nn:])
    nu = np.exp(lnu)
    X_f = cast(X_f).reshape(-1, 2)
    n_f = dt(X_f.shape[0] if n_f_total is None else n_f_total)
    (h, p, q, r), cache = ge._forward(params, X_f, lbd, s, False)
    f = q + (a0 + a1 * h) * p - nu * r + h * (r1 + h * (r2 + r3 * h))
    fb = dt(2) * f / n_f
    ge._backward(params, cache, fb * (a1 * p + r1 + h * (dt(2) * r2 + dt(3) * r3 * h)), fb * (a0 + a1 * h), fb, -nu * fb, G, A)
    mse_f = np.sum(f * f) / n_f
    terms = [fb * p, fb * h * p, -(fb * nu) * r, fb * h, fb * h * h, fb * h * h * h]
    tail_g = np.array([np.sum(t) if (mask >> k) & 1 else dt(0) for k, t in enumerate(terms)], dtype=dt)
    tail_a = np.array([np.sum(ge._abs64(t)) if (mask >> k) & 1 else 0.0 for k, t in enumerate(terms)])
    mse_u = mse_b = dt(0)
    zero = lambda x: np.zeros_like(x)
    if X_u is not None and len(X_u):
        X_u, u = cast(X_u).reshape(-1, 2), cast(u).reshape(-1, 1)
        n_u = dt(X_u.shape[0] if n_u_total is None else n_u_total)
        (hu, _, _, _), cu = ge._forward(params, X_u, lbd, s, False)
        d = hu - u
        ge._backward(params, cu, dt(2) * d / n_u, zero(d), zero(d), zero(d), G, A)
        mse_u = np.sum(d * d) / n_u
    if X_lo is not None and len(X_lo):
        X_lo, X_hi = cast(X_lo).reshape(-1, 2), cast(X_hi).reshape(-1, 2)
        n_b = dt(X_lo.shape[0] if n_b_total is None else n_b_total)
        (hl, pl, _, _), cl = ge._forward(params, X_lo, lbd, s, False)
        (hh, ph, _, _), ch = ge._forward(params, X_hi, lbd, s, False)
        dh, dp = hl - hh, pl - ph
        ge._backward(params, cl, dt(2) * dh / n_b, dt(2) * dp / n_b, zero(dh), zero(dh), G, A)
        ge._backward(params, ch, dt(-2) * dh / n_b, dt(-2) * dp / n_b, zero(dh), zero(dh), G, A)
        mse_b = (np.sum(dh * dh) + np.sum(dp * dp)) / n_b
    flat = lambda T, tail: np.concatenate([np.concatenate([W.ravel(), b.ravel()]) for W, b in T] + [tail])
    grad = flat(G, tail_g)
    assert grad.dtype == np.dtype(dt), grad.dtype
    return mse_f + mse_u + mse_b, grad, flat(A, tail_a), {"f": f, "mse_f": mse_f, "mse_u": mse_u, "mse_b": mse_b}


def loss_grad(theta, layers, lb, ub, X_f, X_u, u, X_lo, X_hi, mask=ALL, n_f_total=None):
    """the float64 oracle -> (loss, gradient, extras)"""
    lo, g, _, ex = restate(theta, layers, lb, ub, X_f, X_u, u, X_lo, X_hi, mask, np.float64, n_f_total)
    return float(lo), g, ex


def residual(theta, layers, lb, ub, X):
    """f at the points X [n, 2] with the current coefficients -> [n, 1]"""
    return restate(theta, layers, lb, ub, X, None, None, None, None)[3]["f"]


def layout(layers):
    """grad_entries.blocks + the six tail entries"""
    out = ge.blocks(layers, "adr_ide")
    nn = n_net(layers)
    return out + [(n, slice(nn + k, nn + k + 1), (1, 1)) for k, n in enumerate(NAMES)]
