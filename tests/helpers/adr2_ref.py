"""numpy restatement of the adr2 kind (PINN_PDE_ADR2, include/pinn_hip.h), in any dtype:

    f   = b u_t + (a0 + a1 u) u_x - nu (u_xx + kappa u_tt) + r1 u + r2 u^2 + r3 u^3 - s
    r_j = alpha_j u + beta_j u_x + gamma_j u_t - g_j                     (three-term wall points)
    L   = mean_f f^2 + mean_u (u - u*)^2 + mean_b [(u_lo - u_hi)^2 + (u_x,lo - u_x,hi)^2] + (1 / N_w) sum_j r_j^2

The four Taylor channels are (h, p, q, r) = (u, u_x, u_t, u_xx + kappa u_tt): the operator d_xx + kappa d_tt passes a tanh layer
as  r = d1 zr + d2 (zp^2 + kappa zq^2)  and a linear layer as u_xx does.  oracle.mlp holds the kappa = 0 sweeps in float64 only,
so this module carries its own; their statements are oracle.mlp's and adr_src_ref's in the same order with every kappa, b and
gamma term added behind, so kappa = 0, b = 1, gamma = 0 returns adr_src_ref.src_loss_grad's values (`==`).
tests/test_adr2_host.py pins the module against torch autograd.

coeffs = (a0, a1, nu, r1, r2, r3, b, kappa).  dtype = np.float32 runs every operation in float32 (the module's own
float32-arithmetic error is what a float32 bound of the GPU tests is measured against)."""
import numpy as np

COEFF_SETS = {
    "adr": (0.3, 1.0, 0.05, 0.2, -0.1, 0.4, 1.0, 0.0),                    # the adr-degenerate vector: b = 1, kappa = 0
    "wave_c2": (0.0, 0.0, 4.0, 0.0, 0.0, 0.0, 0.0, -0.25),                # u_tt = c^2 u_xx, c = 2
    "wave_c02": (0.0, 0.0, 0.04, 0.0, 0.0, 0.0, 0.0, -25.0),              # c = 0.2: kappa = -25
    "telegraph": (0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.3, -1.0),               # the wave row (c = 1) with damping b = 0.3
    "klein_gordon": (0.0, 0.0, 1.0, 1.0, 0.0, 0.5, 0.0, -1.0),            # the wave row with r1 = 1, r3 = 0.5
    "helmholtz": (0.0, 0.0, 1.0, -16.0, 0.0, 0.0, 0.0, 1.0),              # -Laplace u - k^2 u = s, k = 4
    "cdr": (1.5, 0.0, 0.1, 0.0, 0.0, 0.0, -0.7, 1.0),                     # steady convection-diffusion, velocity (a0, b)
    "all": (0.4, -0.8, 0.07, 0.3, -0.2, 0.15, 0.6, -0.35),                # all eight non-zero
}


def layer_shapes(layers):
    return [(layers[i], layers[i + 1]) for i in range(len(layers) - 1)]


def unpack(w, layers, dtype=np.float64):
    w = np.asarray(w, dtype=dtype)
    out, off = [], 0
    for fi, fo in layer_shapes(layers):
        W = w[off:off + fi * fo].reshape(fi, fo)
        off += fi * fo
        b = w[off:off + fo]
        off += fo
        out.append((W, b))
    return out


def pack(params):
    return np.concatenate([np.concatenate([W.ravel(), b.ravel()]) for W, b in params])


def add_grads(ga, gb):
    return [(a[0] + b[0], a[1] + b[1]) for a, b in zip(ga, gb)]


def forward_value(params, X, lb, ub):
    h = 2.0 * (X - lb) / (ub - lb) - 1.0
    for i, (W, b) in enumerate(params):
        h = h @ W + b
        if i < len(params) - 1:
            h = np.tanh(h)
    return h


def value_backward(params, X, lb, ub, out_bar):
    h = 2.0 * (X - lb) / (ub - lb) - 1.0
    acts = []
    L = len(params)
    for i, (W, b) in enumerate(params):
        z = h @ W + b
        a = np.tanh(z) if i < L - 1 else None
        acts.append((h, a))
        h = a if i < L - 1 else z
    grads = [None] * L
    gb = out_bar
    for i in range(L - 1, -1, -1):
        hin, a = acts[i]
        zb = gb if a is None else gb * (1.0 - a * a)
        grads[i] = (hin.T @ zb, zb.sum(axis=0))
        if i > 0:
            gb = zb @ params[i][0].T
    return grads


def taylor_forward(params, X, lb, ub, kappa):
    """-> (H, P, Q, R) of the output layer, R = d2/dx2 + kappa d2/dt2, and the cache of the reverse sweep"""
    s = 2.0 / (ub - lb)
    h = s * (X - lb) - 1.0
    p = np.zeros_like(h)
    q = np.zeros_like(h)
    r = np.zeros_like(h)
    p[:, 0] = s[0]
    q[:, 1] = s[1]
    cache = []
    L = len(params)
    for i, (W, b) in enumerate(params):
        z = h @ W + b
        zp = p @ W
        zq = q @ W
        zr = r @ W
        if i < L - 1:
            a = np.tanh(z)
            d1 = 1.0 - a * a
            d2 = -2.0 * a * d1
            cache.append((h, p, q, r, a, zp, zq, zr))
            h, p, q, r = a, d1 * zp, d1 * zq, d2 * zp * zp + d1 * zr + (kappa * d2 * zq) * zq
        else:
            cache.append((h, p, q, r, None, zp, zq, zr))
            h, p, q, r = z, zp, zq, zr
    return (h, p, q, r), cache


def taylor_backward(params, cache, hb, pb, qb, rb, kappa):
    """reverse sweep from the adjoints of the output channels -> [(dW, db), ...]"""
    L = len(params)
    grads = [None] * L
    for i in range(L - 1, -1, -1):
        W, _ = params[i]
        h, p, q, r, a, zp, zq, zr = cache[i]
        if a is not None:
            d1 = 1.0 - a * a
            d2 = -2.0 * a * d1
            d3 = -2.0 * d1 * (1.0 - 3.0 * a * a)
            zb = d1 * hb + d2 * (zp * pb + zq * qb + zr * rb) + d3 * zp * zp * rb + (kappa * d3 * zq * zq) * rb
            zpb = d1 * pb + 2.0 * d2 * zp * rb
            zqb = d1 * qb + (2.0 * d2 * kappa * zq) * rb
            zrb = d1 * rb
        else:
            zb, zpb, zqb, zrb = hb, pb, qb, rb
        dW = h.T @ zb + p.T @ zpb + q.T @ zqb + r.T @ zrb
        db = zb.sum(axis=0)
        grads[i] = (dW, db)
        if i > 0:
            hb, pb, qb, rb = zb @ W.T, zpb @ W.T, zqb @ W.T, zrb @ W.T
    return grads


def _cast(dtype, *arrays):
    return [None if a is None else np.asarray(a, dtype=dtype) for a in arrays]


def _coeffs(coeffs, dtype):
    c = [dtype(v) for v in coeffs]
    if len(c) != 8:
        raise ValueError("the adr2 kind has eight coefficients (a0, a1, nu, r1, r2, r3, b, kappa), got %d" % len(c))
    return c


def _col(v, n, dtype):
    return np.broadcast_to(np.asarray(v, dtype=dtype).reshape(-1, 1), (n, 1))


def residual(w, layers, lb, ub, X, coeffs, s=None, dtype=np.float64):
    """f at the points X [n, 2] -> [n, 1]; s [n] or None (the operator part N[u])"""
    a0, a1, nu, r1, r2, r3, b, kappa = _coeffs(coeffs, dtype)
    lb, ub, X = _cast(dtype, lb, ub, X)
    (h, p, q, r), _ = taylor_forward(unpack(w, layers, dtype), X, lb, ub, kappa)
    f = b * q + (a0 + a1 * h) * p - nu * r + r1 * h + r2 * h * h + r3 * h * h * h
    return f if s is None else f - np.asarray(s, dtype=dtype).reshape(-1, 1)


def wall_residual(w, layers, lb, ub, X_w, alpha, beta, gamma, g, coeffs, dtype=np.float64):
    """r at the wall points X_w [n, 2] -> [n]"""
    kappa = _coeffs(coeffs, dtype)[7]
    lb, ub, X_w = _cast(dtype, lb, ub, X_w)
    n = X_w.shape[0]
    (h, p, q, _), _ = taylor_forward(unpack(w, layers, dtype), X_w, lb, ub, kappa)
    return (_col(alpha, n, dtype) * h + _col(beta, n, dtype) * p + _col(gamma, n, dtype) * q - _col(g, n, dtype)).ravel()


def adr2_loss_grad(w, layers, lb, ub, X_f, X_u, u, X_lo, X_hi, coeffs, s=None, X_w=None, alpha=None, beta=None, gamma=None,
                   g=None, n_f_total=None, n_u_total=None, n_b_total=None, n_w_total=None, dtype=np.float64):
    """-> (loss, flat gradient, {"f", "mse_f", "mse_u", "mse_b", "mse_w", "r"}); s [N_f] or None, X_u / X_lo / X_w may be None
    or empty"""
    a0, a1, nu, r1, r2, r3, b, kappa = _coeffs(coeffs, dtype)
    lb, ub, X_f, X_u, u, X_lo, X_hi, X_w = _cast(dtype, lb, ub, X_f, X_u, u, X_lo, X_hi, X_w)
    params = unpack(w, layers, dtype)
    N_f = X_f.shape[0] if n_f_total is None else n_f_total
    (h, p, q, r), cache = taylor_forward(params, X_f, lb, ub, kappa)
    f = b * q + (a0 + a1 * h) * p - nu * r + r1 * h + r2 * h * h + r3 * h * h * h
    if s is not None:
        s = np.asarray(s, dtype=dtype).reshape(-1, 1)
        if s.shape != f.shape:
            raise ValueError("s must hold one value per collocation point (%d), got %d" % (f.shape[0], s.size))
        f = f - s
    mse_f = np.sum(f * f) / N_f
    fb = 2.0 * f / N_f
    grads = taylor_backward(params, cache, fb * (a1 * p + r1 + 2.0 * r2 * h + 3.0 * r3 * h * h), fb * (a0 + a1 * h),
                            fb * b, -nu * fb, kappa)
    mse_u = mse_b = 0.0
    if X_u is not None and len(X_u):
        N_u = X_u.shape[0] if n_u_total is None else n_u_total
        d = forward_value(params, X_u, lb, ub) - u.reshape(-1, 1)
        mse_u = np.sum(d * d) / N_u
        grads = add_grads(grads, value_backward(params, X_u, lb, ub, 2.0 * d / N_u))
    if X_lo is not None and len(X_lo):
        N_b = X_lo.shape[0] if n_b_total is None else n_b_total
        (hl, pl, _, _), cl = taylor_forward(params, X_lo, lb, ub, kappa)
        (hu, pu, _, _), cu = taylor_forward(params, X_hi, lb, ub, kappa)
        dh, dp = hl - hu, pl - pu
        mse_b = (np.sum(dh * dh) + np.sum(dp * dp)) / N_b
        z = np.zeros_like(dh)
        grads = add_grads(grads, taylor_backward(params, cl, 2.0 * dh / N_b, 2.0 * dp / N_b, z, z, kappa))
        grads = add_grads(grads, taylor_backward(params, cu, -2.0 * dh / N_b, -2.0 * dp / N_b, z, z, kappa))
    loss, grad = mse_f + mse_u + mse_b, pack(grads)
    ex = {"f": f, "mse_f": mse_f, "mse_u": mse_u, "mse_b": mse_b, "mse_w": 0.0, "r": np.zeros(0)}
    if X_w is None or len(X_w) == 0:
        return loss, grad, ex
    n = X_w.shape[0]
    N_w = n if n_w_total is None else n_w_total
    al, be, ga, gg = (_col(v, n, dtype) for v in (alpha, beta, 0.0 if gamma is None else gamma, g))
    (h, p, q, _), cache = taylor_forward(params, X_w, lb, ub, kappa)
    rw = al * h + be * p + ga * q - gg
    mse_w = np.sum(rw * rw) / N_w
    gw = taylor_backward(params, cache, 2.0 * rw * al / N_w, 2.0 * rw * be / N_w, 2.0 * rw * ga / N_w, np.zeros_like(rw), kappa)
    grad = grad + pack(gw)
    ex["mse_w"], ex["r"] = mse_w, rw.ravel()
    return loss + mse_w, grad, ex
