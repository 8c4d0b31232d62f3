"""numpy reference of the discrete-time adr family with a dispersion term (pde "adrd_disc", include/pinn_hip.h
PINN_PDE_ADRD_DISC):

    N(U) = (a0 + a1 U) U_x - nu U_xx + d3 U_xxx + r1 U + r2 U^2 + r3 U^3       on the first q outputs,
    theta = [net weights | a0, a1, log nu, r1, r2, r3, d3],     nu = exp(log nu), d3 raw.

oracle/mlp.py carries three x-channels; a third derivative needs a fourth, so the Taylor sweeps of a one-input net are
restated here with (value, d/dx, d2/dx2, d3/dx3).  With a = tanh z, d1 = 1 - a^2, d2 = -2 a d1, d3t = -2 d1 (1 - 3 a^2),
d4 = 8 a d1 (2 - 3 a^2):

    a' = d1 z'      a'' = d2 z'^2 + d1 z''      a''' = d3t z'^3 + 3 d2 z' z'' + d1 z'''

and, (hb, pb, rb, sb) being the adjoints of (a, a', a'', a'''),

    zb   = d1 hb + d2 z' pb + (d3t z'^2 + d2 z'') rb + (d4 z'^3 + 3 d3t z' z'' + d2 z''') sb
    z'b  = d1 pb + 2 d2 z' rb + 3 (d3t z'^2 + d2 z'') sb
    z''b = d1 rb + 3 d2 z' sb
    z'''b = d1 sb.

Stage sets, periodic pairs and terms are tests/helpers/adr_disc_oracle.py's.  The seven tail entries, with dN = 2 R M over
the sets that carry a table:

    a0: sum dN U_x    a1: sum dN U U_x    log nu: -nu sum dN U_xx    r1..r3: sum dN U^k    d3: sum dN U_xxx;

bit k of `mask` clear: entry k is exactly 0.0.  nu_on=False is nu = 0: the operator without the diffusion term, the log nu
slot of theta ignored, its gradient entry exactly 0.0.

Every sweep runs in the dtype asked for (float64 by default), so that the float32 arithmetic error of this very algebra can
be measured against float64 on the cases a test uses.
"""
import numpy as np

import adr_disc_oracle as ado

NAMES = ("a0", "a1", "nu", "r1", "r2", "r3", "d3")
NT = 7
n_net = ado.n_net
table = ado.table


def mask_of(names):
    return sum(1 << NAMES.index(n) for n in names)


def pack(w_net, coef):
    """net weights and the seven RAW coefficients (nu >= 0; nu == 0 leaves 0.0 in the slot, as the engine does) -> theta"""
    c = np.array(coef, dtype=np.float64)
    assert c.shape == (NT,) and c[2] >= 0.0
    c[2] = np.log(c[2]) if c[2] > 0.0 else 0.0
    return np.concatenate([np.asarray(w_net, dtype=np.float64), c])


def coef_of(theta, nu_on=True):
    """the raw coefficients a weight vector holds"""
    c = np.array(theta[-NT:], dtype=np.float64)
    c[2] = np.exp(c[2]) if nu_on else 0.0
    return tuple(c)


def operator(coef, U, U_x, U_xx, U_xxx):
    a0, a1, nu, r1, r2, r3, d3 = coef
    return (a0 + a1 * U) * U_x - nu * U_xx + d3 * U_xxx + r1 * U + r2 * U * U + r3 * U * U * U


# ---- four-channel Taylor sweeps of a one-input net, in the dtype of `params` ---------------------------------------------
def unpack(w, layers, dtype=np.float64):
    w = np.asarray(w, dtype=np.float64)
    out, off = [], 0
    for fi, fo in zip(layers[:-1], layers[1:]):
        out.append((w[off:off + fi * fo].reshape(fi, fo).astype(dtype), w[off + fi * fo:off + fi * fo + fo].astype(dtype)))
        off += fi * fo + fo
    return out


def _map(lb, ub, dtype):
    dt = np.dtype(dtype).type
    lbw = np.asarray(lb, dtype=np.float64).reshape(-1)[0]
    return dt(lbw), dt(2.0 / (np.asarray(ub, dtype=np.float64).reshape(-1)[0] - lbw))


def forward4(params, x, lb, ub):
    """-> ((U, U_x, U_xx, U_xxx) of the output layer, each [n, n_out]), cache"""
    dt = params[0][0].dtype.type
    lbd, s = _map(lb, ub, dt)
    x = np.asarray(x, dtype=np.float64).astype(dt).reshape(-1, 1)
    h = s * (x - lbd) - dt(1)
    p, r, t = np.full_like(h, s), np.zeros_like(h), np.zeros_like(h)
    cache = []
    for i, (W, b) in enumerate(params):
        z, zp, zr, zt = h @ W + b, p @ W, r @ W, t @ W
        if i < len(params) - 1:
            a = np.tanh(z)
            d1 = dt(1) - a * a
            d2 = dt(-2) * a * d1
            d3 = dt(-2) * d1 * (dt(1) - dt(3) * a * a)
            cache.append((h, p, r, t, a, zp, zr, zt))
            h, p, r, t = a, d1 * zp, d2 * zp * zp + d1 * zr, d3 * zp * zp * zp + dt(3) * d2 * zp * zr + d1 * zt
        else:
            cache.append((h, p, r, t, None, zp, zr, zt))
            h, p, r, t = z, zp, zr, zt
    return (h, p, r, t), cache


def backward4(params, cache, hb, pb, rb, sb):
    """reverse sweep; hb..sb: adjoints of the four output channels -> [(dW, db), ...] summed over the points"""
    dt = params[0][0].dtype.type
    grads = [None] * len(params)
    for i in range(len(params) - 1, -1, -1):
        W = params[i][0]
        h, p, r, t, a, zp, zr, zt = cache[i]
        if a is not None:
            d1 = dt(1) - a * a
            d2 = dt(-2) * a * d1
            d3 = dt(-2) * d1 * (dt(1) - dt(3) * a * a)
            d4 = dt(8) * a * d1 * (dt(2) - dt(3) * a * a)
            c2 = d3 * zp * zp + d2 * zr
            zb = d1 * hb + d2 * zp * pb + c2 * rb + (d4 * zp * zp * zp + dt(3) * d3 * zp * zr + d2 * zt) * sb
            zpb = d1 * pb + dt(2) * d2 * zp * rb + dt(3) * c2 * sb
            zrb = d1 * rb + dt(3) * d2 * zp * sb
            ztb = d1 * sb
        else:
            zb, zpb, zrb, ztb = hb, pb, rb, sb
        grads[i] = (h.T @ zb + p.T @ zpb + r.T @ zrb + t.T @ ztb, zb.sum(axis=0))
        if i > 0:
            hb, pb, rb, sb = zb @ W.T, zpb @ W.T, zrb @ W.T, ztb @ W.T
    return grads


def _flat(grads):
    return np.concatenate([np.concatenate([W.ravel(), b.ravel()]) for W, b in grads])


def _coefs(theta, layers, dtype, nu_on):
    dt = np.dtype(dtype).type
    n = n_net(layers)
    a0, a1, lnu, r1, r2, r3, d3 = (dt(v) for v in np.asarray(theta, dtype=np.float64)[n:n + NT])
    return a0, a1, (np.exp(lnu) if nu_on else dt(0)), r1, r2, r3, d3


def stage_prediction(theta, layers, x, lb, ub, M, nu_on=True, dtype=np.float64):
    """U + N(U) M^T at the points x (M None: U itself) -> [n, n_out], all arithmetic in `dtype`"""
    params = unpack(np.asarray(theta)[:n_net(layers)], layers, dtype)
    (h, p, r, t), _ = forward4(params, x, lb, ub)
    if M is None:
        return h
    q = M.shape[1]
    M = np.asarray(M, dtype=np.float64).astype(dtype)
    return h + operator(_coefs(theta, layers, dtype, nu_on), h[:, :q], p[:, :q], r[:, :q], t[:, :q]) @ M.T


def _sweep(theta, layers, lb, ub, sets, periodic, nu_on, dtype):
    """-> (terms [3], net gradient, seven unmasked tail entries, their scales A [7] in float64), all arithmetic in `dtype`"""
    dt = np.dtype(dtype).type
    theta = np.asarray(theta, dtype=np.float64)
    params = unpack(theta[:n_net(layers)], layers, dt)
    coef = _coefs(theta, layers, dt, nu_on)
    a0, a1, nu, r1, r2, r3, d3 = coef
    g_net = np.zeros(n_net(layers), dtype=dt)
    terms = [dt(0), dt(0), dt(0)]
    g, A = np.zeros(NT, dtype=dt), np.zeros(NT)
    for s, st in enumerate(sets):
        if st is None or len(st[0]) == 0:
            continue
        x, target, M = st
        (h, p, r, t), cache = forward4(params, x, lb, ub)
        pred = h
        if M is not None:
            M = np.asarray(M, dtype=np.float64).astype(dt)
            q = M.shape[1]
            U, U_x, U_xx, U_xxx = h[:, :q], p[:, :q], r[:, :q], t[:, :q]
            pred = h + operator(coef, U, U_x, U_xx, U_xxx) @ M.T
        res = pred - np.asarray(target, dtype=np.float64).astype(dt).reshape(-1, 1)
        terms[s] = np.sum(res * res)
        hb = dt(2) * res
        pb, rb, sb = np.zeros_like(res), np.zeros_like(res), np.zeros_like(res)
        if M is not None:
            dN = (dt(2) * res) @ M
            hb[:, :q] += dN * (a1 * U_x + r1 + dt(2) * r2 * U + dt(3) * r3 * U * U)
            pb[:, :q] = dN * (a0 + a1 * U)
            rb[:, :q] = -nu * dN
            sb[:, :q] = d3 * dN
            parts = [dN * U_x, dN * U * U_x, -nu * dN * U_xx, dN * U, dN * U * U, dN * U * U * U, dN * U_xxx]
            for k, v in enumerate(parts):
                g[k] += np.sum(v)
                A[k] += float(np.sum(np.abs(v).astype(np.float64)))
        g_net = g_net + _flat(backward4(params, cache, hb, pb, rb, sb))
    if periodic is not None and len(periodic[0]) > 0:
        x_lb, x_ub, order = periodic
        assert order in (0, 1) and len(x_lb) == len(x_ub)
        (hl, pl, _, _), cl = forward4(params, x_lb, lb, ub)
        (hu, pu, _, _), cu = forward4(params, x_ub, lb, ub)
        d = hl - hu
        dx = (pl - pu) if order == 1 else np.zeros_like(d)
        terms[2] = np.sum(d * d) + np.sum(dx * dx)
        z = np.zeros_like(d)
        g_net = g_net + _flat(backward4(params, cl, dt(2) * d, dt(2) * dx, z, z))
        g_net = g_net + _flat(backward4(params, cu, dt(-2) * d, dt(-2) * dx, z, z))
    if not nu_on:
        g[2], A[2] = dt(0), 0.0
    assert g.dtype == np.dtype(dt) and g_net.dtype == np.dtype(dt)
    return terms, g_net, g, A


def tail(theta, layers, lb, ub, sets, dtype=np.float64, nu_on=True):
    """-> (seven unmasked tail entries in `dtype`, their scales A [7] in float64)"""
    _, _, g, A = _sweep(theta, layers, lb, ub, sets, None, nu_on, dtype)
    return g, A


def loss_grad(theta, layers, lb, ub, sets, periodic=None, mask=127, nu_on=True, dtype=np.float64):
    """-> (loss, flat gradient [n_net + 7], {"terms": [set 0, set 1, periodic]}), returned as float64 whatever `dtype`"""
    terms, g_net, g, _ = _sweep(theta, layers, lb, ub, sets, periodic, nu_on, dtype)
    g = np.where([(mask >> k) & 1 for k in range(NT)], g.astype(np.float64), 0.0)
    terms = [float(v) for v in terms]
    return float(terms[0] + terms[1] + terms[2]), np.concatenate([g_net.astype(np.float64), g]), {"terms": terms}


def adam_losses(theta, layers, lb, ub, sets, periodic, mask, n, lr, b1, b2, eps, nu_on=True):
    """the loss before each of n Adam steps (oracle/optim.py's update) -> (losses [n], theta after them)"""
    from oracle import optim
    opt = optim.Adam(lr, b1, b2, eps)
    theta = np.array(theta, dtype=np.float64)
    losses = []
    for _ in range(n):
        lo, g, _ = loss_grad(theta, layers, lb, ub, sets, periodic, mask, nu_on)
        losses.append(lo)
        theta = opt.step(theta, g)
    return np.array(losses), theta


# ---- inputs shared by the host and the GPU tests ------------------------------------------------------------------------
def coefficient_vectors(seed=7):
    """eight vectors: one unit coefficient each over nu = 0.1 (the nu vector is nu = 1 alone), then all seven random in
    [-1, 1] with nu > 0 -- a wrong derivative of one term cannot hide behind the others"""
    out = []
    for k in range(NT):
        c = np.zeros(NT)
        c[2] = 0.1
        c[k] = 1.0
        out.append(tuple(c))
    rs = np.random.RandomState(seed)
    c = rs.uniform(-1.0, 1.0, NT)
    c[2] = abs(c[2]) + 0.01
    out.append(tuple(c))
    return out


def case(layers, q, n0, n1, n_pairs, seed, coef, lb=-1.0, ub=1.0, wscale=0.5):
    """adr_disc_oracle.case with a table on BOTH sets (set 1: minus a second draw) -> (sets, pairs (x_lb, x_ub), theta)"""
    sets, pairs, w = ado.case(layers, q, n0, n1, n_pairs, seed, lb, ub, wscale)
    if sets[1] is not None:
        rs = np.random.RandomState(seed + 5000)
        sets[1] = (sets[1][0], sets[1][1], -table(q, layers[-1], rs.uniform(0.2, 0.6), rs))
    return sets, pairs, pack(w, coef)
