"""numpy reference of the discrete-time adr kind with trainable coefficients (pde "adr_disc_ide", include/pinn_hip.h
PINN_PDE_ADR_DISC_IDE): tests/helpers/adr_disc_oracle.py with the coefficients read from the tail of the weight vector,

    theta = [net weights | a0, a1, log nu, r1, r2, r3],     nu = exp(log nu),

and six more gradient entries.  With dN = 2 R M ([point, column], columns j < q) summed over the stage sets that carry a
table, each with its own,

    dL/da0 = sum dN U_x      dL/da1 = sum dN U U_x      dL/dlog nu = -nu sum dN U_xx
    dL/dr1 = sum dN U        dL/dr2 = sum dN U^2        dL/dr3 = sum dN U^3;

periodic pairs and sets without a table add nothing.  Bit k of `mask` clear: entry k is exactly 0.0.  The loss, the terms
and the net entries are adr_disc_oracle's at the tail's coefficients.

tail(theta, ..., dtype) forms the six entries with ALL arithmetic in `dtype` and their scales A_k = sum |dN dN/dp_k|, the
yardstick tests/helpers/grad_entries.py judges a tail entry by (plain error of the compute type against the wider one).
"""
import numpy as np

import adr_disc_oracle as ado

NAMES = ("a0", "a1", "nu", "r1", "r2", "r3")
n_net = ado.n_net


def mask_of(names):
    return sum(1 << NAMES.index(n) for n in names)


def pack(w_net, coef):
    """net weights and RAW coefficients (nu > 0) -> theta"""
    c = np.array(coef, dtype=np.float64)
    assert c.shape == (6,) and c[2] > 0.0
    c[2] = np.log(c[2])
    return np.concatenate([np.asarray(w_net, dtype=np.float64), c])


def coef_of(theta):
    """the raw coefficients a weight vector holds"""
    c = np.array(theta[-6:], dtype=np.float64)
    c[2] = np.exp(c[2])
    return tuple(c)


def _forward1(params, x, lb, s):
    """oracle.mlp.taylor_forward for a one-input net, (value, d/dx, d2/dx2), in the dtype of `params`"""
    dt = params[0][0].dtype.type
    h = s * (x - lb) - dt(1)
    p, r = np.full_like(h, s), np.zeros_like(h)
    for i, (W, b) in enumerate(params):
        z, zp, zr = h @ W + b, p @ W, r @ W
        if i < len(params) - 1:
            a = np.tanh(z)
            d1 = dt(1) - a * a
            h, p, r = a, d1 * zp, dt(-2) * a * d1 * zp * zp + d1 * zr
        else:
            h, p, r = z, zp, zr
    return h, p, r


def tail(theta, layers, lb, ub, sets, dtype=np.float64):
    """-> (six unmasked tail entries in `dtype`, their scales A [6] in float64); points, targets, tables and weights are
    cast first, as the engine does"""
    dt = np.dtype(dtype).type
    wide = np.longdouble if dt is np.longdouble else np.float64
    lbw = np.asarray(lb, dtype=wide).reshape(-1)[0]
    s = dt(2 / (np.asarray(ub, dtype=wide).reshape(-1)[0] - lbw))
    lbd = dt(lbw)
    theta = np.asarray(theta, dtype=np.float64)
    n = n_net(layers)
    params, off = [], 0
    for fi, fo in zip(layers[:-1], layers[1:]):
        params.append((theta[off:off + fi * fo].reshape(fi, fo).astype(dt), theta[off + fi * fo:off + fi * fo + fo].astype(dt)))
        off += fi * fo + fo
    a0, a1, lnu, r1, r2, r3 = (dt(v) for v in theta[n:n + 6])
    nu = np.exp(lnu)
    g, A = np.zeros(6, dtype=dt), np.zeros(6)
    for st in sets:
        if st is None or len(st[0]) == 0 or st[2] is None:
            continue
        x, target, M = (np.asarray(v, dtype=np.float64).astype(dt) for v in st)
        q = M.shape[1]
        h, p, r = _forward1(params, x.reshape(-1, 1), lbd, s)
        U, U_x, U_xx = h[:, :q], p[:, :q], r[:, :q]
        N = (a0 + a1 * U) * U_x - nu * U_xx + r1 * U + r2 * U * U + r3 * U * U * U
        R = h + N @ M.T - target.reshape(-1, 1)
        dN = (dt(2) * R) @ M
        parts = [dN * U_x, dN * U * U_x, -nu * dN * U_xx, dN * U, dN * U * U, dN * U * U * U]
        for k, t in enumerate(parts):
            g[k] += np.sum(t)
            A[k] += float(np.sum(np.abs(t).astype(np.float64)))
    assert g.dtype == np.dtype(dt)
    return g, A


def loss_grad(theta, layers, lb, ub, sets, periodic=None, mask=63):
    """-> (loss, flat gradient [n_net + 6], {"terms": [set 0, set 1, periodic]})"""
    theta = np.asarray(theta, dtype=np.float64)
    loss, g_net, ex = ado.loss_grad(theta[:-6], layers, lb, ub, sets, coef_of(theta), periodic)
    t, _ = tail(theta, layers, lb, ub, sets)
    t = np.where([(mask >> k) & 1 for k in range(6)], t, 0.0)
    return loss, np.concatenate([g_net, t]), ex


def adam_losses(theta, layers, lb, ub, sets, periodic, mask, n, lr, b1, b2, eps):
    """the loss before each of n Adam steps (oracle/optim.py's update) -> (losses [n], theta after them)"""
    from oracle import optim
    opt = optim.Adam(lr, b1, b2, eps)
    theta = np.array(theta, dtype=np.float64)
    losses = []
    for _ in range(n):
        lo, g, _ = loss_grad(theta, layers, lb, ub, sets, periodic, mask)
        losses.append(lo)
        theta = opt.step(theta, g)
    return np.array(losses), theta


def case(layers, q, n0, n1, n_pairs, seed, coef, lb=-1.0, ub=1.0, wscale=0.5):
    """adr_disc_oracle.case with a table on BOTH sets (set 1: minus a second draw, as the t_1 snapshot of an identification
    carries -dt (b - A)) -> (sets, pairs (x_lb, x_ub), theta)"""
    sets, pairs, w = ado.case(layers, q, n0, n1, n_pairs, seed, lb, ub, wscale)
    if sets[1] is not None:
        rs = np.random.RandomState(seed + 5000)
        sets[1] = (sets[1][0], sets[1][1], -ado.table(q, layers[-1], rs.uniform(0.2, 0.6), rs))
    return sets, pairs, pack(w, coef)
