"""numpy float64 reference of the discrete-time adr kind (pde "adr_disc", include/pinn_hip.h PINN_PDE_ADR_DISC), on the
Taylor-mode forward and reverse sweeps of oracle/mlp.py.

A stage set is (x [n,1], target [n,1], M [n_out,q] or None), as in oracle/disc.py, and contributes
    sum((U + N(U[:, :q]) M^T - target)^2),     N(U) = (a0 + a1 U) U_x - nu U_xx + r1 U + r2 U^2 + r3 U^3
with coef = (a0, a1, nu, r1, r2, r3).  With dN = 2 R M the adjoints of the output channels are
    g_U = 2 R + dN (a1 U_x + r1 + 2 r2 U + 3 r3 U^2),   g_Ux = dN (a0 + a1 U),   g_Uxx = -nu dN.
A periodic set is (x_lb [n], x_ub [n], order) and contributes, over ALL outputs,
    sum((U(x_lb) - U(x_ub))^2)  [+ sum((U_x(x_lb) - U_x(x_ub))^2) when order == 1].
`sets` is always the pair [set 0, set 1]; an entry that is None or has no points is absent.  terms = [set 0, set 1,
periodic], as Engine.loss_grad reports them.
"""
import numpy as np

from oracle import mlp

BURGERS = (0.0, 1.0, 0.01 / np.pi, 0.0, 0.0, 0.0)       # what a new context holds


def operator(coef, U, U_x, U_xx):
    a0, a1, nu, r1, r2, r3 = coef
    return (a0 + a1 * U) * U_x - nu * U_xx + r1 * U + r2 * U * U + r3 * U * U * U


def _bounds(lb, ub):
    return np.asarray(lb, dtype=np.float64).reshape(-1), np.asarray(ub, dtype=np.float64).reshape(-1)


def _present(s):
    return s is not None and len(s[0]) > 0


def stage_prediction(params, x, lb, ub, M, coef):
    """U + N(U) M^T at the points x [n,1] (M None: U itself) -> [n, n_out]"""
    lb, ub = _bounds(lb, ub)
    (h, p, _, r), _ = mlp.taylor_forward(params, np.asarray(x, dtype=np.float64).reshape(-1, 1), lb, ub)
    if M is None:
        return h
    q = M.shape[1]
    return h + operator(coef, h[:, :q], p[:, :q], r[:, :q]) @ M.T


def loss_grad(w, layers, lb, ub, sets, coef, periodic=None):
    """-> (loss, flat gradient, {"terms": [set 0, set 1, periodic]})"""
    lb, ub = _bounds(lb, ub)
    a0, a1, nu, r1, r2, r3 = (float(v) for v in coef)
    params = mlp.unpack(np.asarray(w, dtype=np.float64), layers)
    grads = [(np.zeros_like(W), np.zeros_like(b)) for W, b in params]
    terms = [0.0, 0.0, 0.0]
    for s, st in enumerate(sets):
        if not _present(st):
            continue
        x, target, M = st
        (h, p, _, r), cache = mlp.taylor_forward(params, np.asarray(x, dtype=np.float64).reshape(-1, 1), lb, ub)
        pred = h
        if M is not None:
            q = M.shape[1]
            U, U_x, U_xx = h[:, :q], p[:, :q], r[:, :q]
            pred = h + operator(coef, U, U_x, U_xx) @ M.T
        res = pred - np.asarray(target, dtype=np.float64).reshape(-1, 1)
        terms[s] = float(np.sum(res * res))
        hb, pb, rb = 2.0 * res, np.zeros_like(res), np.zeros_like(res)
        if M is not None:
            dN = (2.0 * res) @ M
            hb[:, :q] += dN * (a1 * U_x + r1 + 2.0 * r2 * U + 3.0 * r3 * U * U)
            pb[:, :q] = dN * (a0 + a1 * U)
            rb[:, :q] = -nu * dN
        grads = mlp.add_grads(grads, mlp.taylor_backward(params, cache, hb, pb, np.zeros_like(res), rb))
    if periodic is not None and len(periodic[0]) > 0:
        x_lb, x_ub, order = periodic
        assert order in (0, 1) and len(x_lb) == len(x_ub)
        (hl, pl, _, _), cl = mlp.taylor_forward(params, np.asarray(x_lb, dtype=np.float64).reshape(-1, 1), lb, ub)
        (hu, pu, _, _), cu = mlp.taylor_forward(params, np.asarray(x_ub, dtype=np.float64).reshape(-1, 1), lb, ub)
        d = hl - hu
        dx = (pl - pu) if order == 1 else np.zeros_like(d)
        terms[2] = float(np.sum(d * d) + np.sum(dx * dx))
        z = np.zeros_like(d)
        grads = mlp.add_grads(grads, mlp.taylor_backward(params, cl, 2.0 * d, 2.0 * dx, z, z))
        grads = mlp.add_grads(grads, mlp.taylor_backward(params, cu, -2.0 * d, -2.0 * dx, z, z))
    return terms[0] + terms[1] + terms[2], mlp.pack(grads), {"terms": terms}


def adam_losses(w, layers, lb, ub, sets, coef, periodic, n, lr, b1, b2, eps):
    """the loss before each of n Adam steps (oracle/optim.py's update) -> (losses [n], weights after them)"""
    from oracle import optim
    opt = optim.Adam(lr, b1, b2, eps)
    w = np.array(w, dtype=np.float64)
    losses = []
    for _ in range(n):
        lo, g, _ = loss_grad(w, layers, lb, ub, sets, coef, periodic)
        losses.append(lo)
        w = opt.step(w, g)
    return np.array(losses), w


# ---- inputs shared by the host and the GPU tests ------------------------------------------------------------------------
def coefficient_vectors(seed=7):
    """six vectors with one unit coefficient each and nu = 0.1 kept on (the nu vector is nu = 1 alone), then one with all
    six random in [-1, 1] and nu > 0: a wrong derivative of one term cannot hide behind the others"""
    out = []
    for k in range(6):
        c = np.zeros(6)
        c[2] = 0.1
        c[k] = 1.0
        out.append(tuple(c))
    rs = np.random.RandomState(seed)
    c = rs.uniform(-1.0, 1.0, 6)
    c[2] = abs(c[2]) + 0.01
    out.append(tuple(c))
    return out


REACTION_HEAVY = (0.3, -0.7, 0.05, -5.0, 1.5, 5.0)


def n_net(layers):
    return sum(a * b + b for a, b in zip(layers[:-1], layers[1:]))


def table(q, n_out, dt, rs=None):
    """dt [A; b] cut or extended to n_out rows (rows beyond q + 1: random, as tests/helpers/disc_cases.py builds them)"""
    from oracle import disc
    A, b, _ = disc.gauss_legendre_butcher(q)
    T = np.vstack([A, b[None, :]])
    if n_out > q + 1:
        T = np.vstack([T, (rs or np.random.RandomState(0)).standard_normal((n_out - q - 1, q)) / q])
    return dt * T[:n_out]


def case(layers, q, n0, n1, n_pairs, seed, lb=-1.0, ub=1.0, wscale=0.5):
    """-> (sets [set 0 with a table, set 1 without], pairs (x_lb, x_ub), flat weights).  The pairs are the walls first, then
    inner pairs a fixed distance apart, so that a kernel which mixed up rows would not cancel."""
    rs = np.random.RandomState(seed)
    M = table(q, layers[-1], rs.uniform(0.2, 0.6), rs)
    x0, x1 = rs.uniform(lb, ub, (n0, 1)), rs.uniform(lb, ub, (n1, 1))
    t0, t1 = -np.sin(np.pi * x0) + 0.1 * rs.standard_normal((n0, 1)), 0.1 * rs.standard_normal((n1, 1))
    sets = [(x0, t0, M) if n0 else None, (x1, t1, None) if n1 else None]
    x_lb = np.concatenate([[lb], rs.uniform(lb, 0.5 * (lb + ub), max(n_pairs - 1, 0))])[:n_pairs]
    x_ub = np.concatenate([[ub], x_lb[1:] + 0.5 * (ub - lb)])[:n_pairs]
    w = wscale * rs.standard_normal(n_net(layers))
    return sets, (x_lb, x_ub), w
