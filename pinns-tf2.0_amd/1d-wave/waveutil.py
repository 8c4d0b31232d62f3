"""Data preparation for the second-order-in-time script (host side, numpy).  One closed-form standing wave,

    u*(x, t) = sin(pi x) cos(c pi t) + 0.5 sin(2 pi x) cos(2 c pi t),      x in [-1, 1],   t in [0, 1],

solves u_tt = c^2 u_xx with zero walls, the initial displacement u*(x, 0) and zero initial velocity.  The engine's "adr2" kind

    b u_t + (a0 + a1 u) u_x - nu (u_xx + kappa u_tt) + r1 u + r2 u^2 + r3 u^3 = s(x, t)

states it with nu = c^2, kappa = -1 / c^2, b = 0 (`EQUATIONS`): "wave" needs no source, "telegraph" (damping b) and
"klein_gordon" (r1, r3) take the manufactured source s = b u*_t + r1 u* + r3 u*^3, formed here from closed forms -- the wave
operator itself vanishes on u*.  The walls and the initial displacement are data points; the initial velocity is a set of
three-term wall points (alpha, beta, gamma, g) = (0, 0, 1, 0) (Engine.set_robin3).
"""
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.append(os.path.join(os.path.dirname(_HERE), "utils"))
from sampling import lhs  # noqa: E402
from plotting import newfig, savefig, saveResultDir  # noqa: E402,F401

C = 1.0                                           # wave speed
# a0, a1, nu, r1, r2, r3, b, kappa of the engine's "adr2" kind
EQUATIONS = {
    "wave": (0.0, 0.0, C * C, 0.0, 0.0, 0.0, 0.0, -1.0 / (C * C)),
    "telegraph": (0.0, 0.0, C * C, 0.0, 0.0, 0.0, 0.3, -1.0 / (C * C)),
    "klein_gordon": (0.0, 0.0, C * C, 1.0, 0.0, 0.5, 0.0, -1.0 / (C * C)),
}
N_X, N_T = 256, 101            # the comparison grid
LB, UB = np.array([-1.0, 0.0]), np.array([1.0, 1.0])


def adr2_coeffs(equation):
    if equation not in EQUATIONS:
        raise ValueError('hp["equation"] must be one of %s (got %r)' % (sorted(EQUATIONS), equation))
    return tuple(float(v) for v in EQUATIONS[equation])


def exact_solution(x, t):
    x, t = np.asarray(x, dtype=np.float64), np.asarray(t, dtype=np.float64)
    return np.sin(np.pi * x) * np.cos(C * np.pi * t) + 0.5 * np.sin(2.0 * np.pi * x) * np.cos(2.0 * C * np.pi * t)


def exact_velocity(x, t):
    """u*_t"""
    x, t = np.asarray(x, dtype=np.float64), np.asarray(t, dtype=np.float64)
    return -C * np.pi * (np.sin(np.pi * x) * np.sin(C * np.pi * t) + np.sin(2.0 * np.pi * x) * np.sin(2.0 * C * np.pi * t))


def source(X, equation):
    """s = N[u*] at the rows (x, t) of X [n, 2] -> [n]: the terms beside the wave operator, which is zero on u*"""
    X = np.asarray(X, dtype=np.float64).reshape(-1, 2)
    _, _, _, r1, r2, r3, b, _ = adr2_coeffs(equation)
    u, u_t = exact_solution(X[:, 0], X[:, 1]), exact_velocity(X[:, 0], X[:, 1])
    return b * u_t + r1 * u + r2 * u * u + r3 * u * u * u


def prep_data(N_0, N_w, N_f):
    """-> x, t, Exact_u, X_star, u_star, X_u_train (N_0 initial points, then N_w points on each wall), u_train, X_v (N_0
    points on t = 0 for the initial velocity), X_f, ub, lb.  Draws from numpy's global RNG in the order: initial points, wall
    times (two draws), velocity points, collocation points."""
    x, t = np.linspace(-1.0, 1.0, N_X).reshape(-1, 1), np.linspace(0.0, 1.0, N_T).reshape(-1, 1)
    Exact_u = exact_solution(x.T, t)
    X, T = np.meshgrid(x, t)
    X_star = np.column_stack((X.ravel(), T.ravel()))
    u_star = Exact_u.reshape(-1, 1)
    lb, ub = LB.copy(), UB.copy()
    x0 = lb[0] + (ub[0] - lb[0]) * np.random.rand(N_0)
    t_lo, t_hi = np.random.rand(N_w), np.random.rand(N_w)
    X_u_train = np.vstack([np.column_stack((x0, np.zeros(N_0))), np.column_stack((np.full(N_w, lb[0]), t_lo)),
                           np.column_stack((np.full(N_w, ub[0]), t_hi))])
    u_train = exact_solution(X_u_train[:, 0], X_u_train[:, 1]).reshape(-1, 1)
    X_v = np.column_stack((lb[0] + (ub[0] - lb[0]) * np.random.rand(N_0), np.zeros(N_0)))
    X_f = lb + (ub - lb) * lhs(2, N_f)
    return x, t, Exact_u, X_star, u_star, X_u_train, u_train, X_v, X_f, ub, lb


def plot_results(u_pred, X_u_train, Exact_u, x, t, save_path=None, save_hp=None, weights=None):
    """Headless figure: predicted and exact u(t, x) side by side with the data points"""
    import matplotlib
    matplotlib.use("Agg")
    U_pred = np.asarray(u_pred).reshape(Exact_u.shape)
    fig, _ = newfig(1.0, 1.1)
    fig.clf()
    lo, hi = float(Exact_u.min()), float(Exact_u.max())
    for i, (field, title) in enumerate(((U_pred, "u(t,x) predicted"), (Exact_u, "u(t,x) exact"))):
        ax = fig.add_subplot(1, 2, i + 1)
        im = ax.imshow(field.T, interpolation="nearest", cmap="rainbow", origin="lower", aspect="auto",
                       extent=[t.min(), t.max(), x.min(), x.max()], vmin=lo, vmax=hi)
        if i == 0:
            ax.plot(X_u_train[:, 1], X_u_train[:, 0], "kx", markersize=2, clip_on=False)
        ax.set_xlabel("t")
        ax.set_ylabel("x")
        ax.set_title(title)
    fig.colorbar(im)
    if save_path is not None and save_hp is not None:
        saveResultDir(save_path, save_hp, weights=weights)
