"""Data preparation for the steady two-dimensional script (host side, numpy): the Helmholtz problem

    -Laplace u - k^2 u = s(x, y)   on [-1, 1]^2,     u = 0 on the walls,     u*(x, y) = sin(pi x) sin(4 pi y),

with s = (17 pi^2 - k^2) u*.  The net's second input plays the role of y: the engine's "adr2" kind

    b u_t + (a0 + a1 u) u_x - nu (u_xx + kappa u_tt) + r1 u + r2 u^2 + r3 u^3 = s

with b = 0, nu = 1, kappa = 1, r1 = -k^2 carries the Laplacian as one Taylor channel.  The walls are data points.
"""
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.append(os.path.join(os.path.dirname(_HERE), "utils"))
from sampling import lhs  # noqa: E402
from plotting import newfig, savefig, saveResultDir  # noqa: E402,F401

N_X, N_Y = 201, 201            # the comparison grid
LB, UB = np.array([-1.0, -1.0]), np.array([1.0, 1.0])


def adr2_coeffs(k):
    """a0, a1, nu, r1, r2, r3, b, kappa of the engine's "adr2" kind"""
    k = float(k)
    return (0.0, 0.0, 1.0, -k * k, 0.0, 0.0, 0.0, 1.0)


def exact_solution(x, y):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return np.sin(np.pi * x) * np.sin(4.0 * np.pi * y)


def source(X, k):
    """s = -Laplace u* - k^2 u* at the rows (x, y) of X [n, 2] -> [n]"""
    X = np.asarray(X, dtype=np.float64).reshape(-1, 2)
    return (17.0 * np.pi * np.pi - float(k) ** 2) * exact_solution(X[:, 0], X[:, 1])


def prep_data(N_w, N_f):
    """-> x, y, Exact_u, X_star, u_star, X_u_train (N_w points on each of the four walls), u_train, X_f, ub, lb.  Draws from
    numpy's global RNG in the order: the walls x = -1, x = 1, y = -1, y = 1, then the collocation points."""
    x, y = np.linspace(-1.0, 1.0, N_X).reshape(-1, 1), np.linspace(-1.0, 1.0, N_Y).reshape(-1, 1)
    Exact_u = exact_solution(x.T, y)
    X, Y = np.meshgrid(x, y)
    X_star = np.column_stack((X.ravel(), Y.ravel()))
    u_star = Exact_u.reshape(-1, 1)
    lb, ub = LB.copy(), UB.copy()
    e = [lb[0] + (ub[0] - lb[0]) * np.random.rand(N_w) for _ in range(4)]
    X_u_train = np.vstack([np.column_stack((np.full(N_w, lb[0]), e[0])), np.column_stack((np.full(N_w, ub[0]), e[1])),
                           np.column_stack((e[2], np.full(N_w, lb[1]))), np.column_stack((e[3], np.full(N_w, ub[1])))])
    u_train = exact_solution(X_u_train[:, 0], X_u_train[:, 1]).reshape(-1, 1)
    X_f = lb + (ub - lb) * lhs(2, N_f)
    return x, y, Exact_u, X_star, u_star, X_u_train, u_train, X_f, ub, lb


def plot_results(u_pred, X_u_train, Exact_u, x, y, save_path=None, save_hp=None, weights=None):
    """Headless figure: predicted and exact u(x, y) side by side with the wall points"""
    import matplotlib
    matplotlib.use("Agg")
    U_pred = np.asarray(u_pred).reshape(Exact_u.shape)
    fig, _ = newfig(1.0, 1.1)
    fig.clf()
    lo, hi = float(Exact_u.min()), float(Exact_u.max())
    for i, (field, title) in enumerate(((U_pred, "u(x,y) predicted"), (Exact_u, "u(x,y) exact"))):
        ax = fig.add_subplot(1, 2, i + 1)
        im = ax.imshow(field, interpolation="nearest", cmap="rainbow", origin="lower", aspect="auto",
                       extent=[x.min(), x.max(), y.min(), y.max()], vmin=lo, vmax=hi)
        if i == 0:
            ax.plot(X_u_train[:, 0], X_u_train[:, 1], "kx", markersize=2, clip_on=False)
        ax.set_xlabel("x")
        ax.set_ylabel("y")
        ax.set_title(title)
    fig.colorbar(im)
    if save_path is not None and save_hp is not None:
        saveResultDir(save_path, save_hp, weights=weights)
