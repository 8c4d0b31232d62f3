"""Data preparation for the manufactured-solutions script (host side, numpy).  One closed-form field,

    u*(x, t) = exp(-t) sin(pi x) + 0.3 t cos(2 pi x),      x in [-1, 1],   t in [0, 1]        (2-periodic in x)

is made the exact solution of ANY member of the engine's "adr" family

    N[u] = u_t + (a0 + a1 u) u_x - nu u_xx + r1 u + r2 u^2 + r3 u^3 = s(x, t)

by the source s = N[u*], formed here from the closed-form derivatives of u* (Engine.set_source,
NeuralNetwork._set_source).  `EQUATIONS` names the coefficient sets hp["equation"] chooses from; hp["walls"] chooses how the
walls x = -1, 1 are stated: "dirichlet" -- Robin rows (alpha, beta, g) = (1, 0, u*(x, t)) (Engine.set_robin) -- or
"periodic" -- pairs (-1, t) <-> (1, t) (Engine.set_boundary).  The initial data are u*(x, 0) = sin(pi x); the error is taken
against u* itself, so nothing has to be integrated and no reference file is read.
"""
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.append(os.path.join(os.path.dirname(_HERE), "utils"))
from sampling import lhs  # noqa: E402
from plotting import newfig, savefig, saveResultDir  # noqa: E402,F401

# a0, a1, nu, r1, r2, r3 of the engine's "adr" kind
EQUATIONS = {
    "burgers": (0.0, 1.0, 0.01 / np.pi, 0.0, 0.0, 0.0),
    "allen_cahn": (0.0, 0.0, 1e-4, -5.0, 0.0, 5.0),
    "fisher_kpp": (0.0, 0.0, 0.01, -2.0, 2.0, 0.0),
    "advection_diffusion": (0.7, 0.0, 0.05, 0.0, 0.0, 0.0),
    "heat": (0.0, 0.0, 0.1, 0.0, 0.0, 0.0),
}
WALLS = ("dirichlet", "periodic")
N_X, N_T = 256, 101            # the comparison grid
LB, UB = np.array([-1.0, 0.0]), np.array([1.0, 1.0])


def adr_coeffs(equation):
    if equation not in EQUATIONS:
        raise ValueError('hp["equation"] must be one of %s (got %r)' % (sorted(EQUATIONS), equation))
    return tuple(float(v) for v in EQUATIONS[equation])


def exact_channels(x, t):
    """u*, u*_x, u*_t, u*_xx at (x, t) (broadcast)"""
    x, t = np.asarray(x, dtype=np.float64), np.asarray(t, dtype=np.float64)
    e, pi = np.exp(-t), np.pi
    s1, c1, s2, c2 = np.sin(pi * x), np.cos(pi * x), np.sin(2.0 * pi * x), np.cos(2.0 * pi * x)
    u = e * s1 + 0.3 * t * c2
    u_x = pi * e * c1 - 0.6 * pi * t * s2
    u_t = -e * s1 + 0.3 * c2
    u_xx = -pi * pi * e * s1 - 1.2 * pi * pi * t * c2
    return u, u_x, u_t, u_xx


def exact_solution(x, t):
    return exact_channels(x, t)[0]


def source(X, coeffs):
    """s = N[u*] at the rows (x, t) of X [n, 2] -> [n]"""
    X = np.asarray(X, dtype=np.float64).reshape(-1, 2)
    a0, a1, nu, r1, r2, r3 = (float(v) for v in coeffs)
    u, u_x, u_t, u_xx = exact_channels(X[:, 0], X[:, 1])
    return u_t + (a0 + a1 * u) * u_x - nu * u_xx + r1 * u + r2 * u * u + r3 * u * u * u


# variable media (1d-mms/inf_cont_mms_var.py, Engine.set_coef_fields): hp["medium"] names one of these coefficient fields
MEDIA = ("graded_rod", "shear_flow", "graded_reaction")


def medium_fields(X, medium):
    """K [n, 6] = (a0, a1, nu, r1, r2, r3) at the rows (x, t) of X [n, 2]:
      "graded_rod"       u_t - (nu(x) u_x)_x = s with nu(x) = 0.1 (1 + 0.8 tanh 8x): the conservative term is the field nu
                         with the field a0 = -nu'(x) = -0.64 / cosh^2 8x
      "shear_flow"       transport in the prescribed velocity field a0(x, t) = 0.7 + 0.3 sin(pi x) cos(pi t), nu = 0.05
      "graded_reaction"  Allen-Cahn (nu = 1e-4, r3 = 5) with the rate r1(x) = -5 (1 + 0.5 x)"""
    if medium not in MEDIA:
        raise ValueError('hp["medium"] must be one of %s (got %r)' % (list(MEDIA), medium))
    X = np.asarray(X, dtype=np.float64).reshape(-1, 2)
    x, t = X[:, 0], X[:, 1]
    K = np.zeros((X.shape[0], 6))
    if medium == "graded_rod":
        th = np.tanh(8.0 * x)
        K[:, 2] = 0.1 * (1.0 + 0.8 * th)
        K[:, 0] = -0.64 * (1.0 - th * th)
    elif medium == "shear_flow":
        K[:, 0] = 0.7 + 0.3 * np.sin(np.pi * x) * np.cos(np.pi * t)
        K[:, 2] = 0.05
    else:
        K[:, 2] = 1e-4
        K[:, 3] = -5.0 * (1.0 + 0.5 * x)
        K[:, 5] = 5.0
    return K


def source_var(X, K):
    """s = N_K[u*] at the rows (x, t) of X [n, 2] with the rows K [n, 6] of coefficients -> [n]"""
    X = np.asarray(X, dtype=np.float64).reshape(-1, 2)
    K = np.asarray(K, dtype=np.float64)
    if K.shape != (X.shape[0], 6):
        raise ValueError("K must hold one row of six coefficients per point (%d), got shape %s" % (X.shape[0], K.shape))
    a0, a1, nu, r1, r2, r3 = (K[:, j] for j in range(6))
    u, u_x, u_t, u_xx = exact_channels(X[:, 0], X[:, 1])
    return u_t + (a0 + a1 * u) * u_x - nu * u_xx + r1 * u + r2 * u * u + r3 * u * u * u


def exact_field(n_x=N_X, n_t=N_T):
    """x [n_x, 1] (both walls included), t [n_t, 1], Exact_u [n_t, n_x]"""
    x, t = np.linspace(-1.0, 1.0, n_x).reshape(-1, 1), np.linspace(0.0, 1.0, n_t).reshape(-1, 1)
    return x, t, exact_solution(x.T, t)


def prep_data(N_0, N_w, N_f, walls="dirichlet"):
    """-> x, t, X, T, Exact_u, X_star, u_star, X_u_train (N_0 initial points), u_train, X_f, wall, ub, lb.
    wall: walls == "dirichlet": ("dirichlet", X_w, alpha, beta, g) with 2 N_w Robin rows (the wall x = -1, then x = 1),
    (alpha, beta, g) = (1, 0, u*); walls == "periodic": ("periodic", X_lo, X_hi) with N_w pairs.  Draws from numpy's global
    RNG in the order: initial points, wall times (two draws for "dirichlet", one for "periodic"), collocation points."""
    if walls not in WALLS:
        raise ValueError('hp["walls"] must be one of %s (got %r)' % (list(WALLS), walls))
    x, t, Exact_u = exact_field()
    X, T = np.meshgrid(x, t)
    X_star = np.column_stack((X.ravel(), T.ravel()))
    u_star = Exact_u.reshape(-1, 1)
    lb, ub = LB.copy(), UB.copy()

    x0 = lb[0] + (ub[0] - lb[0]) * np.random.rand(N_0)
    X_u_train = np.column_stack((x0, np.zeros(N_0)))
    u_train = exact_solution(x0, 0.0).reshape(-1, 1)
    if walls == "dirichlet":
        t_lo, t_hi = np.random.rand(N_w), np.random.rand(N_w)
        X_w = np.vstack([np.column_stack((np.full(N_w, lb[0]), t_lo)), np.column_stack((np.full(N_w, ub[0]), t_hi))])
        wall = ("dirichlet", X_w, np.ones(2 * N_w), np.zeros(2 * N_w), exact_solution(X_w[:, 0], X_w[:, 1]))
    else:
        tb = np.random.rand(N_w)
        wall = ("periodic", np.column_stack((np.full(N_w, lb[0]), tb)), np.column_stack((np.full(N_w, ub[0]), tb)))
    X_f = lb + (ub - lb) * lhs(2, N_f)
    return x, t, X, T, Exact_u, X_star, u_star, X_u_train, u_train, X_f, wall, ub, lb


def plot_inf_cont_results(X_star, u_pred, X_u_train, X_wall, Exact_u, x, t, save_path=None, save_hp=None, weights=None):
    """Headless figure: predicted and exact u(t, x) side by side with the initial and wall points; persisted through
    saveResultDir like the other scripts (`weights`: the trained flat vector, written next to it as weights.npy)."""
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
            for P in (X_u_train, X_wall):
                if P is not None:
                    ax.plot(P[:, 1], P[:, 0], "kx", markersize=2, clip_on=False)
        ax.set_xlabel("t")
        ax.set_ylabel("x")
        ax.set_title(title)
    fig.colorbar(im)
    if save_path is not None and save_hp is not None:
        saveResultDir(save_path, save_hp, weights=weights)
