"""Data preparation for the heat script (host side, numpy): a rod with one insulated and one cooled end,

    u_t = nu u_xx,   x in [0, 1],   t in [0, 1],   u_x(0, t) = 0,   u_x(1, t) + h u(1, t) = 0,   u(x, 0) = cos(mu x)

with mu the first root of mu tan mu = h in (0, pi / 2).  cos(mu x) is the first eigenfunction of that pair of wall
conditions, so the exact field is one decaying mode,

    u(x, t) = exp(-nu mu^2 t) cos(mu x)

and nothing has to be integrated.  `first_root` finds mu by bisection (mu tan mu - h is increasing on the interval, from -h to
+infinity).  In the engine's "adr" kind the equation is the coefficient set [0, 0, nu, 0, 0, 0]; the walls are Robin points
(Engine.set_robin): (alpha, beta, g) = (0, 1, 0) at x = 0 and (h, 1, 0) at x = 1.
"""
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.append(os.path.join(os.path.dirname(_HERE), "utils"))
from sampling import lhs  # noqa: E402
from plotting import newfig, savefig, saveResultDir  # noqa: E402,F401

NU = 0.1                       # default diffusivity
H = 1.0                        # default heat-transfer coefficient of the wall x = 1
N_X, N_T = 256, 101            # the comparison grid


def adr_coeffs(nu=NU):
    """a0, a1, nu, r1, r2, r3 of the engine's "adr" kind"""
    return (0.0, 0.0, float(nu), 0.0, 0.0, 0.0)


def first_root(h):
    """the root of mu tan mu = h in (0, pi / 2), by bisection down to neighbouring doubles"""
    h = float(h)
    if not (np.isfinite(h) and h > 0.0):
        raise ValueError("h must be positive and finite, got %r" % (h,))
    lo, hi = 0.0, np.nextafter(0.5 * np.pi, 0.0)
    while True:
        mid = 0.5 * (lo + hi)
        if mid <= lo or mid >= hi:
            break
        if mid * np.tan(mid) < h:
            lo = mid
        else:
            hi = mid
    # of the two neighbours, the one with the smaller defect
    return lo if abs(lo * np.tan(lo) - h) <= abs(hi * np.tan(hi) - h) else hi


def exact_solution(x, t, nu=NU, h=H):
    mu = first_root(h)
    return np.exp(-nu * mu * mu * np.asarray(t, dtype=np.float64)) * np.cos(mu * np.asarray(x, dtype=np.float64))


def exact_field(nu=NU, h=H, n_x=N_X, n_t=N_T):
    """x [n_x, 1] (both walls included), t [n_t, 1], Exact_u [n_t, n_x]"""
    x, t = np.linspace(0.0, 1.0, n_x).reshape(-1, 1), np.linspace(0.0, 1.0, n_t).reshape(-1, 1)
    return x, t, exact_solution(x.T, t, nu, h)


def prep_data(N_0, N_w, N_f, nu=NU, h=H):
    """-> x, t, X, T, Exact_u, X_star, u_star, X_u_train (N_0 initial points), u_train, X_f, X_w (2 N_w wall points: the
    wall x = 0, then the wall x = 1), alpha, beta, g (their Robin coefficients), ub, lb.  Draws from numpy's global RNG in
    the order: initial points, times of the wall x = 0, times of the wall x = 1, collocation points."""
    x, t, Exact_u = exact_field(nu, h)
    X, T = np.meshgrid(x, t)
    X_star = np.column_stack((X.ravel(), T.ravel()))
    u_star = Exact_u.reshape(-1, 1)
    lb, ub = np.array([0.0, 0.0]), np.array([1.0, 1.0])

    x0 = np.random.rand(N_0)
    X_u_train = np.column_stack((x0, np.zeros(N_0)))
    u_train = exact_solution(x0, 0.0, nu, h).reshape(-1, 1)
    t_lo, t_hi = np.random.rand(N_w), np.random.rand(N_w)
    X_w = np.vstack([np.column_stack((np.zeros(N_w), t_lo)), np.column_stack((np.ones(N_w), t_hi))])
    alpha = np.concatenate([np.zeros(N_w), np.full(N_w, float(h))])       # insulated | Newton cooling
    beta = np.ones(2 * N_w)
    g = np.zeros(2 * N_w)
    X_f = lb + (ub - lb) * lhs(2, N_f)
    return x, t, X, T, Exact_u, X_star, u_star, X_u_train, u_train, X_f, X_w, alpha, beta, g, ub, lb


def plot_inf_cont_results(X_star, u_pred, X_u_train, X_w, Exact_u, x, t, save_path=None, save_hp=None, weights=None):
    """Headless figure: predicted and exact u(t, x) side by side with the initial and wall points; persisted through
    saveResultDir like the other scripts (`weights`: the trained flat vector, written next to it as weights.npy)."""
    import matplotlib
    matplotlib.use("Agg")
    U_pred = np.asarray(u_pred).reshape(Exact_u.shape)
    fig, _ = newfig(1.0, 1.1)
    fig.clf()
    for i, (field, title) in enumerate(((U_pred, "u(t,x) predicted"), (Exact_u, "u(t,x) exact"))):
        ax = fig.add_subplot(1, 2, i + 1)
        im = ax.imshow(field.T, interpolation="nearest", cmap="rainbow", origin="lower", aspect="auto",
                       extent=[t.min(), t.max(), x.min(), x.max()], vmin=0.0, vmax=1.0)
        if i == 0:
            for P in (X_u_train, X_w):
                if P is not None:
                    ax.plot(P[:, 1], P[:, 0], "kx", markersize=2, clip_on=False)
        ax.set_xlabel("t")
        ax.set_ylabel("x")
        ax.set_title(title)
    fig.colorbar(im)
    if save_path is not None and save_hp is not None:
        saveResultDir(save_path, save_hp, weights=weights)
