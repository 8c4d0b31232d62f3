"""Data preparation for the Allen-Cahn script (host side, numpy):

    u_t - 1e-4 u_xx + 5 u^3 - 5 u = 0,   x in [-1, 1] periodic,   t in [0, 1],   u(x, 0) = x^2 cos(pi x)

The exact field is not read from a file: `solve_allen_cahn` integrates the equation with a Fourier split-step scheme (Strang
splitting: half a reaction step, a diffusion step, half a reaction step).  Diffusion is exact in Fourier space and the
reaction u' = 5 u - 5 u^3 has the closed form u / sqrt(u^2 + (1 - u^2) exp(-10 dt)), so the only errors are the
splitting's (second order in dt) and the truncation of the spectrum.  The initial condition has a kink at the periodic seam
(u_x(-1) = 2, u_x(1) = -2), so space converges algebraically: the field is solved on N_SOLVE = 4096 modes and subsampled to
the 512 x 201 grid the script compares against (tests/test_adr_host.py pins both convergence rates).  `exact_field` caches
the result beside the script's results.
"""
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.append(os.path.join(os.path.dirname(_HERE), "utils"))
from sampling import lhs  # noqa: E402
from plotting import newfig, savefig, saveResultDir  # noqa: E402,F401

NU = 1e-4                      # diffusion coefficient
RHO = 5.0                      # reaction rate: u_t = NU u_xx + RHO (u - u^3)
ADR_COEFFS = (0.0, 0.0, NU, -RHO, 0.0, RHO)      # a0, a1, nu, r1, r2, r3 of the engine's "adr" kind
N_X, N_T = 512, 201            # the comparison grid
N_SOLVE, SUBSTEPS = 4096, 50   # the solver's modes and substeps per output time


def initial_condition(x):
    x = np.asarray(x, dtype=np.float64)
    return x * x * np.cos(np.pi * x)


def solve_allen_cahn(n_modes=N_SOLVE, n_t=N_T, substeps=SUBSTEPS, t_end=1.0, nu=NU, rho=RHO):
    """-> x [n_modes] (= -1 + 2 i / n_modes, the wall x = 1 is the image of x = -1), t [n_t], U [n_t, n_modes]"""
    x = -1.0 + 2.0 * np.arange(n_modes) / n_modes
    t = np.linspace(0.0, t_end, n_t)
    dt = (t[1] - t[0]) / substeps
    k = np.pi * np.fft.rfftfreq(n_modes, d=1.0 / n_modes)          # wave numbers of the period 2
    diffuse = np.exp(-nu * k * k * dt)
    e_half = np.exp(-2.0 * rho * (0.5 * dt))

    def react_half(u):
        return u / np.sqrt(u * u + (1.0 - u * u) * e_half)

    u = initial_condition(x)
    U = np.empty((n_t, n_modes))
    U[0] = u
    for i in range(1, n_t):
        for _ in range(substeps):
            u = react_half(u)
            u = np.fft.irfft(np.fft.rfft(u) * diffuse, n=n_modes)
            u = react_half(u)
        U[i] = u
    return x, t, U


def exact_field(cache_dir=None, n_x=N_X, n_t=N_T, n_modes=N_SOLVE, substeps=SUBSTEPS):
    """the field on the comparison grid: x [n_x, 1] (periodic grid without the wall x = 1), t [n_t, 1], Exact_u [n_t, n_x];
    computed once and kept as allen_cahn_exact.npz under cache_dir (None: not cached)"""
    path = None if cache_dir is None else os.path.join(cache_dir, "allen_cahn_exact.npz")
    key = np.array([n_x, n_t, n_modes, substeps], dtype=np.int64)
    if path and os.path.exists(path):
        try:
            with np.load(path) as z:
                if np.array_equal(z["key"], key):
                    return z["x"], z["t"], z["Exact_u"]
        except (OSError, KeyError, ValueError):
            pass
    if n_modes % n_x:
        raise ValueError("n_modes (%d) must be a multiple of n_x (%d)" % (n_modes, n_x))
    xs, t, U = solve_allen_cahn(n_modes, n_t, substeps)
    step = n_modes // n_x
    x, Exact_u = xs[::step].reshape(-1, 1), np.ascontiguousarray(U[:, ::step])
    t = t.reshape(-1, 1)
    if path:
        try:
            os.makedirs(cache_dir, exist_ok=True)
            tmp = path + ".%d.tmp.npz" % os.getpid()
            np.savez(tmp, key=key, x=x, t=t, Exact_u=Exact_u)
            os.replace(tmp, path)
        except OSError:
            pass
    return x, t, Exact_u


def prep_data(N_0, N_b, N_f, cache_dir=None, field=None):
    """-> x, t, X, T, Exact_u, X_star, u_star, X_u_train (N_0 initial points), u_train, X_f, X_lb, X_ub (N_b wall pairs at
    common times), ub, lb.  Draws from numpy's global RNG in the order: initial points, wall times, collocation points."""
    x, t, Exact_u = field if field is not None else exact_field(cache_dir)
    X, T = np.meshgrid(x, t)
    X_star = np.column_stack((X.ravel(), T.ravel()))
    u_star = Exact_u.reshape(-1, 1)
    lb = np.array([-1.0, float(t.min())])
    ub = np.array([1.0, float(t.max())])

    pick = np.random.choice(x.shape[0], N_0, replace=False)
    X_u_train = np.column_stack((x[pick, 0], np.zeros(N_0)))
    u_train = Exact_u[0, pick].reshape(-1, 1)
    tb = lb[1] + (ub[1] - lb[1]) * np.random.rand(N_b)
    X_lb = np.column_stack((np.full(N_b, lb[0]), tb))
    X_ub = np.column_stack((np.full(N_b, ub[0]), tb))
    X_f = lb + (ub - lb) * lhs(2, N_f)
    return x, t, X, T, Exact_u, X_star, u_star, X_u_train, u_train, X_f, X_lb, X_ub, ub, lb


def plot_inf_cont_results(X_star, u_pred, X_u_train, Exact_u, x, t, save_path=None, save_hp=None, weights=None):
    """Headless figure: predicted and exact u(t, x) side by side with the initial points; persisted through saveResultDir
    like the other scripts (`weights`: the trained flat vector, written next to it as weights.npy)."""
    import matplotlib
    matplotlib.use("Agg")
    U_pred = np.asarray(u_pred).reshape(Exact_u.shape)
    fig, _ = newfig(1.0, 1.1)
    fig.clf()
    for i, (field, title) in enumerate(((U_pred, "u(t,x) predicted"), (Exact_u, "u(t,x) split-step"))):
        ax = fig.add_subplot(1, 2, i + 1)
        im = ax.imshow(field.T, interpolation="nearest", cmap="rainbow", origin="lower", aspect="auto",
                       extent=[t.min(), t.max(), x.min(), x.max()], vmin=-1.0, vmax=1.0)
        if i == 0 and X_u_train is not None:
            ax.plot(X_u_train[:, 1], X_u_train[:, 0], "kx", markersize=2, clip_on=False)
        ax.set_xlabel("t")
        ax.set_ylabel("x")
        ax.set_title(title)
    fig.colorbar(im)
    if save_path is not None and save_hp is not None:
        saveResultDir(save_path, save_hp, weights=weights)


def plot_inf_disc_results(x_star, idx_t_0, idx_t_1, x_0, u_0, u_1_pred, Exact_u, x, t, save_path=None, save_hp=None,
                          weights=None):
    """Headless figure of the discrete-time script: the split-step field with the two time slices marked, the t_0 snapshot
    with its data points, and the t_1 snapshot with the predicted last output column"""
    import matplotlib
    matplotlib.use("Agg")
    fig, _ = newfig(1.0, 1.1)
    fig.clf()
    ax = fig.add_subplot(2, 1, 1)
    im = ax.imshow(Exact_u.T, interpolation="nearest", cmap="rainbow", origin="lower", aspect="auto",
                   extent=[t.min(), t.max(), x.min(), x.max()], vmin=-1.0, vmax=1.0)
    fig.colorbar(im)
    for idx in (idx_t_0, idx_t_1):
        ax.axvline(float(t[idx, 0]), color="w", linewidth=1)
    ax.set_xlabel("t")
    ax.set_ylabel("x")
    ax.set_title("u(t,x) split-step")
    ax = fig.add_subplot(2, 2, 3)
    ax.plot(x, Exact_u[idx_t_0, :], "b-", linewidth=2, label="Exact")
    ax.plot(x_0, u_0, "rx", markersize=3, label="Data")
    ax.set_title("t = %.2f" % float(t[idx_t_0, 0]))
    ax.set_xlabel("x")
    ax = fig.add_subplot(2, 2, 4)
    ax.plot(x, Exact_u[idx_t_1, :], "b-", linewidth=2, label="Exact")
    ax.plot(x_star, u_1_pred, "r--", linewidth=2, label="Prediction")
    ax.set_title("t = %.2f" % float(t[idx_t_1, 0]))
    ax.set_xlabel("x")
    ax.legend(frameon=False, loc="best")
    if save_path is not None and save_hp is not None:
        saveResultDir(save_path, save_hp, weights=weights)
