"""Allen-Cahn discrete-time inference (one q-stage implicit Runge-Kutta step) on the MI355X engine:

    u_t - 1e-4 u_xx + 5 u^3 - 5 u = 0,   x in [-1, 1] with periodic walls,   from the snapshot at t_0 = 0.1 to t_1 = 0.9

the second discrete-time example of Raissi, Perdikaris & Karniadakis (2019).  Same CLI, hp keys and stdout log as
1d-burgers/inf_disc_burgers.py (`python 1d-allen-cahn/inf_disc_allen_cahn.py [hp.json]` from the package root).

The network maps x to the q stage values and the solution at t_1 (q + 1 outputs).  The loss is
    sum((U_0_model(x_0) - u_0)^2) + sum_j [(U_j(-1) - U_j(1))^2 + (U_x,j(-1) - U_x,j(1))^2],
    U_0_model = U + dt N(U) IRK_weights^T,   N(U) = -1e-4 U_xx - 5 U + 5 U^3
with the Gauss-Legendre table [A; b] of utils/irk.py.  It is the engine's "adr_disc" kind (csrc/kernels_disc.h): stage set 0
is the N_n points of the t_0 snapshot through dt [A; b], the periodic set is the one pair (-1, +1) at order 1, and the
coefficients are those of inf_cont_allen_cahn.py, [0, 0, 1e-4, -5, 0, 5].  Snapshots and the reference at t_1 come from
allencahnutil.exact_field (the grid rows nearest t_0 and t_1); the error is the relative L2 of the last output column
against the t_1 row.

The default arithmetic is float64, in which the engine's discrete-time kernels hold hidden layers up to 64 wide (128 in
float32, hp["dtype"] = "f32"): the paper's 200-wide layers are out of reach, the default is 4 x 64.
"""
import json
import os
import sys

import numpy as np

np.random.seed(1234)

eqnPath = "1d-allen-cahn"
_root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(os.path.join(_root, eqnPath))
sys.path.append(os.path.join(_root, "utils"))
from logger import Logger  # noqa: E402
from neuralnetwork import NeuralNetwork, set_seed  # noqa: E402
from irk import gauss_legendre_butcher  # noqa: E402
from allencahnutil import ADR_COEFFS, exact_field, plot_inf_disc_results  # noqa: E402

set_seed(1234)

if len(sys.argv) > 1:
    with open(sys.argv[1]) as hpFile:
        hp = json.load(hpFile)
else:
    hp = {
        "N_n": 200,            # data points on the t_0 snapshot
        "q": 100,              # Runge-Kutta stages
        "layers": [1, 64, 64, 64, 64, 101],     # [x] -> [u_1^n(x), ..., u_q^n(x), u^{n+1}(x)]; float64 width limit 64
        "tf_epochs": 1000, "tf_lr": 0.001, "tf_b1": 0.9, "tf_eps": 1e-08,    # Adam
        "nt_epochs": 20000, "nt_lr": 0.8, "nt_ncorr": 50,                    # L-BFGS (an iteration is ~0.1 ms: DESIGN.md 4.15)
        "log_frequency": 100,
    }

T_0, T_1 = 0.1, 0.9


class AllenCahnDiscreteNN(NeuralNetwork):
    pde = "adr_disc"

    def __init__(self, hp, logger, dt, lb, ub, IRK_weights, coeffs=ADR_COEFFS):
        super().__init__(hp, logger, ub, lb)
        self.coeffs = tuple(float(v) for v in coeffs)
        self.dt = float(dt)
        self.q = max(hp["q"], 1)
        self.IRK_weights = IRK_weights
        self._engine.set_pde_params(*self.coeffs)
        self._engine.disc_set_periodic(np.array([float(self.lb[0])]), np.array([float(self.ub[0])]), order=1)

    def _bind(self, x_0, u_0):
        """Stage set 0 = the t_0 snapshot through the IRK table (the walls are the periodic pair, set at construction)."""
        x_0 = np.asarray(x_0, dtype=np.float64).reshape(-1)
        u_0 = np.asarray(u_0, dtype=np.float64).reshape(-1)
        key = (x_0.tobytes(), u_0.tobytes())
        if key != self._bound:
            self._engine.disc_set_stage(0, x_0, u_0, self.dt * np.asarray(self.IRK_weights, dtype=np.float64))    # [q+1, q]
            self._bound = key

    def U_0_model(self, x):
        """U + dt N(U) IRK_weights^T at the points x, [len(x), q+1]."""
        if self._bound is None:
            raise RuntimeError("U_0_model needs the training set bound first (fit / grad)")
        return self._engine.disc_predict(0, np.asarray(x, dtype=np.float64).reshape(-1))

    def get_params(self, numpy=False):
        return self.coeffs

    def predict(self, x_star):
        return self.model(x_star)[:, -1]


def prep_data(N_n, q, cache_dir=None):
    """-> x [n_x,1], t [n_t,1], Exact_u, idx_t_0, idx_t_1, dt, x_0 [N_n,1], u_0 [N_n,1], x_star, u_star [n_x], IRK_weights
    [(q+1), q] = [A; b].  Draws the N_n snapshot points from numpy's global RNG."""
    x, t, Exact_u = exact_field(cache_dir)
    idx_t_0, idx_t_1 = int(np.argmin(np.abs(t[:, 0] - T_0))), int(np.argmin(np.abs(t[:, 0] - T_1)))
    dt = float(t[idx_t_1, 0] - t[idx_t_0, 0])
    pick = np.random.choice(x.shape[0], N_n, replace=False)
    x_0, u_0 = x[pick, :], Exact_u[idx_t_0, pick][:, None]
    A, b, _ = gauss_legendre_butcher(q)
    return x, t, Exact_u, idx_t_0, idx_t_1, dt, x_0, u_0, x, Exact_u[idx_t_1, :], np.vstack([A, b[None, :]])


def run(hp):
    lb, ub = np.array([-1.0]), np.array([1.0])
    (x, t, Exact_u, idx_t_0, idx_t_1, dt, x_0, u_0, x_star, u_star, IRK_weights) = prep_data(
        hp["N_n"], hp["q"], cache_dir=os.path.join(_root, eqnPath, "results"))

    logger = Logger(hp)
    pinn = AllenCahnDiscreteNN(hp, logger, dt, lb, ub, IRK_weights)

    def error():
        u_pred = pinn.predict(x_star)
        return np.linalg.norm(u_pred - u_star, 2) / np.linalg.norm(u_star, 2)

    logger.set_error_fn(error)
    pinn.fit(x_0, u_0)

    u_1_pred = pinn.predict(x_star)
    if not os.environ.get("PINN_NO_PLOT") and pinn.is_root:
        plot_inf_disc_results(x_star, idx_t_0, idx_t_1, x_0, u_0, u_1_pred, Exact_u, x, t,
                              save_path=os.path.join(_root, eqnPath), save_hp=hp, weights=pinn.get_weights())
    return pinn


if __name__ == "__main__":
    pinn = run(hp)
