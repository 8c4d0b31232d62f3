"""Manufactured solutions for the advection-diffusion-reaction family, continuous-time inference on the MI355X engine:

    u_t + (a0 + a1 u) u_x - nu u_xx + r1 u + r2 u^2 + r3 u^3 = s(x, t),   x in [-1, 1],   t in [0, 1]
    s = N[u*],   u*(x, t) = exp(-t) sin(pi x) + 0.3 t cos(2 pi x)

Same CLI and shape as 1d-heat/inf_cont_heat.py (`python 1d-mms/inf_cont_mms.py [hp.json]` from the package root): an hp
dict or JSON file, prep_data, a Logger whose error metric is reduced on the device, a headless figure.  The residual is the
engine's "adr" kind with a source term (NeuralNetwork._set_source, a callable: it follows hp["resample_every"] redraws);
hp["equation"] names the coefficient set (burgers, allen_cahn, fisher_kpp, advection_diffusion, heat: mmsutil.EQUATIONS),
hp["walls"] the wall kind: "dirichlet" -- Robin rows (1, 0, u*(+-1, t)) -- or "periodic" -- pairs (-1, t) <-> (1, t); u* is
2-periodic in x.  Initial data u*(x, 0); the error is the relative L2 distance to u* itself on a 256 x 101 grid.
"""
import json
import os
import sys

import numpy as np

np.random.seed(1234)

eqnPath = "1d-mms"
_root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(os.path.join(_root, eqnPath))
sys.path.append(os.path.join(_root, "utils"))
from logger import Logger  # noqa: E402
from neuralnetwork import NeuralNetwork, set_seed  # noqa: E402
from mmsutil import adr_coeffs, prep_data, source, plot_inf_cont_results  # noqa: E402

set_seed(1234)

if len(sys.argv) > 1:
    with open(sys.argv[1]) as hpFile:
        hp = json.load(hpFile)
else:
    hp = {
        "equation": "burgers",   # burgers | allen_cahn | fisher_kpp | advection_diffusion | heat
        "walls": "dirichlet",    # dirichlet | periodic
        "N_0": 256,              # points on the initial condition
        "N_w": 200,              # points on each wall (dirichlet) / wall pairs (periodic)
        "N_f": 10000,            # collocation points
        "layers": [2, 20, 20, 20, 20, 20, 20, 20, 20, 1],
        "tf_epochs": 200, "tf_lr": 0.003, "tf_b1": 0.9, "tf_eps": None,     # Adam
        "nt_epochs": 500, "nt_lr": 0.8, "nt_ncorr": 50,                     # L-BFGS
        "log_frequency": 20,
    }


class MmsInformedNN(NeuralNetwork):
    pde = "adr"

    def __init__(self, hp, logger, X_f, wall, ub, lb, coeffs):
        super().__init__(hp, logger, ub, lb)
        self.coeffs = tuple(float(v) for v in coeffs)
        X_f = np.asarray(X_f, dtype=np.float64)
        self.x_f = self.tensor(X_f[:, 0:1])
        self.t_f = self.tensor(X_f[:, 1:2])
        self._engine.set_pde_params(*self.coeffs)
        self._set_collocation(X_f)
        if wall[0] == "dirichlet":
            self._set_robin(*wall[1:])
        else:
            self._set_boundary(*wall[1:])
        self._set_source(lambda X: source(X, self.coeffs))

    def f_model(self):
        """Residual N[u] - s at the collocation points, [N_f, 1]."""
        return self._engine.residual()

    def get_params(self, numpy=False):
        return self.coeffs

    def predict(self, X_star):
        return self.model(X_star), self.f_model()


def run(hp):
    coeffs = adr_coeffs(hp.get("equation", "burgers"))
    (x, t, X, T, Exact_u, X_star, u_star, X_u_train, u_train, X_f, wall, ub, lb) = prep_data(
        hp["N_0"], hp["N_w"], hp["N_f"], walls=hp.get("walls", "dirichlet"))

    logger = Logger(hp)
    pinn = MmsInformedNN(hp, logger, X_f, wall, ub, lb, coeffs)
    logger.set_error_fn(lambda: pinn.error_l2(X_star, u_star))
    pinn.fit(X_u_train, u_train)

    u_pred, f_pred = pinn.predict(X_star)
    if pinn.is_root:
        print("Residual with the source: max |N[u] - s| = %.4e over %d points (%s, %s walls)" % (
            float(np.max(np.abs(f_pred))), len(f_pred), hp.get("equation", "burgers"), wall[0]))
    if not os.environ.get("PINN_NO_PLOT") and pinn.is_root:
        X_wall = wall[1] if wall[0] == "dirichlet" else np.vstack(wall[1:])
        plot_inf_cont_results(X_star, u_pred.flatten(), X_u_train, X_wall, Exact_u, x, t,
                              save_path=os.path.join(_root, eqnPath), save_hp=hp, weights=pinn.get_weights())
    return pinn


if __name__ == "__main__":
    pinn = run(hp)
