"""Manufactured solutions in a variable medium, continuous-time inference on the MI355X engine:

    u_t + (a0 + a1 u) u_x - nu u_xx + r1 u + r2 u^2 + r3 u^3 = s(x, t),   x in [-1, 1],   t in [0, 1]
    with the six coefficients FIELDS over the domain,   s = N_K[u*],   u*(x, t) = exp(-t) sin(pi x) + 0.3 t cos(2 pi x)

Same CLI and shape as 1d-mms/inf_cont_mms.py (`python 1d-mms/inf_cont_mms_var.py [hp.json]` from the package root).  The
residual is the engine's "adr" kind with per-point coefficient fields and a source term (NeuralNetwork._set_coef_fields and
_set_source, both callables: they follow hp["resample_every"] redraws).  hp["medium"] names the fields (mmsutil.MEDIA):
"graded_rod" -- nu(x) = 0.1 (1 + 0.8 tanh 8x) in conservative form, -(nu u_x)_x, so a0 = -nu'(x); "shear_flow" --
a0(x, t) = 0.7 + 0.3 sin(pi x) cos(pi t), nu = 0.05; "graded_reaction" -- Allen-Cahn with r1 = -5 (1 + 0.5 x), r3 = 5.
hp["walls"] as in inf_cont_mms.py: "dirichlet" or "periodic" (u* and every field but the rod's are 2-periodic in x; the
pairs state u and u_x, which u* satisfies in any medium).  The error is the relative L2 distance to u* itself.
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
from mmsutil import medium_fields, prep_data, source_var, plot_inf_cont_results  # noqa: E402

set_seed(1234)

if len(sys.argv) > 1:
    with open(sys.argv[1]) as hpFile:
        hp = json.load(hpFile)
else:
    hp = {
        "medium": "graded_rod",  # graded_rod | shear_flow | graded_reaction
        "walls": "dirichlet",    # dirichlet | periodic
        "N_0": 256,              # points on the initial condition
        "N_w": 200,              # points on each wall (dirichlet) / wall pairs (periodic)
        "N_f": 10000,            # collocation points
        "layers": [2, 20, 20, 20, 20, 20, 20, 20, 20, 1],
        "tf_epochs": 200, "tf_lr": 0.003, "tf_b1": 0.9, "tf_eps": None,     # Adam
        "nt_epochs": 500, "nt_lr": 0.8, "nt_ncorr": 50,                     # L-BFGS
        "log_frequency": 20,
    }


class MmsVarInformedNN(NeuralNetwork):
    pde = "adr"

    def __init__(self, hp, logger, X_f, wall, ub, lb, medium):
        super().__init__(hp, logger, ub, lb)
        self.medium = medium
        X_f = np.asarray(X_f, dtype=np.float64)
        self.x_f = self.tensor(X_f[:, 0:1])
        self.t_f = self.tensor(X_f[:, 1:2])
        self._engine.set_pde_params(0.0, 0.0, 0.0, 0.0, 0.0, 0.0)      # not read while the fields are present
        self._set_collocation(X_f)
        if wall[0] == "dirichlet":
            self._set_robin(*wall[1:])
        else:
            self._set_boundary(*wall[1:])
        self._set_coef_fields(lambda X: medium_fields(X, self.medium))
        self._set_source(lambda X: source_var(X, medium_fields(X, self.medium)))

    def f_model(self):
        """Residual N_K[u] - s at the collocation points, [N_f, 1]."""
        return self._engine.residual()

    def get_params(self, numpy=False):
        return self.medium

    def predict(self, X_star):
        return self.model(X_star), self.f_model()


def run(hp):
    medium = hp.get("medium", "graded_rod")
    medium_fields(np.zeros((1, 2)), medium)          # an unknown name is refused before anything is built
    (x, t, X, T, Exact_u, X_star, u_star, X_u_train, u_train, X_f, wall, ub, lb) = prep_data(
        hp["N_0"], hp["N_w"], hp["N_f"], walls=hp.get("walls", "dirichlet"))

    logger = Logger(hp)
    pinn = MmsVarInformedNN(hp, logger, X_f, wall, ub, lb, medium)
    logger.set_error_fn(lambda: pinn.error_l2(X_star, u_star))
    pinn.fit(X_u_train, u_train)

    u_pred, f_pred = pinn.predict(X_star)
    if pinn.is_root:
        print("Residual with the fields and the source: max |N_K[u] - s| = %.4e over %d points (%s, %s walls)" % (
            float(np.max(np.abs(f_pred))), len(f_pred), medium, wall[0]))
    if not os.environ.get("PINN_NO_PLOT") and pinn.is_root:
        X_wall = wall[1] if wall[0] == "dirichlet" else np.vstack(wall[1:])
        plot_inf_cont_results(X_star, u_pred.flatten(), X_u_train, X_wall, Exact_u, x, t,
                              save_path=os.path.join(_root, eqnPath), save_hp=hp, weights=pinn.get_weights())
    return pinn


if __name__ == "__main__":
    pinn = run(hp)
