"""Heat conduction in a rod with an insulated and a cooled end, continuous-time inference on the MI355X engine:

    u_t = nu u_xx,   x in [0, 1],   u_x(0, t) = 0,   u_x(1, t) + h u(1, t) = 0,   u(x, 0) = cos(mu x),   mu tan mu = h

Same CLI and shape as 1d-allen-cahn/inf_cont_allen_cahn.py (`python 1d-heat/inf_cont_heat.py [hp.json]` from the package
root): an hp dict or JSON file, prep_data, a Logger whose error metric is reduced on the device, a headless figure.  The
residual is the engine's "adr" kind with [0, 0, nu, 0, 0, 0]; both walls are Robin points, alpha u + beta u_x = g with
(0, 1, 0) at x = 0 and (h, 1, 0) at x = 1 (NeuralNetwork._set_robin).  The loss is mean f^2 + mean (u - u0)^2 at the
initial points + mean (alpha u + beta u_x - g)^2 over the wall points; the exact field is exp(-nu mu^2 t) cos(mu x)
(heatutil).  hp["nu"] and hp["h"] choose the problem (defaults 0.1 and 1), hp["N_0"], hp["N_w"] (per wall) and hp["N_f"]
the sets.
"""
import json
import os
import sys

import numpy as np

np.random.seed(1234)

eqnPath = "1d-heat"
_root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(os.path.join(_root, eqnPath))
sys.path.append(os.path.join(_root, "utils"))
from logger import Logger  # noqa: E402
from neuralnetwork import NeuralNetwork, set_seed  # noqa: E402
from heatutil import NU, H, adr_coeffs, prep_data, plot_inf_cont_results  # noqa: E402

set_seed(1234)

if len(sys.argv) > 1:
    with open(sys.argv[1]) as hpFile:
        hp = json.load(hpFile)
else:
    hp = {
        "nu": NU, "h": H,      # diffusivity, heat-transfer coefficient of the wall x = 1
        "N_0": 256,            # points on the initial condition
        "N_w": 200,            # points on each wall
        "N_f": 10000,          # collocation points
        "layers": [2, 20, 20, 20, 20, 20, 20, 20, 20, 1],
        "tf_epochs": 200, "tf_lr": 0.003, "tf_b1": 0.9, "tf_eps": None,     # Adam
        "nt_epochs": 500, "nt_lr": 0.8, "nt_ncorr": 50,                     # L-BFGS
        "log_frequency": 20,
    }


class HeatInformedNN(NeuralNetwork):
    pde = "adr"

    def __init__(self, hp, logger, X_f, X_w, alpha, beta, g, ub, lb, coeffs):
        super().__init__(hp, logger, ub, lb)
        self.coeffs = tuple(float(v) for v in coeffs)
        X_f = np.asarray(X_f, dtype=np.float64)
        self.x_f = self.tensor(X_f[:, 0:1])
        self.t_f = self.tensor(X_f[:, 1:2])
        self._engine.set_pde_params(*self.coeffs)
        self._set_collocation(X_f)
        self._set_robin(X_w, alpha, beta, g)

    def f_model(self):
        """Residual at the collocation points, [N_f, 1]."""
        return self._residual_collocation()

    def wall_residual(self):
        """alpha u + beta u_x - g at the wall points, [2 N_w]."""
        return self._engine.robin_residual()

    def get_params(self, numpy=False):
        return self.coeffs

    def predict(self, X_star):
        return self.model(X_star), self.f_model()


def run(hp):
    nu, h = float(hp.get("nu", NU)), float(hp.get("h", H))
    (x, t, X, T, Exact_u, X_star, u_star, X_u_train, u_train, X_f, X_w, alpha, beta, g, ub, lb) = prep_data(
        hp["N_0"], hp["N_w"], hp["N_f"], nu=nu, h=h)

    logger = Logger(hp)
    pinn = HeatInformedNN(hp, logger, X_f, X_w, alpha, beta, g, ub, lb, adr_coeffs(nu))
    logger.set_error_fn(lambda: pinn.error_l2(X_star, u_star))
    pinn.fit(X_u_train, u_train)

    u_pred = pinn.predict(X_star)[0]
    if pinn.is_root:
        print("Wall conditions: max |alpha u + beta u_x - g| = %.4e over %d points" % (
            float(np.max(np.abs(pinn.wall_residual()))), len(X_w)))
    if not os.environ.get("PINN_NO_PLOT") and pinn.is_root:
        plot_inf_cont_results(X_star, u_pred.flatten(), X_u_train, X_w, Exact_u, x, t,
                              save_path=os.path.join(_root, eqnPath), save_hp=hp, weights=pinn.get_weights())
    return pinn


if __name__ == "__main__":
    pinn = run(hp)
