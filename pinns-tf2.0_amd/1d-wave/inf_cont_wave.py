"""Second order in time on the MI355X engine: wave, telegraph (damped wave) and Klein-Gordon equations,

    u_tt - c^2 u_xx + b u_t + r1 u + r3 u^3 = s(x, t),   x in [-1, 1],   t in [0, 1],
    exact field u* = sin(pi x) cos(c pi t) + 0.5 sin(2 pi x) cos(2 c pi t)

Same CLI and shape as 1d-mms/inf_cont_mms.py (`python 1d-wave/inf_cont_wave.py [hp.json]` from the package root).  The residual
is the engine's "adr2" kind, which carries u_xx + kappa u_tt as one Taylor channel: nu = c^2, kappa = -1 / c^2
(waveutil.EQUATIONS; hp["equation"] = "wave" | "telegraph" | "klein_gordon", the last two with a manufactured source).  Zero
walls and the initial displacement u*(x, 0) are data points; the initial velocity u_t(x, 0) = 0 is a set of three-term wall
points (0, 0, 1, 0) (NeuralNetwork._set_robin3).  The error is the relative L2 distance to u* on a 256 x 101 grid.
"""
import json
import os
import sys

import numpy as np

np.random.seed(1234)

eqnPath = "1d-wave"
_root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(os.path.join(_root, eqnPath))
sys.path.append(os.path.join(_root, "utils"))
from logger import Logger  # noqa: E402
from neuralnetwork import NeuralNetwork, set_seed  # noqa: E402
from waveutil import adr2_coeffs, prep_data, source, plot_results  # noqa: E402

set_seed(1234)

if len(sys.argv) > 1:
    with open(sys.argv[1]) as hpFile:
        hp = json.load(hpFile)
else:
    hp = {
        "equation": "wave",      # wave | telegraph | klein_gordon
        "N_0": 256,              # points on the initial displacement, and as many on the initial velocity
        "N_w": 200,              # points on each wall
        "N_f": 10000,            # collocation points
        "layers": [2, 20, 20, 20, 20, 20, 20, 20, 20, 1],
        "tf_epochs": 2000, "tf_lr": 0.003, "tf_b1": 0.9, "tf_eps": None,    # Adam
        "nt_epochs": 20000, "nt_lr": 0.8, "nt_ncorr": 50,                   # L-BFGS
        "log_frequency": 2000,
    }


class WaveInformedNN(NeuralNetwork):
    pde = "adr2"

    def __init__(self, hp, logger, X_f, X_v, ub, lb, equation):
        self.coeffs = adr2_coeffs(equation)
        super().__init__(dict(hp, adr2=list(self.coeffs)), logger, ub, lb)
        self.equation = equation
        self._set_collocation(X_f)
        self._set_robin3(X_v, 0.0, 0.0, 1.0, 0.0)                # u_t(x, 0) = 0
        if equation != "wave":
            self._set_source(lambda X: source(X, equation))

    def f_model(self):
        """Residual N[u] - s at the collocation points, [N_f, 1]."""
        return self._engine.residual()

    def get_params(self, numpy=False):
        return self.coeffs

    def predict(self, X_star):
        return self.model(X_star), self.f_model()


def run(hp):
    equation = hp.get("equation", "wave")
    (x, t, Exact_u, X_star, u_star, X_u_train, u_train, X_v, X_f, ub, lb) = prep_data(hp["N_0"], hp["N_w"], hp["N_f"])
    logger = Logger(hp)
    pinn = WaveInformedNN(hp, logger, X_f, X_v, ub, lb, equation)
    logger.set_error_fn(lambda: pinn.error_l2(X_star, u_star))
    pinn.fit(X_u_train, u_train)

    u_pred, f_pred = pinn.predict(X_star)
    if pinn.is_root:
        print("Residual: max |N[u] - s| = %.4e over %d points (%s)" % (float(np.max(np.abs(f_pred))), len(f_pred), equation))
    if not os.environ.get("PINN_NO_PLOT") and pinn.is_root:
        plot_results(u_pred.flatten(), X_u_train, Exact_u, x, t, save_path=os.path.join(_root, eqnPath), save_hp=hp,
                     weights=pinn.get_weights())
    return pinn


if __name__ == "__main__":
    pinn = run(hp)
