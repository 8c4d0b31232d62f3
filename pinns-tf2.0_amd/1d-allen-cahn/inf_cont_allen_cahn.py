"""Allen-Cahn continuous-time inference on the MI355X engine:

    u_t - 1e-4 u_xx + 5 u^3 - 5 u = 0,   x in [-1, 1] with periodic walls,   u(x, 0) = x^2 cos(pi x)

the equation residual-adaptive sampling (hp["resample"] = "rad") and its relatives are usually shown on.  Same CLI and shape
as 1d-burgers/inf_cont_burgers.py (`python 1d-allen-cahn/inf_cont_allen_cahn.py [hp.json]` from the package root): an hp
dict or JSON file, prep_data, a Logger whose error metric is reduced on the device, a headless figure.  The residual is the
engine's "adr" kind, f = u_t + (a0 + a1 u) u_x - nu u_xx + r1 u + r2 u^2 + r3 u^3 with [0, 0, 1e-4, -5, 0, 5]; the loss is
mean f^2 + mean (u - u0)^2 at the initial points + mean [(u(-1,t) - u(1,t))^2 + (u_x(-1,t) - u_x(1,t))^2] over the wall pairs.
The exact field comes from allencahnutil's Fourier split-step solver, computed at start-up and cached under results/.

Loss weights (hp["point_weights"], utils/neuralnetwork.py _pw_options; off in the default hp).  The two usual recipes for this
equation, whose plain loss tends to settle in u = 0:
    a fixed weight W on the initial condition   "point_weights": true, "pw_init": [sqrt(W), 1, 1]       (e.g. [10, 1, 1])
    self-adaptive weights (arXiv:2009.04544)    "point_weights": true, "pw_lr": [lr_0, lr_f, 0]         (e.g. [0.05, 0.01, 0])
pw_init / pw_lr are [initial points, collocation points, wall pairs]; fit() prints where the weights ended.
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
from allencahnutil import ADR_COEFFS, prep_data, plot_inf_cont_results  # noqa: E402

set_seed(1234)

if len(sys.argv) > 1:
    with open(sys.argv[1]) as hpFile:
        hp = json.load(hpFile)
else:
    hp = {
        "N_0": 512,            # points on the initial condition
        "N_b": 200,            # periodic wall pairs
        "N_f": 20000,          # collocation points
        "layers": [2, 20, 20, 20, 20, 20, 20, 20, 20, 1],
        "tf_epochs": 100, "tf_lr": 0.03, "tf_b1": 0.9, "tf_eps": None,      # Adam
        "nt_epochs": 200, "nt_lr": 0.8, "nt_ncorr": 50,                     # L-BFGS
        "log_frequency": 10,
    }


class AllenCahnInformedNN(NeuralNetwork):
    pde = "adr"

    def __init__(self, hp, logger, X_f, X_lb, X_ub, ub, lb, coeffs=ADR_COEFFS):
        super().__init__(hp, logger, ub, lb)
        self.coeffs = tuple(float(v) for v in coeffs)
        X_f = np.asarray(X_f, dtype=np.float64)
        self.x_f = self.tensor(X_f[:, 0:1])
        self.t_f = self.tensor(X_f[:, 1:2])
        self._engine.set_pde_params(*self.coeffs)
        self._set_collocation(X_f)
        self._set_boundary(np.asarray(X_lb, dtype=np.float64), np.asarray(X_ub, dtype=np.float64))

    def f_model(self):
        """Residual at the collocation points, [N_f, 1]."""
        return self._residual_collocation()

    def get_params(self, numpy=False):
        return self.coeffs

    def predict(self, X_star):
        return self.model(X_star), self.f_model()


def run(hp):
    cache_dir = os.path.join(_root, eqnPath, "results")
    (x, t, X, T, Exact_u, X_star, u_star, X_u_train, u_train, X_f, X_lb, X_ub, ub, lb) = prep_data(
        hp["N_0"], hp["N_b"], hp["N_f"], cache_dir=cache_dir)

    logger = Logger(hp)
    pinn = AllenCahnInformedNN(hp, logger, X_f, X_lb, X_ub, ub, lb)
    logger.set_error_fn(lambda: pinn.error_l2(X_star, u_star))
    pinn.fit(X_u_train, u_train)

    u_pred = pinn.predict(X_star)[0]
    if not os.environ.get("PINN_NO_PLOT") and pinn.is_root:
        plot_inf_cont_results(X_star, u_pred.flatten(), X_u_train, Exact_u, x, t,
                              save_path=os.path.join(_root, eqnPath), save_hp=hp, weights=pinn.get_weights())
    return pinn


if __name__ == "__main__":
    pinn = run(hp)
