"""A steady problem in two space dimensions on the MI355X engine: Helmholtz,

    -Laplace u - k^2 u = s(x, y)   on [-1, 1]^2,   u = 0 on the walls,   exact field u* = sin(pi x) sin(4 pi y)

Same CLI and shape as 1d-mms/inf_cont_mms.py (`python 2d-helmholtz/inf_helmholtz.py [hp.json]` from the package root).  The
net's second input is y; the residual is the engine's "adr2" kind with b = 0, nu = 1, kappa = 1, r1 = -k^2, which carries
u_xx + u_yy as one Taylor channel (helmholtzutil.adr2_coeffs), and the source s = (17 pi^2 - k^2) u*.  The walls are data
points.  hp["k"] is the wave number (k = 0: Poisson).  The error is the relative L2 distance to u* on a 201 x 201 grid.
"""
import json
import os
import sys

import numpy as np

np.random.seed(1234)

eqnPath = "2d-helmholtz"
_root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(os.path.join(_root, eqnPath))
sys.path.append(os.path.join(_root, "utils"))
from logger import Logger  # noqa: E402
from neuralnetwork import NeuralNetwork, set_seed  # noqa: E402
from helmholtzutil import adr2_coeffs, prep_data, source, plot_results  # noqa: E402

set_seed(1234)

if len(sys.argv) > 1:
    with open(sys.argv[1]) as hpFile:
        hp = json.load(hpFile)
else:
    hp = {
        "k": 4.0,                # wave number
        "N_w": 200,              # points on each of the four walls
        "N_f": 10000,            # collocation points
        "layers": [2, 20, 20, 20, 20, 20, 20, 20, 20, 1],
        "tf_epochs": 2000, "tf_lr": 0.003, "tf_b1": 0.9, "tf_eps": None,    # Adam
        "nt_epochs": 20000, "nt_lr": 0.8, "nt_ncorr": 50,                   # L-BFGS
        "log_frequency": 2000,
    }


class HelmholtzInformedNN(NeuralNetwork):
    pde = "adr2"

    def __init__(self, hp, logger, X_f, ub, lb, k):
        self.coeffs = adr2_coeffs(k)
        super().__init__(dict(hp, adr2=list(self.coeffs)), logger, ub, lb)
        self._set_collocation(X_f)
        self._set_source(lambda X: source(X, k))

    def f_model(self):
        """Residual N[u] - s at the collocation points, [N_f, 1]."""
        return self._engine.residual()

    def get_params(self, numpy=False):
        return self.coeffs

    def predict(self, X_star):
        return self.model(X_star), self.f_model()


def run(hp):
    k = float(hp.get("k", 4.0))
    (x, y, Exact_u, X_star, u_star, X_u_train, u_train, X_f, ub, lb) = prep_data(hp["N_w"], hp["N_f"])
    logger = Logger(hp)
    pinn = HelmholtzInformedNN(hp, logger, X_f, ub, lb, k)
    logger.set_error_fn(lambda: pinn.error_l2(X_star, u_star))
    pinn.fit(X_u_train, u_train)

    u_pred, f_pred = pinn.predict(X_star)
    if pinn.is_root:
        print("Residual with the source: max |N[u] - s| = %.4e over %d points (k = %g)" % (
            float(np.max(np.abs(f_pred))), len(f_pred), k))
    if not os.environ.get("PINN_NO_PLOT") and pinn.is_root:
        plot_results(u_pred.flatten(), X_u_train, Exact_u, x, y, save_path=os.path.join(_root, eqnPath), save_hp=hp,
                     weights=pinn.get_weights())
    return pinn


if __name__ == "__main__":
    pinn = run(hp)
