"""Allen-Cahn continuous-time identification on the MI355X engine: recover nu, r1 and r3 of

    u_t - nu u_xx + r1 u + r3 u^3 = 0            (truth: nu = 1e-4, r1 = -5, r3 = 5)

from N_u samples of the field, the way 1d-burgers/ide_cont_burgers.py recovers Burgers' two parameters.  The residual is the
engine's "adr_ide" kind, f = u_t + (a0 + a1 u) u_x - nu u_xx + r1 u + r2 u^2 + r3 u^3 with the six coefficients behind the
network weights; hp["adr_trainable"] names the ones that are learned (here nu, r1, r3: a0, a1, r2 stay frozen at 0, bit for
bit) and hp["adr_init"] gives the start values, away from the truth.  nu is trained as log nu, so a coefficient of size 1e-4
moves at Adam's usual rates.  The loss is mean f^2 + mean (u - u*)^2, both at the sampled points (they are handed over as
collocation points as well).  Same CLI as the other scripts (`python 1d-allen-cahn/ide_cont_allen_cahn.py [hp.json]` from the
package root); the field comes from allencahnutil's Fourier split-step solver (solve_allen_cahn), cached under results/.
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
from neuralnetwork import ADR_NAMES, NeuralNetwork, set_seed  # noqa: E402
from allencahnutil import ADR_COEFFS, exact_field, plot_inf_cont_results  # noqa: E402

set_seed(1234)

if len(sys.argv) > 1:
    with open(sys.argv[1]) as hpFile:
        hp = json.load(hpFile)
else:
    hp = {
        "N_u": 2000,           # samples of the field
        "noise": 0.0,          # standard deviation of the added noise, in units of std(u)
        "layers": [2, 20, 20, 20, 20, 20, 20, 20, 20, 1],
        "tf_epochs": 2000, "tf_lr": 0.003, "tf_b1": 0.9, "tf_eps": None,    # Adam
        "nt_epochs": 2000, "nt_lr": 0.8, "nt_ncorr": 50,                    # L-BFGS
        "log_frequency": 100,
    }
hp.setdefault("adr_trainable", ["nu", "r1", "r3"])
hp.setdefault("adr_init", [0.0, 0.0, 1e-3, -1.0, 0.0, 1.0])      # nu, r1, r3 start away from the truth [1e-4, -5, 5]


def prep_data(N_u, noise=0.0, cache_dir=None, field=None):
    """-> x, t, Exact_u, X_star, u_star, X_u_train (N_u grid points, drawn without replacement), u_train (+ noise * std(u)
    * standard normal, as burgersutil.prep_data), ub, lb"""
    x, t, Exact_u = field if field is not None else exact_field(cache_dir)
    X, T = np.meshgrid(x, t)
    X_star = np.column_stack((X.ravel(), T.ravel()))
    u_star = Exact_u.reshape(-1, 1)
    lb, ub = np.array([-1.0, float(t.min())]), np.array([1.0, float(t.max())])
    idx = np.random.choice(X_star.shape[0], N_u, replace=False)
    X_u_train, u_train = X_star[idx, :], u_star[idx, :]
    u_train = u_train + noise * np.std(u_train) * np.random.randn(u_train.shape[0], u_train.shape[1])
    return x, t, Exact_u, X_star, u_star, X_u_train, u_train, ub, lb


class AllenCahnIdentificationNN(NeuralNetwork):
    pde = "adr_ide"

    def __init__(self, hp, logger, X_u, ub, lb):
        super().__init__(hp, logger, ub, lb)
        self._set_collocation(np.asarray(X_u, dtype=np.float64))     # the residual is taken at the data points

    def f_model(self, X=None):
        """Residual with the current coefficients at X [N, 2] (default: the sampled points), [N, 1]."""
        if X is None:
            return self._residual_collocation()
        return self._engine.residual_at(np.asarray(X, dtype=np.float64))

    def predict(self, X_star):
        return self.model(X_star), self.f_model(X_star)


def relative_errors(found, truth=ADR_COEFFS, names=("nu", "r1", "r3")):
    return {n: abs(found[ADR_NAMES.index(n)] - truth[ADR_NAMES.index(n)]) / abs(truth[ADR_NAMES.index(n)]) for n in names}


def run(hp):
    cache_dir = os.path.join(_root, eqnPath, "results")
    x, t, Exact_u, X_star, u_star, X_u_train, u_train, ub, lb = prep_data(
        hp["N_u"], noise=float(hp.get("noise", 0.0)), cache_dir=cache_dir)

    logger = Logger(hp)
    pinn = AllenCahnIdentificationNN(hp, logger, X_u_train, ub, lb)
    learned = [n for n in hp["adr_trainable"] if ADR_COEFFS[ADR_NAMES.index(n)] != 0.0]

    def error():          # mean relative error of the learned coefficients whose true value is not 0
        e = relative_errors(pinn.get_params(numpy=True), names=learned)
        return sum(e.values()) / max(len(e), 1)

    logger.set_error_fn(error)
    pinn.fit(X_u_train, u_train)

    found = pinn.get_params(numpy=True)
    if pinn.is_root:
        print("identified coefficients (truth, relative error):")
        for k, n in enumerate(ADR_NAMES):
            tag = "trained" if n in hp["adr_trainable"] else "frozen"
            rel = "%.3e" % (abs(found[k] - ADR_COEFFS[k]) / abs(ADR_COEFFS[k])) if ADR_COEFFS[k] != 0.0 else "-"
            print("  %-2s = % .8e   (% .8e, %s)  %s" % (n, found[k], ADR_COEFFS[k], rel, tag))
    u_pred = pinn.predict(X_star)[0]
    if not os.environ.get("PINN_NO_PLOT") and pinn.is_root:
        plot_inf_cont_results(X_star, u_pred.flatten(), X_u_train, Exact_u, x, t,
                              save_path=os.path.join(_root, eqnPath), save_hp=hp, weights=pinn.get_weights())
    return pinn


if __name__ == "__main__":
    pinn = run(hp)
