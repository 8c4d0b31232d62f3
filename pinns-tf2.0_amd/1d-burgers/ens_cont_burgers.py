"""Burgers continuous-time ensemble: hp["members"] seeds of the inf_cont_burgers hp (or, with hp["identify"], of the
ide_cont_burgers hp) trained side by side on one point set by one engine ensemble (utils/ensemble.py), then one line per
member and the spread: the final error, or lambda_1 and lambda_2.
    python 1d-burgers/ens_cont_burgers.py [hp.json]          (run from the package root)
Member k uses hp["seed"] + k (default 1234 + k) for its initial weights and ends bit-identical to that seed trained alone.
"""
import json
import os
import sys

import numpy as np

np.random.seed(1234)

eqnPath = "1d-burgers"
_root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(os.path.join(_root, eqnPath))
sys.path.append(os.path.join(_root, "utils"))
from logger import Logger  # noqa: E402
from ensemble import NeuralNetworkEnsemble  # noqa: E402
from burgersutil import prep_data  # noqa: E402

if len(sys.argv) > 1:
    with open(sys.argv[1]) as hpFile:
        hp = json.load(hpFile)
else:
    hp = {"members": 8, "identify": False}
identify = bool(hp.get("identify", False))
defaults = ({"N_u": 2000, "layers": [2, 20, 20, 20, 20, 20, 20, 20, 20, 1],          # ide_cont_burgers.py
             "tf_epochs": 100, "tf_lr": 0.001, "tf_b1": 0.9, "tf_eps": None,
             "nt_epochs": 500, "nt_lr": 0.8, "nt_ncorr": 50, "log_frequency": 10} if identify else
            {"N_u": 100, "N_f": 10000, "layers": [2, 20, 20, 20, 20, 20, 20, 20, 20, 1],   # inf_cont_burgers.py
             "tf_epochs": 100, "tf_lr": 0.03, "tf_b1": 0.9, "tf_eps": None,
             "nt_epochs": 200, "nt_lr": 0.8, "nt_ncorr": 50, "log_frequency": 10})
hp = dict(defaults, **hp)


def spread(name, v):
    v = np.asarray(v, dtype=np.float64)
    print("%s: min %.6e  median %.6e  max %.6e  mean %.6e  std %.3e" % (name, v.min(), np.median(v), v.max(), v.mean(),
                                                                        v.std(ddof=1) if v.size > 1 else 0.0))


def run(hp):
    path = os.path.join(_root, eqnPath, "data", "burgers_shock.mat")
    seed0 = int(hp.get("seed", 1234))
    members = [{"seed": seed0 + k} for k in range(int(hp["members"]))]
    hp_model = {k: v for k, v in hp.items() if k not in ("members", "identify", "seed")}
    logger = Logger(hp)
    if identify:
        x, t, X, T, Exact_u, X_star, u_star, X_u_train, u_train, ub, lb = prep_data(path, hp["N_u"], noise=0.0)
        ens = NeuralNetworkEnsemble(hp_model, logger, ub, lb, members, pde="burgers_ide")
    else:
        (x, t, X, T, Exact_u, X_star, u_star,
         X_u_train, u_train, X_f, ub, lb) = prep_data(path, hp["N_u"], hp["N_f"], noise=0.0)
        ens = NeuralNetworkEnsemble(hp_model, logger, ub, lb, members, pde="burgers")
        ens.set_collocation(X_f)
        ens.set_pde_params(0.01 / np.pi)
    ens.fit(X_u_train, u_train)
    if identify:
        l1, l2 = ens.get_params(numpy=True)
        for k, m in enumerate(members):
            print("member %2d  seed %d  l1 = %.6f  l2 = %.6e  L-BFGS done %d" % (k, m["seed"], l1[k], l2[k], ens.nt_done[k]))
        spread("l1", l1)
        spread("l2", l2)
    else:
        err = ens.error_l2(X_star, u_star)
        for k, m in enumerate(members):
            print("member %2d  seed %d  error = %.6e  L-BFGS done %d" % (k, m["seed"], err[k], ens.nt_done[k]))
        spread("error", err)
    return ens


if __name__ == "__main__":
    run(hp)
