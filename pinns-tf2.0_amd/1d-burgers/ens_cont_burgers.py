"""Burgers continuous-time ensemble: hp["members"] seeds of the inf_cont_burgers hp (or, with hp["identify"], of the
ide_cont_burgers hp) trained side by side on one point set by one engine ensemble (utils/ensemble.py), then one line per
member and the spread: the final error, or lambda_1 and lambda_2.
    python 1d-burgers/ens_cont_burgers.py [hp.json]          (run from the package root)
Member k uses hp["seed"] + k (default 1234 + k) for its initial weights and ends bit-identical to that seed trained alone.
Two more ways to use the members (inference unless noted):
    hp["nu_sweep"] = [nu_0, ..., nu_K-1]   one member per viscosity (hp["members"] is ignored); prints each member's
                                           final loss and nu, and the error of the member at nu = 0.01/pi
    hp["bagged"] = true                    member k draws its own N_u data subsample and N_f collocation set (inference;
                                           identification: its N_u data points) with np.random.seed(hp["seed"] + k);
                                           prints the error (or lambda) spread
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


def final_losses(ens):
    """each member's last logged loss: L-BFGS, or Adam when L-BFGS logged nothing"""
    return np.array([ens.nt_log[k][1][-1] if len(ens.nt_log[k][1]) else ens.adam_losses[-1, k]
                     for k in range(ens.n_members)])


def bags(path, hp, seed0, K):
    """member k's data (and collocation) drawn as prep_data draws them, after np.random.seed(seed0 + k)"""
    picked = []
    for k in range(K):
        np.random.seed(seed0 + k)
        r = prep_data(path, hp["N_u"], noise=0.0) if identify else prep_data(path, hp["N_u"], hp["N_f"], noise=0.0)
        picked.append(r[7:9] if identify else r[7:10])        # (X_u, u) or (X_u, u, X_f)
    return [np.stack(column) for column in zip(*picked)]


def run(hp):
    path = os.path.join(_root, eqnPath, "data", "burgers_shock.mat")
    seed0 = int(hp.get("seed", 1234))
    nu_sweep = hp.get("nu_sweep")
    bagged = bool(hp.get("bagged", False))
    if nu_sweep is not None and identify:
        raise ValueError("nu_sweep is an inference option (identification learns nu)")
    K = len(nu_sweep) if nu_sweep is not None else int(hp["members"])
    members = [{"seed": seed0 + k} for k in range(K)]
    if nu_sweep is not None:
        for k, nu in enumerate(nu_sweep):
            members[k]["nu"] = float(nu)
    hp_model = {k: v for k, v in hp.items() if k not in ("members", "identify", "seed", "nu_sweep", "bagged")}
    logger = Logger(hp)
    if identify:
        x, t, X, T, Exact_u, X_star, u_star, X_u_train, u_train, ub, lb = prep_data(path, hp["N_u"], noise=0.0)
        if bagged:
            X_u_train, u_train = bags(path, hp, seed0, K)
        ens = NeuralNetworkEnsemble(hp_model, logger, ub, lb, members, pde="burgers_ide")
    else:
        (x, t, X, T, Exact_u, X_star, u_star,
         X_u_train, u_train, X_f, ub, lb) = prep_data(path, hp["N_u"], hp["N_f"], noise=0.0)
        if bagged:
            X_u_train, u_train, X_f = bags(path, hp, seed0, K)
        ens = NeuralNetworkEnsemble(hp_model, logger, ub, lb, members, pde="burgers")
        ens.set_collocation(X_f)
        ens.set_pde_params(0.01 / np.pi)
    ens.fit(X_u_train, u_train)
    if nu_sweep is not None:
        loss = final_losses(ens)
        err = ens.error_l2(X_star, u_star)
        for k, m in enumerate(members):
            print("member %2d  nu = %.6e  final loss = %.6e  L-BFGS done %d" % (k, m["nu"], loss[k], ens.nt_done[k]))
        for k, m in enumerate(members):
            if m["nu"] == 0.01 / np.pi:
                print("member %2d  nu = 0.01/pi  error = %.6e" % (k, err[k]))
        return ens
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
