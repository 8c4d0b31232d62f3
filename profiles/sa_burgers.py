#!/usr/bin/env python3
"""A first accuracy look at self-adaptive point weights (include/pinn_hip.h pinn_sa_*) on Burgers inference: the 8 x 20
float64 net, N_u = 100, N_f = 2000 from the reference's prep_data stream, --seeds glorot initialisations, --adam Adam epochs
at rate --lr then --lbfgs L-BFGS iterations; arm "fixed" = the plain loss, arm "sa" = weights from 1 with ascent rate
--sa-lr during Adam, frozen in L-BFGS.  Relative L2 error on the reference's 25 600-point grid per seed, medians per arm.
Reported, not gated.  Prints ONE JSON line; --out writes it too."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pinns-tf2.0_amd")
sys.path.insert(0, PKG)
sys.path.insert(0, os.path.join(PKG, "1d-burgers"))
sys.path.insert(0, ROOT)
import pinn_native  # noqa: E402
import burgersutil  # noqa: E402
from oracle import init  # noqa: E402

LAYERS = [2] + [20] * 8 + [1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=5)
    ap.add_argument("--adam", type=int, default=5000)
    ap.add_argument("--lbfgs", type=int, default=1000)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--sa-lr", type=float, default=5e-3)
    ap.add_argument("--out")
    a = ap.parse_args()
    np.random.seed(1234)
    r = burgersutil.prep_data(os.path.join(PKG, "1d-burgers", "data", "burgers_shock.mat"), 100, 2000, noise=0.0)
    X_star, u_star, X_u, u, X_f, ub, lb = r[5], r[6], r[7], r[8], r[9], r[10], r[11]
    res = {"layers": LAYERS, "n_u": 100, "n_f": 2000, "adam": a.adam, "lbfgs": a.lbfgs, "lr": a.lr, "sa_lr": a.sa_lr,
           "arms": {}}
    for arm in ("fixed", "sa"):
        errs, lam = [], []
        for seed in range(a.seeds):
            w0 = init.glorot_flat(LAYERS, seed=1234 + seed)
            eng = pinn_native.Engine(LAYERS, lb, ub, pde="burgers", dtype="f64")
            eng.set_collocation(X_f)
            eng.set_data(X_u, u)
            eng.set_pde_params(0.01 / np.pi)
            eng.set_weights(w0)
            eng.adam_init(a.lr, 0.9, 0.999, 1e-7)
            if arm == "sa":
                eng.sa_set_weights(np.ones(eng.n_u), np.ones(eng.n_f))
                eng.sa_adam_init(a.sa_lr)
            eng.adam_run(a.adam, want_losses=False)
            eng.lbfgs_begin(a.lbfgs, 0.8, 50, np.finfo(float).eps)
            done = 0
            while not done:
                _, _, done = eng.lbfgs_run(250)
            errs.append(float(eng.error_l2(X_star, u_star)))
            if arm == "sa":
                lu, lf = eng.sa_get_weights()
                lam.append([float(lu.min()), float(np.median(lu)), float(lu.max()), float(lf.min()), float(np.median(lf)),
                            float(lf.max())])
            eng.close()
        res["arms"][arm] = {"errors": errs, "median": float(np.median(errs))}
        if lam:
            res["arms"][arm]["lambda_u_f_min_median_max"] = lam
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
