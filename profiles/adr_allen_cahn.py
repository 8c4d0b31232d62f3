#!/usr/bin/env python3
"""A first accuracy look at the Allen-Cahn script's default schedule (1d-allen-cahn/inf_cont_allen_cahn.py: 8 x 20 float64
net, N_0 = 512, N_b = 200, N_f = 20 000, 100 Adam epochs at 0.03, 200 L-BFGS iterations at 0.8) in three arms:
  fixed  the collocation set of prep_data, kept;
  lhs    a new device-side Latin hypercube every --every Adam epochs;
  rad    a residual-adaptive redraw (pinn_rad_collocation, pool 10 N_f, k = 1, c = 1) every --every Adam epochs;
over --seeds glorot initialisations.  Relative L2 error against the split-step field on the 512 x 201 grid per seed, median
and range per arm.  Reported, not gated.  Prints ONE JSON line; --out writes it too."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pinns-tf2.0_amd")
sys.path.insert(0, PKG)
sys.path.insert(0, os.path.join(PKG, "1d-allen-cahn"))
sys.path.insert(0, ROOT)
import pinn_native  # noqa: E402
import allencahnutil as ac  # noqa: E402
from oracle import init  # noqa: E402

LAYERS = [2] + [20] * 8 + [1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=5)
    ap.add_argument("--adam", type=int, default=100)
    ap.add_argument("--lbfgs", type=int, default=200)
    ap.add_argument("--lr", type=float, default=0.03)
    ap.add_argument("--every", type=int, default=20)
    ap.add_argument("--n-f", type=int, default=20000)
    ap.add_argument("--out")
    a = ap.parse_args()
    np.random.seed(1234)
    (x, t, X, T, Exact_u, X_star, u_star, X_u, u, X_f, X_lb, X_ub, ub, lb) = ac.prep_data(512, 200, a.n_f)
    res = {"layers": LAYERS, "n_0": 512, "n_b": 200, "n_f": a.n_f, "adam": a.adam, "lbfgs": a.lbfgs, "lr": a.lr,
           "every": a.every, "arms": {}}
    for arm in ("fixed", "lhs", "rad"):
        errs, losses = [], []
        for seed in range(a.seeds):
            eng = pinn_native.Engine(LAYERS, lb, ub, pde="adr", dtype="f64")
            eng.set_pde_params(*ac.ADR_COEFFS)
            eng.set_collocation(X_f)
            eng.set_data(X_u, u)
            eng.set_boundary(X_lb, X_ub)
            eng.set_weights(init.glorot_flat(LAYERS, seed=1234 + seed))
            eng.adam_init(a.lr, 0.9, 0.999, 1e-7)
            done_epochs = 0
            while done_epochs < a.adam:
                if arm != "fixed" and done_epochs > 0:
                    if arm == "lhs":
                        eng.lhs_collocation(a.n_f, 1234 + done_epochs)
                    else:
                        eng.rad_collocation(a.n_f, 1234 + done_epochs, 10 * a.n_f, k=1, c=1.0)
                n = min(a.every, a.adam - done_epochs)
                eng.adam_run(n, want_losses=False)
                done_epochs += n
            eng.lbfgs_begin(a.lbfgs, 0.8, 50, np.finfo(float).eps)
            done = 0
            while not done:
                _, _, done = eng.lbfgs_run(250)
            errs.append(float(eng.error_l2(X_star, u_star)))
            losses.append(float(eng.loss_grad(want_grad=False)[0]))
            eng.close()
        res["arms"][arm] = {"errors": errs, "median": float(np.median(errs)), "min": float(np.min(errs)),
                            "max": float(np.max(errs)), "final_losses": losses}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
