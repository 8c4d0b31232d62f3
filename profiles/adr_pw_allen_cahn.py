#!/usr/bin/env python3
"""A first accuracy look at loss weights on Allen-Cahn (the sets of 1d-allen-cahn/inf_cont_allen_cahn.py: 8 x 20 float64 net,
N_0 = 512, N_b = 200, N_f = 20 000), 10^4 Adam epochs then 2000 L-BFGS iterations, in three arms:
  plain     the unweighted loss (the state profiles/adr_allen_cahn.json records as not training);
  fixed_ic  a fixed weight of 100 on the initial condition: pw_init [10, 1, 1], rates 0;
  sa        self-adaptive weights on the initial and the collocation points (arXiv:2009.04544): pw_init 1,
            pw_lr [--sa-lr-0, --sa-lr-f, 0];
over --seeds glorot initialisations.  Relative L2 error against the split-step field on the 512 x 201 grid per seed, median
and range per arm, and where the weights ended.  Reported, not gated.  Prints ONE JSON line; --out writes it too."""
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
    ap.add_argument("--adam", type=int, default=10000)
    ap.add_argument("--lbfgs", type=int, default=2000)
    ap.add_argument("--lr", type=float, default=0.001)
    ap.add_argument("--sa-lr-0", type=float, default=0.05)
    ap.add_argument("--sa-lr-f", type=float, default=0.005)
    ap.add_argument("--n-f", type=int, default=20000)
    ap.add_argument("--out")
    a = ap.parse_args()
    np.random.seed(1234)
    (x, t, X, T, Exact_u, X_star, u_star, X_u, u, X_f, X_lb, X_ub, ub, lb) = ac.prep_data(512, 200, a.n_f)
    res = {"layers": LAYERS, "n_0": 512, "n_b": 200, "n_f": a.n_f, "adam": a.adam, "lbfgs": a.lbfgs, "lr": a.lr,
           "sa_lr": [a.sa_lr_0, a.sa_lr_f, 0.0], "arms": {}}
    arms = {"plain": None, "fixed_ic": ((10.0, 1.0, 1.0), (0.0, 0.0, 0.0)), "sa": ((1.0, 1.0, 1.0), (a.sa_lr_0, a.sa_lr_f, 0.0))}
    for arm, pw in arms.items():
        errs, losses, lam_stats, bad = [], [], [], []
        for seed in range(a.seeds):
            eng = pinn_native.Engine(LAYERS, lb, ub, pde="adr", dtype="f64")
            eng.set_pde_params(*ac.ADR_COEFFS)
            eng.set_collocation(X_f)
            eng.set_data(X_u, u)
            eng.set_boundary(X_lb, X_ub)
            eng.set_weights(init.glorot_flat(LAYERS, seed=1234 + seed))
            eng.adam_init(a.lr, 0.9, 0.999, 1e-7)
            if pw:
                eng.pw_set(np.full(eng.n_u, pw[0][0]), np.full(eng.n_f, pw[0][1]), np.full(eng.n_b, pw[0][2]))
                eng.pw_adam_init(*pw[1])
            done_epochs = 0
            while done_epochs < a.adam:
                n = min(1000, a.adam - done_epochs)
                eng.adam_run(n, want_losses=False)
                done_epochs += n
            eng.lbfgs_begin(a.lbfgs, 0.8, 50, np.finfo(float).eps)
            done = 0
            while not done:
                _, _, done = eng.lbfgs_run(250)
            errs.append(float(eng.error_l2(X_star, u_star)))
            losses.append(float(eng.loss_grad(want_grad=False)[0]))
            bad.append(int(eng.status()[1]))       # number of the first evaluation with a non-finite loss (0: none)
            if pw:
                lam_stats.append([[float(l.min()), float(np.median(l)), float(l.max())] for l in eng.pw_get()])
            eng.close()
        # median / min / max over all runs (NaN as soon as one run diverged) and, beside them, over the runs that ended finite
        fin = [e for e in errs if np.isfinite(e)]
        res["arms"][arm] = {"errors": errs, "median": float(np.median(errs)), "min": float(np.min(errs)),
                            "max": float(np.max(errs)), "n_finite": len(fin),
                            "median_finite": float(np.median(fin)) if fin else None,
                            "min_finite": float(np.min(fin)) if fin else None,
                            "max_finite": float(np.max(fin)) if fin else None,
                            "final_losses": losses, "first_nonfinite_evaluation": bad,
                            "lambda_min_median_max_u_f_b": lam_stats}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
