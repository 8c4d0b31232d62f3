#!/usr/bin/env python3
"""Final error of Burgers inference (1d-burgers/inf_cont_burgers.py's problem and hp) with three collocation schedules:
  fixed  the host set of prep_data, never redrawn (the reference's behaviour)
  lhs    a device Latin hypercube redrawn every 100 Adam epochs (hp["resample_every"] = 100)
  rad    residual-based adaptive sampling every 100 Adam epochs (hp["resample"] = "rad", k = 1, c = 1, pool 10^5)
N_f = 2000, N_u = 100, 8 x 20 float64, Adam 5000 epochs (lr 0.03, the script's, and 0.001) then L-BFGS 1000 iterations, over --seeds seeds (the
seed draws the data and collocation sets, the initial weights and the redraw seeds).  Reported: every run's relative L2
error on the 25 600-point grid, and per arm the median, min and max.  Prints ONE JSON line; --out writes it too.
    python profiles/rad_burgers.py [--seeds 5] [--adam 5000] [--lbfgs 1000] [--out profiles/rad_burgers.json]"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pinns-tf2.0_amd", "utils"))
sys.path.insert(0, os.path.join(ROOT, "pinns-tf2.0_amd", "1d-burgers"))
import neuralnetwork  # noqa: E402
from logger import Logger  # noqa: E402
from burgersutil import prep_data  # noqa: E402

MAT = os.path.join(ROOT, "pinns-tf2.0_amd", "1d-burgers", "data", "burgers_shock.mat")
ARMS = {"fixed": {}, "lhs": {"resample_every": 100},
        "rad": {"resample_every": 100, "resample": "rad", "rad_k": 1, "rad_c": 1.0, "rad_pool": 100000}}


def run(arm, seed, adam, lbfgs, lr):
    hp = {"N_u": 100, "N_f": 2000, "layers": [2] + [20] * 8 + [1], "tf_epochs": adam, "tf_lr": lr, "tf_b1": 0.9,
          "tf_eps": None, "nt_epochs": lbfgs, "nt_lr": 0.8, "nt_ncorr": 50, "log_frequency": 1000, "dtype": "f64",
          "seed": seed, "resample_seed": 1000 * seed}
    hp.update(ARMS[arm])
    np.random.seed(seed)
    (x, t, X, T, Exact_u, X_star, u_star, X_u, u, X_f, ub, lb) = prep_data(MAT, hp["N_u"], hp["N_f"], noise=0.0)
    with contextlib.redirect_stdout(io.StringIO()):
        logger = Logger(hp)
        nn = neuralnetwork.NeuralNetwork(hp, logger, ub, lb)
        nn._set_collocation(X_f)
        nn._engine.set_pde_params(0.01 / np.pi)
        logger.set_error_fn(lambda: nn.error_l2(X_star, u_star))
        t0 = time.perf_counter()
        nn.fit(X_u, u)
        secs = time.perf_counter() - t0
    return float(nn.error_l2(X_star, u_star)), secs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=5)
    ap.add_argument("--adam", type=int, default=5000)
    ap.add_argument("--lbfgs", type=int, default=1000)
    ap.add_argument("--tf-lr", default="0.03,0.001", help="Adam learning rates, one schedule each (0.03: the script's)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"problem": "burgers inference, N_f 2000, N_u 100, 8x20 f64", "adam_epochs": a.adam, "lbfgs_iters": a.lbfgs,
           "redraw_every": 100, "rad": {"k": 1, "c": 1.0, "pool": 100000}, "schedules": {}}
    for lr in [float(v) for v in a.tf_lr.split(",")]:
        arms = res["schedules"]["tf_lr=%g" % lr] = {}
        for arm in ARMS:                           # runs are deterministic: the order of the arms does not matter
            errs, secs = [], []
            for s in range(1, a.seeds + 1):
                e, t = run(arm, s, a.adam, a.lbfgs, lr)
                errs.append(e)
                secs.append(t)
            arms[arm] = {"error_l2": errs, "median": float(np.median(errs)), "min": float(np.min(errs)),
                         "max": float(np.max(errs)), "fit_seconds": secs}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
