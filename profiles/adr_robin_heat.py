#!/usr/bin/env python3
"""A first look at the heat script's accuracy: 1d-heat/inf_cont_heat.py's default hp (nu = 0.1, h = 1, 256 initial points,
200 points per wall, N_f = 10 000, 200 Adam epochs, 500 L-BFGS iterations), --seeds seeds (numpy's stream of the point sets
and the initial weights), one model after the other in one process.  Per seed: the final relative L2 error on the 256 x 101
grid and max |alpha u + beta u_x - g| over the 400 wall points; medians and ranges.  Prints ONE JSON line; --out writes it
too.  No threshold: a record, not a test."""
import argparse
import contextlib
import io
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pinns-tf2.0_amd")
for p in (PKG, os.path.join(PKG, "utils"), os.path.join(PKG, "1d-heat")):
    sys.path.insert(0, p)
os.environ["PINN_NO_PLOT"] = "1"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    saved, sys.argv = sys.argv, sys.argv[:1]
    import inf_cont_heat as script          # its module-level hp is the default schedule
    sys.argv = saved
    import heatutil as hu
    from logger import Logger
    import pinn_native
    runs = []
    for seed in range(a.seeds):
        hp = dict(script.hp, seed=1234 + seed, log_frequency=10 ** 9)
        np.random.seed(1234 + seed)
        (x, t, X, T, Exact_u, X_star, u_star, X_u, u, X_f, X_w, alpha, beta, g, ub, lb) = hu.prep_data(
            hp["N_0"], hp["N_w"], hp["N_f"], nu=hp["nu"], h=hp["h"])
        with contextlib.redirect_stdout(io.StringIO()):
            logger = Logger(hp)
            pinn = script.HeatInformedNN(hp, logger, X_f, X_w, alpha, beta, g, ub, lb, hu.adr_coeffs(hp["nu"]))
            logger.set_error_fn(lambda: pinn.error_l2(X_star, u_star))
            pinn.fit(X_u, u)
        loss, _, terms = pinn._engine.loss_grad(want_grad=False)
        runs.append({"seed": 1234 + seed, "error_l2": float(pinn.error_l2(X_star, u_star)),
                     "wall_max": float(np.max(np.abs(pinn.wall_residual()))), "loss": float(loss),
                     "terms": [float(v) for v in terms]})
        pinn._engine.close()
    err, wall = [r["error_l2"] for r in runs], [r["wall_max"] for r in runs]
    res = {"device": pinn_native.device_info(0)["name"], "hp": {k: v for k, v in script.hp.items()}, "runs": runs,
           "error_l2_median": float(np.median(err)), "error_l2_range": [min(err), max(err)],
           "wall_max_median": float(np.median(wall)), "wall_max_range": [min(wall), max(wall)]}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
