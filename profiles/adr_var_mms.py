#!/usr/bin/env python3
"""A first look at the variable-media script's accuracy: 1d-mms/inf_cont_mms_var.py's default schedule (256 initial
points, 200 wall points / pairs, N_f = 10 000, 200 Adam epochs, 500 L-BFGS iterations), every medium of mmsutil.MEDIA,
both wall kinds, --seeds seeds (numpy's stream of the point sets and the initial weights), one model after the other in one
process.  Per cell: the final relative L2 error against u* on the 256 x 101 grid per seed, its median and range, and the
median of max |N_K[u] - s| over the collocation points.  Prints ONE JSON line; --out writes it too.  No threshold: a record,
not a test."""
import argparse
import contextlib
import io
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pinns-tf2.0_amd")
for p in (PKG, os.path.join(PKG, "utils"), os.path.join(PKG, "1d-mms")):
    sys.path.insert(0, p)
os.environ["PINN_NO_PLOT"] = "1"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    saved, sys.argv = sys.argv, sys.argv[:1]
    import inf_cont_mms_var as script           # its module-level hp is the default schedule
    sys.argv = saved
    import mmsutil as mu
    from logger import Logger
    import pinn_native
    cells = {}
    for eq in mu.MEDIA:
        for walls in mu.WALLS:
            runs = []
            for seed in range(a.seeds):
                hp = dict(script.hp, medium=eq, walls=walls, seed=1234 + seed, log_frequency=10 ** 9)
                np.random.seed(1234 + seed)
                (x, t, X, T, Exact_u, X_star, u_star, X_u, u, X_f, wall, ub, lb) = mu.prep_data(
                    hp["N_0"], hp["N_w"], hp["N_f"], walls=walls)
                with contextlib.redirect_stdout(io.StringIO()):
                    logger = Logger(hp)
                    pinn = script.MmsVarInformedNN(hp, logger, X_f, wall, ub, lb, eq)
                    logger.set_error_fn(lambda: pinn.error_l2(X_star, u_star))
                    pinn.fit(X_u, u)
                loss, _, terms = pinn._engine.loss_grad(want_grad=False)
                runs.append({"seed": 1234 + seed, "error_l2": float(pinn.error_l2(X_star, u_star)),
                             "res_max": float(np.max(np.abs(pinn.f_model()))), "loss": float(loss),
                             "terms": [float(v) for v in terms]})
                pinn._engine.close()
            err = [r["error_l2"] for r in runs]
            cells["%s/%s" % (eq, walls)] = {"runs": runs, "error_l2_median": float(np.median(err)),
                                            "error_l2_range": [min(err), max(err)],
                                            "res_max_median": float(np.median([r["res_max"] for r in runs]))}
            print("%s/%s: error_l2 median %.3e range [%.3e, %.3e]" % (eq, walls, np.median(err), min(err), max(err)),
                  file=sys.stderr, flush=True)
    res = {"device": pinn_native.device_info(0)["name"], "hp": {k: v for k, v in script.hp.items()}, "seeds": a.seeds,
           "cells": cells}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
