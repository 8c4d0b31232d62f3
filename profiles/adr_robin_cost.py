#!/usr/bin/env python3
"""Cost of the Robin point class on the float64 register-stash kernel: k_fused20d<PDE_ADR, 8> (no Robin points: the kernel
every earlier build runs) against k_fused20d<PDE_ADR_ROBIN, 8> with 400 Robin points (200 per wall) behind the same data
and collocation points, same weights, in one process.  Cases: N_f = 10^4 (one tile per workgroup) and 10^6 (the tile loop);
the equation is the one of profiles/adr_cost.py (Burgers coefficients [0, 1, nu, 0, 0, 0], 100 data points, no pairs), so
the figure without Robin points is comparable with adr_cost.json's "kernel_us_adr".  The 400 points are 6.25 more tiles of
work beside the class branch and the (alpha, beta) loads: 400 of 10 500 / 1 000 500 points.  Per case: warm-up, then
--blocks alternating blocks of --reps loss+gradient evaluations (plain, robin, plain, robin, ...); the kernel's own
duration comes from the engine's launch-attached events (pinn_timing_*: exact begin-to-end of the kernel on path 7).
Medians over the blocks, their range and the blocks themselves.  Prints ONE JSON line; --out writes it too."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pinns-tf2.0_amd"))
sys.path.insert(0, ROOT)
import pinn_native  # noqa: E402
from oracle import init  # noqa: E402

LAYERS = [2] + [20] * 8 + [1]
LB, UB = np.array([-1.0, 0.0]), np.array([1.0, 0.99])
NU = 0.01 / np.pi
N_W = 400


def engine(n_f, n_w):
    eng = pinn_native.Engine(LAYERS, LB, UB, pde="adr", dtype="f64")
    rs = np.random.RandomState(0)
    Xu = np.column_stack([rs.uniform(-1, 1, 100), rs.uniform(0, 0.99, 100)])
    eng.set_data(Xu, -np.sin(np.pi * Xu[:, 0:1]))
    eng.set_collocation(np.column_stack([rs.uniform(-1, 1, n_f), rs.uniform(0, 0.99, n_f)]))
    eng.set_pde_params(0.0, 1.0, NU, 0.0, 0.0, 0.0)
    if n_w:
        X_w = np.column_stack([np.where(np.arange(n_w) % 2, 1.0, -1.0), rs.uniform(0, 0.99, n_w)])
        eng.set_robin(X_w, rs.uniform(0.5, 1.5, n_w), rs.uniform(0.5, 1.5, n_w), rs.uniform(-1, 1, n_w))
    eng.set_weights(init.glorot_flat(LAYERS))
    assert eng.kernel_path() == 7
    return eng


def block(eng, reps):
    """kernel us per evaluation over reps event-bracketed evaluations"""
    eng.sync()
    eng.timing_enable(reps, 1)
    for _ in range(reps):
        eng.loss_grad(want_grad=False)
    eng.sync()
    t = eng.timing_read()
    assert t["kernel_exact"]
    return t["fwd_ms"] * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out")
    a = ap.parse_args()
    res = {"device": pinn_native.device_info(0)["name"], "layers": LAYERS, "blocks": a.blocks, "reps": a.reps, "n_w": N_W}
    for n_f in (10000, 1000000):
        reps = a.reps if n_f <= 10000 else max(a.reps // 10, 10)
        engs = {"adr": engine(n_f, 0), "robin400": engine(n_f, N_W)}
        for e in engs.values():
            block(e, reps)                           # warm-up
        kern = {k: [] for k in engs}
        for _ in range(a.blocks):
            for k, e in engs.items():
                kern[k].append(block(e, reps))
        med = {k: float(np.median(v)) for k, v in kern.items()}
        res["nf%d" % n_f] = {"reps": reps, **{"kernel_us_" + k: m for k, m in med.items()},
                             **{"kernel_us_range_" + k: [float(min(v)), float(max(v))] for k, v in kern.items()},
                             "extra_us_robin400": med["robin400"] - med["adr"],
                             "extra_pct_robin400": 100.0 * (med["robin400"] - med["adr"]) / med["adr"],
                             **{"kernel_us_blocks_" + k: v for k, v in kern.items()}}
        for e in engs.values():
            e.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
