#!/usr/bin/env python3
"""Cost of self-adaptive point weights (include/pinn_hip.h pinn_sa_*): the Adam step of the float64 8 x 20 Burgers net with
the weights on (k_fused20d's SAW variant, ascent folded into the evaluation) against the same context with them off, at
N_f = 10^4 (one tile per workgroup) and 10^6 (the tile loop).  Per case: warm-up, then --blocks alternating blocks of --reps
Adam steps (off, on, off, on, ...) bracketed by syncs; the loss+gradient kernel's own duration comes from the engine's
launch-attached events (pinn_timing_*: exact begin-to-end of the kernel on path 7).  Medians over the blocks.  Prints ONE
JSON line; --out writes it too."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pinns-tf2.0_amd"))
sys.path.insert(0, ROOT)
import pinn_native  # noqa: E402
from oracle import init  # noqa: E402

LAYERS = [2] + [20] * 8 + [1]
LB, UB = np.array([-1.0, 0.0]), np.array([1.0, 0.99])


def engine(n_f):
    eng = pinn_native.Engine(LAYERS, LB, UB, pde="burgers", dtype="f64")
    rs = np.random.RandomState(0)
    Xu = np.column_stack([rs.uniform(-1, 1, 100), rs.uniform(0, 0.99, 100)])
    eng.set_data(Xu, -np.sin(np.pi * Xu[:, 0:1]))
    eng.set_collocation(np.column_stack([rs.uniform(-1, 1, n_f), rs.uniform(0, 0.99, n_f)]))
    eng.set_pde_params(0.01 / np.pi)
    eng.set_weights(init.glorot_flat(LAYERS))
    eng.adam_init(1e-3)
    return eng


def block(eng, reps):
    """(wall us per step without events, kernel us per evaluation from a second, event-bracketed run of the same length)"""
    eng.sync()
    t0 = time.perf_counter()
    eng.adam_run(reps, want_losses=False)
    eng.sync()
    wall = (time.perf_counter() - t0) / reps * 1e6
    eng.timing_enable(reps, 1)
    eng.adam_run(reps, want_losses=False)
    eng.sync()
    t = eng.timing_read()
    assert t["kernel_exact"]
    return wall, t["fwd_ms"] * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out")
    a = ap.parse_args()
    res = {"device": pinn_native.device_info(0)["name"], "layers": LAYERS, "blocks": a.blocks, "reps": a.reps}
    for n_f in (10000, 1000000):
        eng = engine(n_f)
        reps = a.reps if n_f <= 10000 else max(a.reps // 10, 10)
        eng.sa_adam_init(0.01)
        for on in (False, True):                     # warm-up of both variants
            if on:
                eng.sa_set_weights(np.ones(eng.n_u), np.ones(eng.n_f))
            block(eng, reps)
            eng.sa_disable()
        wall = {False: [], True: []}
        kern = {False: [], True: []}
        for _ in range(a.blocks):
            for on in (False, True):
                if on:
                    eng.sa_set_weights(np.ones(eng.n_u), np.ones(eng.n_f))
                w, k = block(eng, reps)
                wall[on].append(w)
                kern[on].append(k)
                eng.sa_disable()
        res["nf%d" % n_f] = {"reps": reps,
                             "step_us_off": float(np.median(wall[False])), "step_us_on": float(np.median(wall[True])),
                             "kernel_us_off": float(np.median(kern[False])), "kernel_us_on": float(np.median(kern[True])),
                             "kernel_us_blocks_off": kern[False], "kernel_us_blocks_on": kern[True]}
        eng.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
