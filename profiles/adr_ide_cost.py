#!/usr/bin/env python3
"""Cost of the trainable-coefficient residual on the float64 register-stash kernel: k_fused20d<ADR_IDE, 8> (pde "adr_ide", all
six coefficients trained) against the unchanged k_fused20d<ADR, 8> (pde "adr") on the same points, weights and coefficients,
in one process.  Cases: N_f = 10^4 (one tile per workgroup) and 10^6 (the tile loop), each without boundary pairs and with 200
periodic pairs.  Per case: warm-up, then --blocks alternating blocks of --reps loss+gradient evaluations (adr, adr_ide, adr,
adr_ide, ...); the kernel's own duration comes from the engine's launch-attached events (pinn_timing_*: exact begin-to-end of
the kernel on path 7).  Medians over the blocks and the blocks themselves.  Prints ONE JSON line; --out writes it too."""
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
COEFFS = [0.3, -0.8, 0.02, 0.6, -0.4, 1.5]


def engine(pde, n_f, n_b):
    eng = pinn_native.Engine(LAYERS, LB, UB, pde=pde, dtype="f64")
    rs = np.random.RandomState(0)
    Xu = np.column_stack([rs.uniform(-1, 1, 100), rs.uniform(0, 0.99, 100)])
    eng.set_data(Xu, -np.sin(np.pi * Xu[:, 0:1]))
    eng.set_collocation(np.column_stack([rs.uniform(-1, 1, n_f), rs.uniform(0, 0.99, n_f)]))
    if n_b:
        tb = rs.uniform(0, 0.99, n_b)
        eng.set_boundary(np.column_stack([np.full(n_b, -1.0), tb]), np.column_stack([np.full(n_b, 1.0), tb]))
    w = init.glorot_flat(LAYERS)
    if pde == "adr_ide":
        eng.set_weights(np.concatenate([w, np.zeros(6)]))
        eng.set_pde_trainable(63)
    else:
        eng.set_weights(w)
    eng.set_pde_params(*COEFFS)
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
    res = {"device": pinn_native.device_info(0)["name"], "layers": LAYERS, "blocks": a.blocks, "reps": a.reps, "coeffs": COEFFS}
    for n_f in (10000, 1000000):
        reps = a.reps if n_f <= 10000 else max(a.reps // 10, 10)
        engs = {"adr": engine("adr", n_f, 0), "adr_ide": engine("adr_ide", n_f, 0),
                "adr_pairs200": engine("adr", n_f, 200), "adr_ide_pairs200": engine("adr_ide", n_f, 200)}
        for e in engs.values():
            block(e, reps)                           # warm-up
        kern = {k: [] for k in engs}
        for _ in range(a.blocks):
            for k, e in engs.items():
                kern[k].append(block(e, reps))
        res["nf%d" % n_f] = {"reps": reps, **{"kernel_us_" + k: float(np.median(v)) for k, v in kern.items()},
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
