#!/usr/bin/env python3
"""Cost of per-point coefficient fields on the float64 register-stash kernel: k_fused20d<PDE_ADR, 8> (no fields: the kernel
every earlier build runs, the yardstick) against k_fused20d<PDE_ADR_VAR, 8> with a row of six coefficients at every collocation
point (every row the constant set: the same arithmetic on the same values), same data and collocation points, same weights, in
one process.  Cases: N_f = 10^4 (one tile per workgroup) and 10^6 (the tile loop); the equation is the one of
profiles/adr_cost.py, adr_robin_cost.py and adr_src_cost.py (Burgers coefficients [0, 1, nu, 0, 0, 0], 100 data points, no
pairs, no Robin points, no source), so the figure without fields is comparable with theirs.  The fields cost three 16-byte
loads (48 bytes) and the source's 8-byte load and subtraction per collocation point in the seed block.  Per case: warm-up,
then --blocks alternating blocks of --reps loss+gradient evaluations (plain, fields, plain, fields, ...); the kernel's own
duration comes from the engine's
launch-attached events (pinn_timing_*: exact begin-to-end of the kernel on path 7).  Medians over the blocks, their range
(the block-to-block spread the difference is read against) and the blocks themselves.  Prints ONE JSON line; --out writes
it too."""
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


def engine(n_f, with_fields):
    eng = pinn_native.Engine(LAYERS, LB, UB, pde="adr", dtype="f64")
    rs = np.random.RandomState(0)
    Xu = np.column_stack([rs.uniform(-1, 1, 100), rs.uniform(0, 0.99, 100)])
    eng.set_data(Xu, -np.sin(np.pi * Xu[:, 0:1]))
    X_f = np.column_stack([rs.uniform(-1, 1, n_f), rs.uniform(0, 0.99, n_f)])
    eng.set_collocation(X_f)
    eng.set_pde_params(0.0, 1.0, NU, 0.0, 0.0, 0.0)
    if with_fields:
        eng.set_coef_fields(np.tile([0.0, 1.0, NU, 0.0, 0.0, 0.0], (n_f, 1)))
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
    res = {"device": pinn_native.device_info(0)["name"], "layers": LAYERS, "blocks": a.blocks, "reps": a.reps}
    for n_f in (10000, 1000000):
        reps = a.reps if n_f <= 10000 else max(a.reps // 10, 10)
        engs = {"adr": engine(n_f, False), "var": engine(n_f, True)}
        for e in engs.values():
            block(e, reps)                           # warm-up
        kern = {k: [] for k in engs}
        for _ in range(a.blocks):
            for k, e in engs.items():
                kern[k].append(block(e, reps))
        med = {k: float(np.median(v)) for k, v in kern.items()}
        res["nf%d" % n_f] = {"reps": reps, **{"kernel_us_" + k: m for k, m in med.items()},
                             **{"kernel_us_range_" + k: [float(min(v)), float(max(v))] for k, v in kern.items()},
                             "extra_us_var": med["var"] - med["adr"],
                             "extra_pct_var": 100.0 * (med["var"] - med["adr"]) / med["adr"],
                             "spread_us_adr": float(max(kern["adr"]) - min(kern["adr"])),
                             "spread_us_var": float(max(kern["var"]) - min(kern["var"])),
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
