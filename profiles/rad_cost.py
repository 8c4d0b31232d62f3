#!/usr/bin/env python3
"""Device time of one residual-based adaptive redraw (Engine.rad_collocation, include/pinn_hip.h pinn_rad_collocation) on
the float64 / float32 8 x 20 Burgers net, against the Adam step of the same context:
  nf1e4_m1e5_f64   N_f = 10^4, pool M = 10^5, float64
  nf1e4_m1e5_f32   the same in float32
  shard125k_m1e6   a 125 000-point shard of a 10^6-point design, M = 10^6, float64
Each case: warm-up, then blocks of --reps redraws (same count: in place, enqueue only) bracketed by syncs, median over
--blocks blocks; the Adam step likewise.  The per-kernel split comes from a separate run under
`rocprofv3 --kernel-trace --stats -d D -o rad -- python profiles/rad_cost.py --redraws-only`, summarised by
profiles/summarize_rocpd.py into profiles/rad_cost_kernel_stats.txt.  Prints ONE JSON line; --out writes it too."""
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
CASES = [("nf1e4_m1e5_f64", "f64", 10000, 10000, 100000), ("nf1e4_m1e5_f32", "f32", 10000, 10000, 100000),
         ("shard125k_m1e6", "f64", 1000000, 125000, 1000000)]


def engine(dtype, n_design, count):
    eng = pinn_native.Engine(LAYERS, LB, UB, pde="burgers", dtype=dtype)
    rs = np.random.RandomState(0)
    Xu = np.column_stack([rs.uniform(-1, 1, 100), np.zeros(100)])
    eng.set_data(Xu, -np.sin(np.pi * Xu[:, 0:1]), n_total=100)
    eng.set_pde_params(0.01 / np.pi)
    eng.lhs_collocation(n_design, 1, first=0, count=count)
    eng.set_weights(init.glorot_flat(LAYERS))
    eng.adam_init(1e-3)
    eng.adam_run(20)
    return eng


def timed(fn, reps, blocks, eng):
    out = []
    for _ in range(blocks):
        eng.sync()
        t0 = time.perf_counter()
        for i in range(reps):
            fn(i)
        eng.sync()
        out.append((time.perf_counter() - t0) / reps * 1e6)
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--redraws-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"net": "2-20x8-1 burgers", "cases": {}}
    for name, dtype, n_design, count, M in CASES:
        eng = engine(dtype, n_design, count)
        redraw = lambda i: eng.rad_collocation(n_design, 100 + i, M, k=1, c=1.0, first=0, count=count)  # noqa: E731
        redraw(0)
        if a.redraws_only:
            for i in range(a.reps):
                redraw(i)
            eng.sync()
            continue
        us_rad = timed(redraw, a.reps, a.blocks, eng)
        us_adam = timed(lambda i: eng.adam_run(10, want_losses=False), a.reps, a.blocks, eng) / 10.0
        res["cases"][name] = {"dtype": dtype, "n_design": n_design, "count": count, "pool": M,
                              "redraw_us": us_rad, "adam_step_us": us_adam, "adam_steps_per_redraw": us_rad / us_adam}
        eng.close()
    if a.redraws_only:
        return
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
