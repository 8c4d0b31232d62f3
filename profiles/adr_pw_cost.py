#!/usr/bin/env python3
"""Cost of the per-point loss weights of the adr kind on the float64 register-stash kernel: k_fused20d<ADR, 8, ., SAW>
against the unchanged k_fused20d<ADR, 8> on the same points and weights, in one process (built like profiles/adr_cost.py).
Cases: N_f = 10^4 (one tile per workgroup) and 10^6 (the tile loop), without boundary pairs and with 200 periodic pairs.
Arms, all timed inside Adam steps (theta rate 1e-12, so the weights stay where they are):
  adr        the plain kernel, the yardstick;
  pw_fixed   weights on, all rates 0: lambda is read, nothing is written back;
  pw_sa      all three rates on (1e-9): lambda, m and v of every point and pair are read and written back every step.
Per case: warm-up, then --blocks alternating blocks of --reps steps (adr, pw_fixed, pw_sa, adr, ...); the kernel's own
duration comes from the engine's launch-attached events (pinn_timing_*: exact begin-to-end of the kernel on path 7).
Medians over the blocks, their range, and the blocks themselves.  Prints ONE JSON line; --out writes it too."""
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
LB, UB = np.array([-1.0, 0.0]), np.array([1.0, 1.0])
ALLEN_CAHN = (0.0, 0.0, 1e-4, -5.0, 0.0, 5.0)


def engine(arm, n_f, n_b):
    eng = pinn_native.Engine(LAYERS, LB, UB, pde="adr", dtype="f64")
    rs = np.random.RandomState(0)
    x0 = rs.uniform(-1, 1, 100)
    eng.set_data(np.column_stack([x0, np.zeros(100)]), (x0 * x0 * np.cos(np.pi * x0)).reshape(-1, 1))
    eng.set_collocation(LB + (UB - LB) * rs.uniform(size=(n_f, 2)))
    eng.set_pde_params(*ALLEN_CAHN)
    if n_b:
        tb = rs.uniform(0, 1, n_b)
        eng.set_boundary(np.column_stack([np.full(n_b, -1.0), tb]), np.column_stack([np.full(n_b, 1.0), tb]))
    eng.set_weights(init.glorot_flat(LAYERS))
    assert eng.kernel_path() == 7
    eng.adam_init(1e-12, 0.9, 0.999, 1e-7)
    if arm != "adr":
        eng.pw_set(rs.uniform(0.5, 2.0, 100), rs.uniform(0.5, 2.0, n_f), rs.uniform(0.5, 2.0, n_b))
        r = 1e-9 if arm == "pw_sa" else 0.0
        eng.pw_adam_init(r, r, r)
    return eng


def block(eng, reps):
    """kernel us per evaluation over reps event-bracketed Adam steps"""
    eng.sync()
    eng.timing_enable(reps, 1)
    eng.adam_run(reps, want_losses=False)
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
        for n_b in (0, 200):
            engs = {arm: engine(arm, n_f, n_b) for arm in ("adr", "pw_fixed", "pw_sa")}
            for e in engs.values():
                block(e, reps)                           # warm-up
            kern = {k: [] for k in engs}
            for _ in range(a.blocks):
                for k, e in engs.items():
                    kern[k].append(block(e, reps))
            med = {k: float(np.median(v)) for k, v in kern.items()}
            res["nf%d_nb%d" % (n_f, n_b)] = {
                "reps": reps, **{"kernel_us_" + k: m for k, m in med.items()},
                **{"kernel_us_range_" + k: [float(np.min(v)), float(np.max(v))] for k, v in kern.items()},
                **{"extra_us_" + k: med[k] - med["adr"] for k in ("pw_fixed", "pw_sa")},
                **{"extra_pct_" + k: 100.0 * (med[k] / med["adr"] - 1.0) for k in ("pw_fixed", "pw_sa")},
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
