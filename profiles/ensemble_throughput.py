#!/usr/bin/env python3
"""Member throughput of an ensemble (pinn_native.Ensemble) against a solo Engine in the same process, float64 Burgers
inference at the default size (N_f = 10^4, N_u = 100, 8 x 20, kernel path 7).

For each K: Adam member-steps/s = K x steps / s and L-BFGS member-iterations/s, each the median over `--blocks` timed
blocks of >= `--seconds` s (the block length is calibrated first; every block ends with the host reading the losses, as
adam_run / lbfgs_run do).  Prints ONE JSON line.
    python profiles/ensemble_throughput.py [--ks 1,2,4,8,16,32] [--seconds 1.0] [--blocks 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pinns-tf2.0_amd"))
sys.path.insert(0, os.path.join(ROOT, "pinns-tf2.0_amd", "1d-burgers"))
import pinn_native  # noqa: E402
import burgersutil  # noqa: E402

LAYERS = [2] + [20] * 8 + [1]
MAX_ITER = 100000                     # L-BFGS never reaches it here: every timed iteration is a real one


def glorot(rs):
    from scipy.stats import truncnorm
    out = []
    for fi, fo in zip(LAYERS[:-1], LAYERS[1:]):
        out.append(truncnorm.rvs(-2, 2, size=(fi, fo), random_state=rs).ravel() * np.sqrt(2.0 / (fi + fo)) / 0.87962566103423978)
        out.append(np.zeros(fo))
    return np.concatenate(out)


def timed(fn, n, seconds, blocks):
    """median seconds per unit of fn(n_units) over `blocks` blocks of >= seconds each"""
    fn(max(n // 10, 1))                                   # warm-up
    t0 = time.perf_counter()
    fn(n)
    dt = time.perf_counter() - t0
    n = max(int(n * seconds / max(dt, 1e-6) * 1.1), 1)
    per = []
    for _ in range(blocks):
        t0 = time.perf_counter()
        fn(n)
        per.append((time.perf_counter() - t0) / n)
    return float(np.median(per)), n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="1,2,4,8,16,32")
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--blocks", type=int, default=3)
    a = ap.parse_args()
    np.random.seed(1234)
    r = burgersutil.prep_data(os.path.join(ROOT, "pinns-tf2.0_amd", "1d-burgers", "data", "burgers_shock.mat"), 100, 10000,
                              noise=0.0)
    X_u, u, X_f, ub, lb = r[7], r[8], r[9], r[10], r[11]
    rs = np.random.RandomState(7)
    W = np.stack([glorot(rs) for _ in range(64)])

    def setup(e):
        e.set_collocation(X_f)
        e.set_data(X_u, u)
        e.set_pde_params(0.01 / np.pi)

    out = {"workload": "burgers f64 8x20, N_f=10000, N_u=100, kernel path 7", "seconds_per_block": a.seconds,
           "blocks": a.blocks, "device": pinn_native.device_info(0)["name"], "adam": {}, "lbfgs": {}}
    eng = pinn_native.Engine(LAYERS, lb, ub, pde="burgers", dtype="f64")
    setup(eng)
    eng.set_weights(W[0])
    eng.adam_init(1e-4)
    s, n = timed(lambda k: eng.adam_run(k), 200, a.seconds, a.blocks)
    out["solo"] = {"adam_step_us": s * 1e6, "adam_steps_per_s": 1.0 / s}
    eng.lbfgs_begin(MAX_ITER, 0.8, 50, 0.0, 0.0)
    s, n = timed(lambda k: eng.lbfgs_collect(eng.lbfgs_enqueue(k)), 200, a.seconds, a.blocks)
    out["solo"].update({"lbfgs_iter_us": s * 1e6, "lbfgs_iters_per_s": 1.0 / s})
    eng.close()
    for K in [int(v) for v in a.ks.split(",")]:
        ens = pinn_native.Ensemble(LAYERS, lb, ub, K)
        setup(ens)
        ens.set_weights(W[:K])
        ens.adam_init(1e-4)
        s, n = timed(lambda k: ens.adam_run(k), 100, a.seconds, a.blocks)
        out["adam"][str(K)] = {"step_us": s * 1e6, "member_steps_per_s": K / s,
                               "vs_solo": (K / s) / out["solo"]["adam_steps_per_s"], "steps_per_block": n}
        ens.lbfgs_begin(MAX_ITER, 0.8, 50, 0.0, 0.0)
        s, n = timed(lambda k: ens.lbfgs_run(k), 100, a.seconds, a.blocks)
        done = ens.lbfgs_run(0)[2]
        out["lbfgs"][str(K)] = {"iter_us": s * 1e6, "member_iters_per_s": K / s,
                                "vs_solo": (K / s) / out["solo"]["lbfgs_iters_per_s"], "iters_per_block": n,
                                "members_done": int(np.sum(done != 0))}
        ens.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
