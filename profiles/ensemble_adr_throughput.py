#!/usr/bin/env python3
"""Member throughput of an ensemble of the adr kind (pinn_native.AdrEnsemble) against a solo Engine(pde="adr") in the same
process: Allen-Cahn, float64, 8 x 20, N_f = 10^4 with the script's default N_0 = 512 initial points and N_b = 200 wall pairs,
kernel path 7.

The solo engine and every ensemble are built first; then the timed blocks ALTERNATE -- one block of the solo engine, one of
each K, and round again -- so that a drift of the clocks or of the machine's other load falls on all of them alike.  For each:
Adam member-steps/s = K x steps / s and L-BFGS member-iterations/s, each the median over `--blocks` blocks of >= `--seconds`
s (the block length is calibrated first; every block ends with the host reading the losses, as adam_run / lbfgs_run do),
and the ratio to the solo engine's rate in this process.  Prints ONE JSON line (and writes it to --out).
    python profiles/ensemble_adr_throughput.py [--ks 1,2,4,8,16] [--seconds 1.0] [--blocks 3] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pinns-tf2.0_amd"))
sys.path.insert(0, os.path.join(ROOT, "pinns-tf2.0_amd", "1d-allen-cahn"))
import pinn_native  # noqa: E402
import allencahnutil  # noqa: E402

LAYERS = [2] + [20] * 8 + [1]
MAX_ITER = 1000000                    # L-BFGS never reaches it here: every timed iteration is a real one


def glorot(rs):
    from scipy.stats import truncnorm
    out = []
    for fi, fo in zip(LAYERS[:-1], LAYERS[1:]):
        out.append(truncnorm.rvs(-2, 2, size=(fi, fo), random_state=rs).ravel() * np.sqrt(2.0 / (fi + fo)) / 0.87962566103423978)
        out.append(np.zeros(fo))
    return np.concatenate(out)


def calibrate(fn, n, seconds):
    """units per block of >= seconds"""
    fn(max(n // 10, 1))                                   # warm-up
    t0 = time.perf_counter()
    fn(n)
    dt = time.perf_counter() - t0
    return max(int(n * seconds / max(dt, 1e-6) * 1.1), 1)


def alternate(fns, seconds, blocks):
    """fns: {name: fn(n_units)} -> {name: (median seconds per unit, units per block, [seconds per unit of every block])}"""
    n = {k: calibrate(fn, 100, seconds) for k, fn in fns.items()}
    per = {k: [] for k in fns}
    for _ in range(blocks):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            fn(n[k])
            per[k].append((time.perf_counter() - t0) / n[k])
    return {k: (float(np.median(v)), n[k], v) for k, v in per.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="1,2,4,8,16")
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    Ks = [int(v) for v in a.ks.split(",")]
    np.random.seed(1234)
    r = allencahnutil.prep_data(512, 200, 10000)
    X_u, u, X_f, X_lb, X_ub, ub, lb = r[7:14]
    rs = np.random.RandomState(7)
    W = np.stack([glorot(rs) for _ in range(max(Ks))])

    def setup(e):
        e.set_collocation(X_f)
        e.set_data(X_u, u)
        e.set_boundary(X_lb, X_ub)

    out = {"workload": "allen-cahn (adr) f64 8x20, N_f=10000, N_0=512, N_b=200, kernel path 7",
           "seconds_per_block": a.seconds, "blocks": a.blocks, "order": "alternating blocks: solo, then each K, repeated",
           "device": pinn_native.device_info(0)["name"], "adam": {}, "lbfgs": {}}
    eng = pinn_native.Engine(LAYERS, lb, ub, pde="adr", dtype="f64")
    setup(eng)
    eng.set_pde_params(*allencahnutil.ADR_COEFFS)
    eng.set_weights(W[0])
    assert eng.kernel_path() == 7
    ens = {}
    for K in Ks:
        e = pinn_native.AdrEnsemble(LAYERS, lb, ub, K)
        setup(e)
        e.set_pde_params(np.tile(np.asarray(allencahnutil.ADR_COEFFS), (K, 1)))     # a row per member, as a sweep sets them
        e.set_weights(W[:K])
        ens[K] = e

    eng.adam_init(1e-4)
    for e in ens.values():
        e.adam_init(1e-4)
    fns = {"solo": lambda n: eng.adam_run(n)}
    fns.update({str(K): (lambda n, e=e: e.adam_run(n)) for K, e in ens.items()})
    res = alternate(fns, a.seconds, a.blocks)
    s = res["solo"][0]
    out["solo"] = {"adam_step_us": s * 1e6, "adam_steps_per_s": 1.0 / s, "adam_block_us": [v * 1e6 for v in res["solo"][2]]}
    for K in Ks:
        s, n, v = res[str(K)]
        out["adam"][str(K)] = {"step_us": s * 1e6, "member_steps_per_s": K / s,
                               "vs_solo": (K / s) / out["solo"]["adam_steps_per_s"], "steps_per_block": n,
                               "block_us": [x * 1e6 for x in v]}

    eng.lbfgs_begin(MAX_ITER, 0.8, 50, 0.0, 0.0)
    for e in ens.values():
        e.lbfgs_begin(MAX_ITER, 0.8, 50, 0.0, 0.0)
    fns = {"solo": lambda n: eng.lbfgs_collect(eng.lbfgs_enqueue(n))}
    fns.update({str(K): (lambda n, e=e: e.lbfgs_run(n)) for K, e in ens.items()})
    res = alternate(fns, a.seconds, a.blocks)
    s = res["solo"][0]
    out["solo"].update({"lbfgs_iter_us": s * 1e6, "lbfgs_iters_per_s": 1.0 / s,
                        "lbfgs_block_us": [v * 1e6 for v in res["solo"][2]], "nonfinite": int(eng.status()[1] != 0)})
    for K in Ks:
        s, n, v = res[str(K)]
        done = ens[K].lbfgs_run(0)[2]
        out["lbfgs"][str(K)] = {"iter_us": s * 1e6, "member_iters_per_s": K / s,
                                "vs_solo": (K / s) / out["solo"]["lbfgs_iters_per_s"], "iters_per_block": n,
                                "block_us": [x * 1e6 for x in v], "members_done": int(np.sum(done != 0)),
                                "members_nonfinite": int(np.sum(ens[K].status()[1] != 0))}
    eng.close()
    for e in ens.values():
        e.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
