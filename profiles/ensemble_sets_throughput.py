#!/usr/bin/env python3
"""Adam step time of an ensemble on shared point sets against the same ensemble size on one point set per member
(pinn_native.Ensemble set_* with [K, ...] arrays, include/pinn_hip.h pinn_ensk_*), float64 Burgers inference at the default
size (N_f = 10^4, N_u = 100, 8 x 20, kernel path 7), both in one process.

The two ensembles are timed in alternating blocks (shared, per-member, shared, ...) of >= `--seconds` s each, so that
clock and thermal drift hit both alike; reported: the median step time of each and their ratio.  Also the time of one
device-side redraw of all members' collocation sets (lhs_collocation), the per-member analogue of Engine.lhs_collocation.
Prints ONE JSON line.
    python profiles/ensemble_sets_throughput.py [--k 8] [--seconds 1.0] [--blocks 5]"""
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
MAT = os.path.join(ROOT, "pinns-tf2.0_amd", "1d-burgers", "data", "burgers_shock.mat")


def glorot(rs):
    out = []
    for fi, fo in zip(LAYERS[:-1], LAYERS[1:]):
        out.append(np.clip(rs.standard_normal(fi * fo), -2, 2) * np.sqrt(2.0 / (fi + fo)) / 0.87962566103423978)
        out.append(np.zeros(fo))
    return np.concatenate(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--blocks", type=int, default=5)
    a = ap.parse_args()
    K = a.k
    sets = []
    for k in range(K):                                   # member k's bag: prep_data after np.random.seed(1234 + k)
        np.random.seed(1234 + k)
        r = burgersutil.prep_data(MAT, 100, 10000, noise=0.0)
        sets.append(r[7:12])
    ub, lb = sets[0][3], sets[0][4]
    rs = np.random.RandomState(7)
    W = np.stack([glorot(rs) for _ in range(K)])
    nu = 0.01 / np.pi * (1.0 + 0.1 * np.arange(K))

    shared = pinn_native.Ensemble(LAYERS, lb, ub, K)
    shared.set_collocation(sets[0][2])
    shared.set_data(sets[0][0], sets[0][1])
    shared.set_pde_params(0.01 / np.pi)
    per = pinn_native.Ensemble(LAYERS, lb, ub, K)
    per.set_collocation(np.stack([s[2] for s in sets]))
    per.set_data(np.stack([s[0] for s in sets]), np.stack([s[1] for s in sets]))
    per.set_pde_params(nu)
    for e in (shared, per):
        e.set_weights(W)
        e.adam_init(1e-4)
        e.adam_run(200)                                  # warm-up (sets uploaded, plan made)

    t0 = time.perf_counter()
    shared.adam_run(500)
    n = max(int(500 * a.seconds / max(time.perf_counter() - t0, 1e-6)), 1)
    times = {"shared": [], "per_member": []}
    for _ in range(a.blocks):
        for name, e in (("shared", shared), ("per_member", per)):
            t0 = time.perf_counter()
            e.adam_run(n)
            times[name].append((time.perf_counter() - t0) / n)

    seeds = np.arange(K, dtype=np.uint64) + np.uint64(77)
    per.lhs_collocation(10000, seeds)
    per.loss_grad(want_grad=False)                      # sets rebuilt for the design; the next draws are in place
    reps = 200
    t0 = time.perf_counter()
    for i in range(reps):
        per.lhs_collocation(10000, seeds + np.uint64(i))
    per.loss_grad(want_grad=False)
    lhs_us = (time.perf_counter() - t0) / reps * 1e6

    med = {k: float(np.median(v)) for k, v in times.items()}
    out = {"workload": "burgers f64 8x20, N_f=10000, N_u=100, kernel path 7, Adam", "members": K,
           "device": pinn_native.device_info(0)["name"], "steps_per_block": n, "blocks": a.blocks,
           "shared_step_us": med["shared"] * 1e6, "per_member_step_us": med["per_member"] * 1e6,
           "per_member_over_shared": med["per_member"] / med["shared"],
           "shared_blocks_us": [v * 1e6 for v in times["shared"]],
           "per_member_blocks_us": [v * 1e6 for v in times["per_member"]],
           "lhs_redraw_all_members_us": lhs_us}
    print(json.dumps(out))
    shared.close()
    per.close()


if __name__ == "__main__":
    main()
