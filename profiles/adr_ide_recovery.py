#!/usr/bin/env python3
"""Coefficient recovery with the "adr_ide" kind, a first look (not a gate):
  allen_cahn  1d-allen-cahn/ide_cont_allen_cahn.py's model: nu, r1, r3 from N_u = 2000 samples of the split-step field,
              start [1e-3, -1, 1], truth [1e-4, -5, 5]
  burgers     a1 and nu from N_u = 2000 samples of burgers_shock.mat (start a1 = 0, log nu = -6, as the reference's
              identification script), against what pde "burgers_ide" reaches from the same start on the same schedule
Schedules and seeds are in the output.  Prints ONE JSON line; --out writes it too."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pinns-tf2.0_amd")
for p in (ROOT, PKG, os.path.join(PKG, "utils"), os.path.join(PKG, "1d-burgers"), os.path.join(PKG, "1d-allen-cahn")):
    sys.path.insert(0, p)
os.environ.setdefault("PINN_NO_PLOT", "1")

LAYERS = [2] + [20] * 8 + [1]


def schedule(a):
    return {"layers": LAYERS, "seed": a.seed, "tf_epochs": a.adam, "tf_lr": a.lr, "tf_b1": 0.9, "tf_eps": None,
            "nt_epochs": a.lbfgs, "nt_lr": 0.8, "nt_ncorr": 50, "log_frequency": 500}


def allen_cahn(a):
    argv, sys.argv = sys.argv, sys.argv[:1]           # the script reads an hp file from its command line
    try:
        import ide_cont_allen_cahn as script
    finally:
        sys.argv = argv
    from allencahnutil import ADR_COEFFS
    np.random.seed(a.seed)
    hp = dict(schedule(a), N_u=a.n_u, noise=0.0, adr_trainable=["nu", "r1", "r3"], adr_init=[0.0, 0.0, 1e-3, -1.0, 0.0, 1.0])
    pinn = script.run(hp)
    found = pinn.get_params(numpy=True)
    loss = pinn._engine.loss_grad(want_grad=False)[0]
    return {"hp": hp, "truth": list(ADR_COEFFS), "found": list(found), "final_loss": loss,
            "relative_error": script.relative_errors(found)}


def burgers(a):
    import burgersutil
    from logger import Logger
    from neuralnetwork import NeuralNetwork
    np.random.seed(a.seed)
    r = burgersutil.prep_data(os.path.join(PKG, "1d-burgers", "data", "burgers_shock.mat"), a.n_u, noise=0.0)
    X_u, u, ub, lb = r[7], r[8], r[9], r[10]
    truth = (1.0, 0.01 / np.pi)
    out = {"truth": list(truth)}

    class Ide(NeuralNetwork):
        pde = "burgers_ide"

        def _extra_params(self):
            return np.array([0.0, -6.0])

    hp = schedule(a)
    m = Ide(dict(hp), Logger(dict(hp)), ub, lb)
    m.logger.set_error_fn(lambda: 0.0)
    m.fit(X_u, u)
    w = m._engine.get_weights()
    out["burgers_ide"] = {"found": [float(w[-2]), float(np.exp(w[-1]))], "final_loss": m._engine.loss_grad(want_grad=False)[0]}

    hp2 = dict(hp, adr_trainable=["a1", "nu"], adr_init=[0.0, 0.0, float(np.exp(-6.0)), 0.0, 0.0, 0.0])
    m = NeuralNetwork(dict(hp2), Logger(dict(hp2)), ub, lb, pde="adr_ide")
    m._set_collocation(X_u)
    m.logger.set_error_fn(lambda: 0.0)
    m.fit(X_u, u)
    p = m.get_params(numpy=True)
    out["adr_ide"] = {"found": [p[1], p[2]], "all_six": list(p), "final_loss": m._engine.loss_grad(want_grad=False)[0]}
    for k in ("burgers_ide", "adr_ide"):
        f = out[k]["found"]
        out[k]["relative_error"] = [abs(f[0] - truth[0]) / truth[0], abs(f[1] - truth[1]) / truth[1]]
    out["hp"] = hp2
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--adam", type=int, default=2000)
    ap.add_argument("--lbfgs", type=int, default=2000)
    ap.add_argument("--lr", type=float, default=0.003)
    ap.add_argument("--n-u", dest="n_u", type=int, default=2000)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--out")
    a = ap.parse_args()
    import pinn_native
    res = {"device": pinn_native.device_info(0)["name"], "allen_cahn": allen_cahn(a), "burgers": burgers(a)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
