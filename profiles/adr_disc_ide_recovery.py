"""What pde "adr_disc_ide" recovers from two snapshots, recorded and not gated: writes
profiles/adr_disc_ide_recovery.json with the schedules and seeds inside.

  allen_cahn  1d-allen-cahn/ide_disc_allen_cahn.py's default run (r1, r3 trained from -2, 2; truth -5, 5)
  heat        the heat mode u = exp(-nu pi^2 t) sin(pi x), nu = 0.1, snapshots at t = 0.1 and 0.9, nu trained from 2 x the
              truth, every other coefficient frozen at 0 (a linear case with a closed form)

    python profiles/adr_disc_ide_recovery.py [allen_cahn] [heat]"""
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pinns-tf2.0_amd")
for p in (ROOT, PKG, os.path.join(PKG, "utils"), os.path.join(PKG, "1d-allen-cahn")):
    sys.path.insert(0, p)
os.environ.setdefault("PINN_NO_PLOT", "1")
cases = [a for a in sys.argv[1:] if a in ("allen_cahn", "heat")] or ["allen_cahn", "heat"]
sys.argv = sys.argv[:1]                      # the script reads an hp file from its own command line
mod = importlib.import_module("ide_disc_allen_cahn")
from logger import Logger  # noqa: E402
from neuralnetwork import ADR_NAMES, set_seed  # noqa: E402
from irk import gauss_legendre_butcher  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "adr_disc_ide_recovery.json")


def report(pinn, hp, truth, losses):
    found = pinn.get_params(numpy=True)
    rel = {n: (abs(found[k] - truth[k]) / abs(truth[k]) if truth[k] != 0.0 else None) for k, n in enumerate(ADR_NAMES)
           if n in hp["adr_trainable"]}
    return {"hp": hp, "truth": list(truth), "start": list(hp["adr_init"]), "found": list(found), "relative_error": rel,
            "loss_first": losses[0], "loss_last": losses[-1]}


def run_allen_cahn():
    np.random.seed(1234)
    set_seed(1234)
    hp = json.loads(json.dumps(mod.hp))
    hp["seed_numpy"], hp["seed_init"] = 1234, 1234
    x_0, u_0, x_1, u_1, _, _, dt, q, _, al, be, _, _ = mod.prep_data(hp["N_0"], hp["N_1"], hp["q"], hp["t_0"], hp["t_1"])
    hp["layers"][-1] = q
    pinn = mod.AllenCahnDiscreteIdentificationNN(hp, Logger(hp), dt, np.array([-1.0]), np.array([1.0]), q, al, be)
    pinn.logger.set_error_fn(lambda: 0.0)
    first = pinn.loss(x_0, u_0, x_1, u_1)
    pinn.fit(x_0, u_0, x_1, u_1)
    return report(pinn, hp, mod.ADR_COEFFS, [first, pinn.loss(x_0, u_0, x_1, u_1)])


def run_heat():
    nu, t_0, t_1, q = 0.1, 0.1, 0.9, 16
    np.random.seed(4321)
    set_seed(4321)
    hp = {"N_0": 100, "N_1": 100, "q": q, "layers": [1, 32, 32, q], "t_0": t_0, "t_1": t_1,
          "tf_epochs": 2000, "tf_lr": 0.001, "tf_b1": 0.9, "tf_eps": 1e-08, "nt_epochs": 10000, "nt_lr": 0.8, "nt_ncorr": 50,
          "log_frequency": 1000, "adr_trainable": ["nu"], "adr_init": [0.0, 0.0, 2.0 * nu, 0.0, 0.0, 0.0],
          "seed_numpy": 4321, "seed_init": 4321}
    u = lambda x, t: np.exp(-nu * np.pi ** 2 * t) * np.sin(np.pi * x)
    x_0, x_1 = np.random.uniform(-1, 1, (hp["N_0"], 1)), np.random.uniform(-1, 1, (hp["N_1"], 1))
    A, b, _ = gauss_legendre_butcher(q)
    pinn = mod.AllenCahnDiscreteIdentificationNN(hp, Logger(hp), t_1 - t_0, np.array([-1.0]), np.array([1.0]), q, A, b[None, :])
    pinn.logger.set_error_fn(lambda: abs(pinn.get_params(numpy=True)[2] - nu) / nu)
    args = (x_0, u(x_0, t_0), x_1, u(x_1, t_1))
    first = pinn.loss(*args)
    pinn.fit(*args)
    return report(pinn, hp, (0.0, 0.0, nu, 0.0, 0.0, 0.0), [first, pinn.loss(*args)])


if __name__ == "__main__":
    out = {}
    if os.path.exists(OUT):
        with open(OUT) as f:
            out = json.load(f)
    for c in cases:
        out[c] = run_allen_cahn() if c == "allen_cahn" else run_heat()
        print(c, json.dumps(out[c]["relative_error"]), out[c]["found"], flush=True)
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
