"""kernel times of one evaluation at 1d-kdv/ide_disc_kdv.py's default shape by the engine's event timing
(pinn_timing_*), adrd_disc beside adr_disc_ide in both dtypes; run from the repository root (PINN_HIP_LIB chooses
the library: this commit's or the parent's)"""
import os, sys, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "pinns-tf2.0_amd")); sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import numpy as np
import pinn_native
from oracle import disc, init
q, layers = 50, [1, 50, 50, 50, 50, 50]
rs = np.random.RandomState(0)
x0, x1 = rs.uniform(-1, 1, 199), rs.uniform(-1, 1, 201)
A, b, _ = disc.gauss_legendre_butcher(q)
sol = lambda x, t: 1.5 / np.cosh(0.5 * np.sqrt(200.0) * (x - 0.5 * t + 0.3)) ** 2
sets = [(x0, sol(x0, 0.2), 0.6 * A), (x1, sol(x1, 0.8), -0.6 * (b[None, :] - A))]
w = init.glorot_flat(layers)
out = {"lib": os.environ.get("PINN_HIP_LIB", "tree")}
for pde, tail, dtype in [("adr_disc_ide", [0, 0.5, np.log(1e-3), 0, 0, 0], "f64"), ("adrd_disc", [0, 0.5, np.log(1e-3), 0, 0, 0, 0.005], "f64"),
                         ("adr_disc_ide", [0, 0.5, np.log(1e-3), 0, 0, 0], "f32"), ("adrd_disc", [0, 0.5, np.log(1e-3), 0, 0, 0, 0.005], "f32")]:
    try:
        eng = pinn_native.Engine(layers, [-1.0], [1.0], pde=pde, dtype=dtype)
    except (ValueError, pinn_native.PinnNativeError):      # a library from before the kind
        out[pde + "_" + dtype] = "no such kind"
        continue
    for k, st in enumerate(sets):
        eng.disc_set_stage(k, *st)
    eng.set_weights(np.concatenate([w, tail]))
    eng.set_pde_trainable(2 | (64 if pde == "adrd_disc" else 0))
    for _ in range(20):
        eng.loss_grad()
    eng.timing_enable(200)
    for _ in range(200):
        eng.loss_grad()
    t = eng.timing_read()
    out[pde + "_" + dtype] = {k: (round(float(v) * 1e3, 2) if k.endswith("_ms") else v) for k, v in t.items()}
    eng.close()
print("TIMING_US " + json.dumps(out))
