"""Per-Adam-step time of the default inf_disc_burgers shape (q = 500, [1,50,50,50,501], 250 + 2 points, float64) with the
library PINN_HIP_LIB names (or the tree's own): for A/B comparisons of two builds, one process each, alternating
(DESIGN.md 4.15).  200 warm-up steps, then 9 repeats of 1000 steps between synchronisations.  Prints the repeats, their
median, and digests of loss + gradient and of the weights after all steps (two builds that compute the same print the same).
    PINN_HIP_LIB=/path/to/other/libpinn_hip.so python profiles/time_disc_ab.py parent;  python profiles/time_disc_ab.py new"""
import hashlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pinns-tf2.0_amd")
for p in (ROOT, PKG, os.path.join(PKG, "utils"), os.path.join(PKG, "1d-burgers")):
    sys.path.insert(0, p)
import pinn_native  # noqa: E402

if os.environ.get("PINN_HIP_LIB"):
    # an older build may lack entry points this binding knows: do not bind those
    import subprocess
    syms = subprocess.run(["nm", "-D", os.environ["PINN_HIP_LIB"]], capture_output=True, text=True).stdout
    for name in list(pinn_native._SIGNATURES):
        if name not in syms:
            pinn_native._SIGNATURES.pop(name)
import burgersutil  # noqa: E402
from oracle import disc, init  # noqa: E402

tag = sys.argv[1] if len(sys.argv) > 1 else "lib"
lb, ub = np.array([-1.0]), np.array([1.0])
np.random.seed(1234)
r = burgersutil.prep_data(os.path.join(PKG, "1d-burgers", "data", "burgers_shock.mat"), N_n=250, q=500, lb=lb, ub=ub,
                          noise=0.0, idx_t_0=10, idx_t_1=90)
layers = [1, 50, 50, 50, 501]
sets = disc.inference_sets(r[4], r[5], r[6], r[2], r[9])
w = init.glorot_flat(layers)
eng = pinn_native.Engine(layers, lb, ub, pde="burgers_disc", dtype="f64")
for s, (x, t, M) in enumerate(sets):
    eng.disc_set_stage(s, x, t, M)
eng.set_pde_params(0.01 / np.pi)
eng.set_weights(w)
loss, grad, terms = eng.loss_grad()
h = hashlib.sha256(np.float64(loss).tobytes() + grad.tobytes() + terms.tobytes()).hexdigest()[:16]
eng.adam_init(1e-3, 0.9, 0.999, 1e-8)
eng.adam_run(200, want_losses=False)
eng.sync()
N, us = 1000, []
for rep in range(9):
    t0 = time.perf_counter()
    eng.adam_run(N, want_losses=False)
    eng.sync()
    us.append((time.perf_counter() - t0) / N * 1e6)
wsum = hashlib.sha256(eng.get_weights().tobytes()).hexdigest()[:16]
print("%s loss %.15e digest %s weights-after %s  us/step %s  median %.2f min %.2f max %.2f"
      % (tag, loss, h, wsum, " ".join("%.2f" % v for v in us), np.median(us), min(us), max(us)), flush=True)
eng.close()
