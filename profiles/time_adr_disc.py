"""Per-step time of the default inf_disc_allen_cahn shape (q = 100, [1,64,64,64,64,101], 200 points + 1 pair, float64):
host clock around synchronised Adam runs (9 x 1000 steps after 200 warm-up steps), and the engine's own event timing
(pinn_timing_*) over 200 evaluations.    python profiles/time_adr_disc.py"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pinns-tf2.0_amd")
for p in (ROOT, PKG, os.path.join(PKG, "utils"), os.path.join(PKG, "1d-allen-cahn")):
    sys.path.insert(0, p)
import pinn_native  # noqa: E402
from irk import gauss_legendre_butcher  # noqa: E402
import allencahnutil as ac  # noqa: E402
from oracle import init  # noqa: E402

q, layers = 100, [1, 64, 64, 64, 64, 101]
x, t, E = ac.exact_field(None)
i0, i1 = int(np.argmin(np.abs(t[:, 0] - 0.1))), int(np.argmin(np.abs(t[:, 0] - 0.9)))
dt = float(t[i1, 0] - t[i0, 0])
rs = np.random.RandomState(1234)
pick = rs.choice(x.shape[0], 200, replace=False)
A, b, _ = gauss_legendre_butcher(q)
eng = pinn_native.Engine(layers, [-1.0], [1.0], pde="adr_disc", dtype="f64")
eng.disc_set_stage(0, x[pick, 0], E[i0, pick], dt * np.vstack([A, b[None, :]]))
eng.disc_set_periodic([-1.0], [1.0], 1)
eng.set_pde_params(*ac.ADR_COEFFS)
eng.set_weights(init.glorot_flat(layers))
print("loss", eng.loss_grad()[0], eng.loss_grad()[2])
eng.adam_init(1e-3, 0.9, 0.999, 1e-8)
eng.adam_run(200, want_losses=False)
eng.sync()
us = []
for rep in range(9):
    t0 = time.perf_counter()
    eng.adam_run(1000, want_losses=False)
    eng.sync()
    us.append((time.perf_counter() - t0) / 1000 * 1e6)
print("allen-cahn disc default shape f64: us/Adam step %s  median %.2f min %.2f max %.2f"
      % (" ".join("%.2f" % v for v in us), np.median(us), min(us), max(us)))
eng.timing_enable(200)
eng.adam_run(200, want_losses=False)
eng.sync()
print("pinn_timing:", eng.timing_read(), flush=True)
eng.close()
