"""Per-Adam-step time of the default Allen-Cahn discrete-time shape (q = 100, [1,64,64,64,64,101], 200 points + 1 pair,
float64) as pde "adr_disc" or as "adr_disc_ide" with all six coefficients trained, one process per call, for alternating
A/B runs in one session (the method of profiles/time_disc_ab.py): 200 warm-up steps, then 9 repeats of 1000
steps between synchronisations.  Prints the repeats, their median, and digests of loss + gradient and of the weights after
all steps.  PINN_HIP_LIB names another build of the library (an older one: only "adr_disc").
    python profiles/time_adr_disc_ide.py adr_disc [tag];  python profiles/time_adr_disc_ide.py adr_disc_ide [tag]"""
import hashlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pinns-tf2.0_amd")
for p in (ROOT, PKG, os.path.join(PKG, "utils"), os.path.join(PKG, "1d-allen-cahn")):
    sys.path.insert(0, p)
import pinn_native  # noqa: E402

if os.environ.get("PINN_HIP_LIB"):
    # an older build may lack entry points this binding knows: do not bind those
    import subprocess
    syms = subprocess.run(["nm", "-D", os.environ["PINN_HIP_LIB"]], capture_output=True, text=True).stdout
    for name in list(pinn_native._SIGNATURES):
        if name not in syms:
            pinn_native._SIGNATURES.pop(name)
from irk import gauss_legendre_butcher  # noqa: E402
import allencahnutil as ac  # noqa: E402
from oracle import init  # noqa: E402

kind = sys.argv[1] if len(sys.argv) > 1 else "adr_disc_ide"
tag = sys.argv[2] if len(sys.argv) > 2 else kind
q, layers = 100, [1, 64, 64, 64, 64, 101]
x, t, E = ac.exact_field(None)
i0, i1 = int(np.argmin(np.abs(t[:, 0] - 0.1))), int(np.argmin(np.abs(t[:, 0] - 0.9)))
dt = float(t[i1, 0] - t[i0, 0])
rs = np.random.RandomState(1234)
pick = rs.choice(x.shape[0], 200, replace=False)
A, b, _ = gauss_legendre_butcher(q)
eng = pinn_native.Engine(layers, [-1.0], [1.0], pde=kind, dtype="f64")
eng.disc_set_stage(0, x[pick, 0], E[i0, pick], dt * np.vstack([A, b[None, :]]))
eng.disc_set_periodic([-1.0], [1.0], 1)
w = init.glorot_flat(layers)
if kind == "adr_disc_ide":
    eng.set_weights(np.concatenate([w, np.zeros(6)]))
    eng.set_pde_params(*ac.ADR_COEFFS)
    eng.set_pde_trainable(63)
else:
    eng.set_weights(w)
    eng.set_pde_params(*ac.ADR_COEFFS)
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
