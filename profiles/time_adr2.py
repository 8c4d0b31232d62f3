"""time of one evaluation by the engine's event timing (pinn_timing_*), 200 evaluations after 20, at the headline
shape (8 x 20, N_f = 10 000, 100 data points) and at N_f = 40 000: pde "adr2" (wave coefficients, three-term wall points, a
source) beside pde "adr" with a zero source, on kernel path 7 (float64) and on path 0 (float64 and float32); run from
the repository root (PINN_HIP_LIB chooses the library: this commit's or the parent's, which has no "adr2")"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "pinns-tf2.0_amd"))
import numpy as np  # noqa: E402
import pinn_native  # noqa: E402
from oracle import init  # noqa: E402

layers = [2] + [20] * 8 + [1]
LB, UB = np.array([-1.0, 0.0]), np.array([1.0, 1.0])
w = init.glorot_flat(layers)
out = {"lib": os.environ.get("PINN_HIP_LIB", "tree")}
for N_f in (10000, 40000):
    rs = np.random.RandomState(0)
    X_f = LB + (UB - LB) * rs.uniform(size=(N_f, 2))
    X_u = np.column_stack([rs.uniform(-1, 1, 100), np.zeros(100)])
    u = -np.sin(np.pi * X_u[:, 0:1])
    for pde, path, dtype in (("adr", 7, "f64"), ("adr2", 7, "f64"), ("adr", 0, "f64"), ("adr2", 0, "f64"), ("adr", 0, "f32"),
                             ("adr2", 0, "f32")):
        key = "%s_path%d_%s_Nf%d" % (pde, path, dtype, N_f)
        try:
            eng = pinn_native.Engine(layers, LB, UB, pde=pde, dtype=dtype)
        except (ValueError, pinn_native.PinnNativeError):      # a library from before the kind
            out[key] = "no such kind"
            continue
        eng.set_collocation(X_f)
        eng.set_data(X_u, u)
        if pde == "adr2":
            eng.set_pde_params(0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, -1.0)
            eng.set_robin3(X_u, 0.0, 0.0, 1.0, 0.0)
            eng.set_source(np.sin(X_f[:, 0]))
        else:
            eng.set_source(np.zeros(N_f))
        eng.set_kernel_path(path)
        eng.set_weights(w)
        for _ in range(20):
            eng.loss_grad()
        eng.timing_enable(200)
        for _ in range(200):
            eng.loss_grad()
        t = eng.timing_read()
        out[key] = {k: (round(float(v) * 1e3, 2) if k.endswith("_ms") else v) for k, v in t.items()}
        eng.close()
print("TIMING_US " + json.dumps(out))
