"""Loss + gradient of the float64 one-tile kernels (k_fused20d<., ., true>, kernel path 7) on a fixed list of cases, by whichever
library pinn_native loads (PINN_HIP_LIB names a variant build):

    python tests/helpers/onetile_cases.py OUT.npz [REPEATS]

writes `<case>/loss`, `<case>/grad`, `<case>/terms` per case and, for the ragged cases when REPEATS is given,
`<case>/repeats_equal`: how many of REPEATS evaluations gave the bits of the first (itself included).
tests/test_gpu_onetile_fold.py runs it once per library and compares the files bit for bit.  Every set has at most 64 points per compute unit, so each tile has a workgroup of its own."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "pinns-tf2.0_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

LB, UB = np.array([-1.0, 0.0]), np.array([1.0, 1.0])
NU = 0.01 / np.pi
PDES = ("burgers", "burgers_ide", "adr")
DEPTHS = (4, 6, 8)
WEIGHTS = ("canonical", "perturbed")
# (collocation points, data points, boundary pairs): whole tiles, and one set whose last tile is partly padding
FULL = (3968, 128, 0)         # 4096 points = 64 tiles
RAGGED = (2000, 37, 0)        # 2037 points: 31 tiles and 53 points
RAGGED_ADR = (2000, 37, 9)    # 2055 points with the 9 pairs


def case_ids():
    ids = ["%s-d%d-%s-full" % (p, d, w) for p in PDES for d in DEPTHS for w in WEIGHTS]
    return ids + ["%s-d8-perturbed-ragged" % p for p in PDES]


def point_sets(n_f, n_u, n_b, seed=11):
    rs = np.random.RandomState(seed)
    X_f = LB + (UB - LB) * rs.uniform(size=(n_f, 2))
    x0 = rs.uniform(-1, 1, n_u)
    X_u = np.column_stack([x0, rs.uniform(0, 1, n_u)])
    u = (-np.sin(np.pi * x0) * np.exp(-X_u[:, 1])).reshape(-1, 1)
    tb = rs.uniform(0, 1, n_b)
    return X_f, X_u, u, np.column_stack([np.full(n_b, -1.0), tb]), np.column_stack([np.full(n_b, 1.0), tb])


def engine_for(case):
    """-> engine with sets and weights of the case in place, on path 7"""
    import adr_ref
    from oracle import init
    from pinn_native import Engine
    pde, depth, wkind, skind = case.split("-")
    depth = int(depth[1:])
    layers = [2] + [20] * depth + [1]
    n_f, n_u, n_b = FULL if skind == "full" else RAGGED_ADR if pde == "adr" else RAGGED
    if pde == "adr" and skind == "full":
        n_f, n_b = n_f - 64, 32
    X_f, X_u, u, X_lo, X_hi = point_sets(n_f, n_u, n_b)
    eng = Engine(layers, LB, UB, pde=pde, dtype="f64")
    if pde == "burgers":
        eng.set_collocation(X_f); eng.set_data(X_u, u); eng.set_pde_params(NU)
    elif pde == "burgers_ide":                       # the data points carry the residual
        eng.set_data(np.vstack([X_f, X_u]), np.vstack([np.tanh(X_f[:, :1] - X_f[:, 1:]), u]))
    else:
        eng.set_pde_params(*adr_ref.ALLEN_CAHN)
        eng.set_collocation(X_f); eng.set_data(X_u, u); eng.set_boundary(X_lo, X_hi)
    eng.set_kernel_path(7)
    assert eng.kernel_path() == 7
    w = init.glorot_flat(layers)
    if eng.n_params == w.size + 2:
        w = np.concatenate([w, [0.0, -6.0]])
    assert eng.n_params == w.size
    if wkind == "perturbed":
        w = w + 0.05 * np.random.RandomState(7).standard_normal(w.size)
    eng.set_weights(w)
    return eng


def run_all(out, repeats=0):
    res = {}
    for case in case_ids():
        eng = engine_for(case)
        loss, grad, terms = eng.loss_grad()
        grad, terms = np.array(grad, copy=True), np.array(terms, copy=True)
        if repeats and case.endswith("ragged"):
            same = 1
            for _ in range(repeats - 1):
                l2, g2, t2 = eng.loss_grad()
                same += int(l2 == loss and np.array_equal(g2, grad) and np.array_equal(t2, terms))
            res[case + "/repeats_equal"] = np.int64(same)
        eng.close()
        res[case + "/loss"] = np.float64(loss)
        res[case + "/grad"] = np.asarray(grad, dtype=np.float64)
        res[case + "/terms"] = np.asarray(terms, dtype=np.float64)
    np.savez(out, **res)


if __name__ == "__main__":
    run_all(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 0)
    print("wrote", sys.argv[1])
