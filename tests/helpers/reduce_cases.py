"""Loss, gradient, 3 Adam steps and 3 L-BFGS iterations on point sets chosen by their number of gradient rows, by whichever
library pinn_native loads (PINN_HIP_LIB names a variant build):

    python tests/helpers/reduce_cases.py OUT.npz [REPEATS]

The row count of the reduction kernels (csrc/kernels_optim.h, reduce_column) is the number of workgroups of the fused kernel:
ceil((N_f + N_u) / 64) while that is at most the number of compute units, the number of compute units beyond (tile loop).
Per case it writes `<case>/loss`, `/terms`, `/grad` (loss_grad), `/adam_losses`, `/adam_w` (3 Adam steps), `/lbfgs_iters`,
`/lbfgs_losses`, `/lbfgs_w` (lbfgs_begin + 3 iterations) and `/repeats_equal`: how many of REPEATS evaluations gave the bits
of the first (itself included).  tests/test_gpu_reduce_one_round.py runs it once per library and compares the files bit for
bit."""
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
N_U = 10
# a slice q of the 16 owns rows q, q + 16, ...: the smallest row counts at which a slice gains or loses a row (1, 2, 15-17),
# the eighth, ninth and tenth row of a slice come and go (112-145), the headline's 158 and its neighbours, and the second
# round of 8 fills up (255, 256)
ROWS = (1, 2, 15, 16, 17, 112, 113, 127, 128, 129, 143, 144, 145, 158, 159, 160, 161, 255, 256)
TILE_LOOP_TILES = 300          # more tiles than compute units (256): the tile loop, 256 rows
# engine kinds: float64 8x20 for every row count; the others where a slice has 1-2, 9-10 and 16 rows
KINDS = {"f64d8": ROWS + ("loop",), "f64d4": (17, 158, 256), "f32d8": (17, 158, 256), "ens2": (17, 158, 256)}


def case_ids():
    return ["%s-r%s" % (k, r) for k, rows in KINDS.items() for r in rows]


def n_f_of(rows):
    """collocation points for `rows` tiles with N_U data points, the last tile 57 points and 7 of padding"""
    tiles = TILE_LOOP_TILES if rows == "loop" else int(rows)
    return 64 * tiles - 7 - N_U


def point_set(n_f, seed):
    rs = np.random.RandomState(seed)
    X_f = LB + (UB - LB) * rs.uniform(size=(n_f, 2))
    x0 = rs.uniform(-1, 1, N_U)
    X_u = np.column_stack([x0, rs.uniform(0, 1, N_U)])
    return X_f, X_u, (-np.sin(np.pi * x0) * np.exp(-X_u[:, 1])).reshape(-1, 1)


def run_case(case, repeats):
    from oracle import init
    from pinn_native import Engine, Ensemble
    kind, rows = case.split("-r")
    depth = 4 if kind == "f64d4" else 8
    layers = [2] + [20] * depth + [1]
    X_f, X_u, u = point_set(n_f_of(rows if rows == "loop" else int(rows)), 11)
    w = init.glorot_flat(layers)
    w = w + 0.05 * np.random.RandomState(7).standard_normal(w.size)
    if kind == "ens2":
        eng = Ensemble(layers, LB, UB, 2)
        w = np.stack([w, w + 0.05 * np.random.RandomState(8).standard_normal(w.size)])
    else:
        eng = Engine(layers, LB, UB, pde="burgers", dtype="f32" if kind == "f32d8" else "f64")
    eng.set_collocation(X_f); eng.set_data(X_u, u); eng.set_pde_params(NU)
    eng.set_weights(w)
    if kind != "ens2":
        assert eng.kernel_path() == (2 if kind == "f32d8" else 7), eng.kernel_path()
    loss, grad, terms = eng.loss_grad()
    loss, grad, terms = np.array(loss, copy=True), np.array(grad, copy=True), np.array(terms, copy=True)
    same = 1
    for _ in range(repeats - 1):
        l2, g2, t2 = eng.loss_grad()
        same += int(np.array_equal(l2, loss) and np.array_equal(g2, grad) and np.array_equal(t2, terms))
    res = {"loss": loss, "grad": grad, "terms": terms, "repeats_equal": np.int64(same)}
    eng.adam_init(1e-3, 0.9, 0.999, 1e-7)
    res["adam_losses"] = np.array(eng.adam_run(3), copy=True)
    res["adam_w"] = np.array(eng.get_weights(), copy=True)
    eng.lbfgs_begin(50, 0.8, 50, np.finfo(float).eps)
    iters, losses, _ = eng.lbfgs_run(3)
    res["lbfgs_iters"] = np.concatenate([np.ravel(a) for a in iters]) if kind == "ens2" else np.asarray(iters)
    res["lbfgs_losses"] = np.concatenate([np.ravel(a) for a in losses]) if kind == "ens2" else np.asarray(losses)
    res["lbfgs_w"] = np.array(eng.get_weights(), copy=True)
    eng.close()
    return {"%s/%s" % (case, k): np.asarray(v) for k, v in res.items()}


def run_all(out, repeats=1):
    res = {}
    for case in case_ids():
        res.update(run_case(case, repeats))
    np.savez(out, **res)


if __name__ == "__main__":
    run_all(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 1)
    print("wrote", sys.argv[1])
