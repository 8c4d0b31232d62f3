"""The cells tests/test_gpu_adr_var.py evaluates on the device and tests/test_adr_var_host.py checks on the CPU for not being
vacuous: sets, weights and cell scheme of tests/test_gpu_adr_source.py (the same seeds, so the same points), the test fields

    K[:, j] = b_j (1 + 0.3 sin((j + 2) x + j) exp(-t / (j + 1))),      b_j = c_j + 3 sgn(c_j)   (sgn(0) = +1)

with c the cell's constant set -- every column within 30 % of b_j, so nu stays > 0; the six columns distinct at every point, so
a shifted index, a swapped column or a read of the constants fails -- and the restatement of a cell, computed once and shared.

Why the base is c_j shifted by 3 and not c_j itself (0.1 where that is 0): the fields have to move the loss of every cell by at
least 10 % against the restatement with the constant set c (tests/test_adr_var_host.py asserts it), or a kernel that read the
constants would pass the loss check of that cell.  The net of these cells is a perturbed Glorot draw whose channels are small
(rms u 0.10, u_x 0.05, u_t 0.18, u_xx 0.10) beside the source (rms 0.8), so with the base c_j a 30 % modulation of the
coefficients moved the loss by 7e-5 (a Robin cell without source) to 3 % only; with shifts of 0.5, 1 and 2 the smallest
movement was 2e-4, 4e-3 and 7 %, with 3 it is 15 %."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adr_ref  # noqa: E402
import adr_src_ref  # noqa: E402
import adr_var_ref  # noqa: E402

LB, UB = np.array([-1.0, 0.0]), np.array([1.0, 1.0])

# (2 n_b + n_0) points stand in front of the collocation block: table row 0 at lane 0, 1, 14, 15, at point 50 and at the
# first lane of the second tile
OFFSETS = {0: (0, 0), 1: (0, 1), 14: (7, 0), 15: (7, 1), 50: (0, 50), 64: (7, 50)}       # offset -> (n_b, n_0)
BLOCKS = (1, 15, 16, 17, 64, 2048)


def layers_of(depth, width=20):
    return [2] + [width] * depth + [1]


def source_of(X):
    return np.sin(3.0 * X[:, 0]) * np.exp(-X[:, 1]) + 0.5


def fields_of(X, coeffs):
    X = np.asarray(X, dtype=np.float64)
    x, t = X[:, 0], X[:, 1]
    K = np.empty((X.shape[0], 6))
    for j in range(6):
        c = float(coeffs[j]) + (3.0 if float(coeffs[j]) >= 0.0 else -3.0)
        K[:, j] = c * (1.0 + 0.3 * np.sin((j + 2) * x + j) * np.exp(-t / (j + 1)))
    return K


@functools.lru_cache(maxsize=None)
def weights(depth, seed=7):
    """a glorot draw plus 0.05 * standard_normal: biases non-zero"""
    from oracle import init
    w = init.glorot_flat(layers_of(depth))
    w = w + 0.05 * np.random.RandomState(seed).standard_normal(w.size)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def point_sets(N_f, n_0=512, n_b=50, seed=3):
    """collocation points, initial data u(x, 0) = x^2 cos(pi x), n_b wall pairs, the source at the collocation points"""
    rs = np.random.RandomState(seed)
    X_f = LB + (UB - LB) * rs.uniform(size=(N_f, 2))
    x0 = rs.uniform(-1, 1, n_0)
    X_u = np.column_stack([x0, np.zeros(n_0)])
    u = (x0 * x0 * np.cos(np.pi * x0)).reshape(-1, 1)
    tb = rs.uniform(0, 1, n_b)
    X_lo, X_hi = np.column_stack([np.full(n_b, -1.0), tb]), np.column_stack([np.full(n_b, 1.0), tb])
    s = source_of(X_f)
    for a in (X_f, X_u, u, X_lo, X_hi, s):
        a.setflags(write=False)
    return X_f, X_u, u, X_lo, X_hi, s


@functools.lru_cache(maxsize=None)
def robin_points(n_w, seed=11):
    """x alternating between the walls, random t, alpha, beta in U(-1.5, 1.5) with every fifth alpha and every seventh beta 0
    (never both: such a point is refused), g in U(-1, 1)"""
    if n_w == 0:
        return None
    rs = np.random.RandomState(seed)
    j = np.arange(n_w)
    X_w = np.column_stack([np.where(j % 2, 1.0, -1.0), rs.uniform(0, 1, n_w)])
    alpha, beta, g = rs.uniform(-1.5, 1.5, n_w), rs.uniform(-1.5, 1.5, n_w), rs.uniform(-1, 1, n_w)
    alpha[j % 5 == 4] = 0.0
    beta[(j % 7 == 6) & (alpha != 0.0)] = 0.0
    for a in (X_w, alpha, beta, g):
        a.setflags(write=False)
    return X_w, alpha, beta, g


@functools.lru_cache(maxsize=None)
def cell_fields(name, N_f, n_0, n_b):
    K = fields_of(point_sets(N_f, n_0, n_b)[0], adr_ref.COEFF_SETS[name])
    K.setflags(write=False)
    return K


def _cell_args(depth, N_f, n_0, n_b):
    X_f, X_u, u, X_lo, X_hi, s = point_sets(N_f, n_0, n_b)
    return (weights(depth), layers_of(depth), LB, UB, X_f, X_u if n_0 else None, u if n_0 else None,
            X_lo if n_b else None, X_hi if n_b else None), s


@functools.lru_cache(maxsize=None)
def reference(depth, name, N_f, n_0, n_b, n_w, with_source):
    """the restatement with the test fields on a cell: computed once, shared, never written to"""
    args, s = _cell_args(depth, N_f, n_0, n_b)
    return adr_var_ref.var_loss_grad(*args, cell_fields(name, N_f, n_0, n_b), s if with_source else None,
                                     *(robin_points(n_w) or ()))


@functools.lru_cache(maxsize=None)
def constant_loss(depth, name, N_f, n_0, n_b, n_w, with_source):
    """the loss of the same cell with the cell's constant set instead of the fields"""
    args, s = _cell_args(depth, N_f, n_0, n_b)
    return adr_src_ref.src_loss_grad(*args, adr_ref.COEFF_SETS[name], s if with_source else None,
                                     *(robin_points(n_w) or ()))[0]


# the cells of the GPU file's parity tests: (tag, depth, name, N_f, n_0, n_b, n_w, with_source)
def variant_cells():
    return [("a:d%d:Nf%d" % (d, N_f), d, "all_nonzero", N_f, 512, 0, 0, True) for d in (4, 6, 8) for N_f in (2048, 40000)]


def alignment_cells():
    return [("b:Nf%d:off%d" % (N_f, off), 8, "all_nonzero", N_f, n_0, n_b, 0, True)
            for N_f in BLOCKS for off, (n_b, n_0) in sorted(OFFSETS.items())]


def robin_cells():
    return [("c:nw%d:%s" % (n_w, "src" if src else "nosrc"), 8, "all_nonzero", 2048, 512, 7, n_w, src)
            for n_w in (0, 1, 50) for src in (True, False)]


def equation_cells():
    return [("d:%s" % name, 8, name, 2048, 512, 50, 0, True) for name in sorted(adr_ref.COEFF_SETS)]


def all_cells():
    return variant_cells() + alignment_cells() + robin_cells() + equation_cells()
