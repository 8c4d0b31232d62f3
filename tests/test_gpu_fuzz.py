"""GPU: randomized shape sweep of the continuous models through the C ABI against the oracle -- widths 1..128,
2..12 dense layers, ragged point counts, all three residual kinds, f64 (1e-10) and f32 (5e-5): every kernel family
the engine can choose for a shape (generic, HBM-stash width-20, register-stash 8x20, wide MFMA, shape-generic MFMA
tile16 -- also each of its halves paired with the generic other half, paths 5 and 6) is hit by some case, and for
shapes with several eligible families all of them are compared."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import grad_entries as ge  # noqa: E402

pytestmark = pytest.mark.gpu

NU = 0.01 / np.pi
LB, UB = np.array([-1.0, 0.0]), np.array([1.0, 0.99])


def rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300)


def assert_entries(grad, judged, path, layers, dtype, record):
    """every entry on its own rounding scale (tests/helpers/grad_entries.py): the lambda gradients, 1e-5 of the largest
    entry, are invisible to rel()"""
    _, g_ref, A, yard, layout = judged
    dev, block, (row, col) = ge.entry_dev(grad, g_ref, A, layout)
    k = ge.K[(ge.family_of(path, layers, dtype), dtype)]
    record(path=path, entry_dev=dev, yardstick=yard, ratio=dev / yard, block=block, row=row, col=col)
    assert dev <= k * yard, "path %d: %s[%d,%d] is off by %.3e of its scale, bound %.3e" % (path, block, row, col, dev, k * yard)


def cases():
    rs = np.random.RandomState(2026)
    out = []
    fixed = [("burgers", 20, 8), ("burgers_ide", 20, 8), ("burgers", 20, 3), ("schrodinger", 100, 4),
             ("burgers", 100, 4), ("burgers_ide", 65, 4), ("schrodinger", 128, 4),      # the fused float64 sweep (path 8)
             ("schrodinger", 100, 2), ("burgers", 80, 3), ("burgers_ide", 112, 2),
             ("burgers", 1, 1), ("burgers", 128, 2), ("schrodinger", 24, 3), ("burgers_ide", 7, 11),
             # round 5, strip-granular launch plans of the fused float64 sweep (t16_deal): 124 = a 3-strip wave followed by
             # 16-row tiles that start at rows 76 / 92 / 108; 116 = edge strips AND 13 row strips; 68 / 97 = one strip beyond
             # a tile boundary (4 and 1 live rows)
             ("burgers", 124, 3), ("schrodinger", 116, 4), ("burgers_ide", 68, 2), ("burgers", 97, 4)]
    for pde, W, H in fixed:
        out.append((pde, W, H, int(rs.randint(1, 700)), int(rs.randint(1, 90)), int(rs.randint(0, 2 ** 31))))
    for _ in range(10):
        pde = ["burgers", "burgers_ide", "schrodinger"][rs.randint(3)]
        out.append((pde, int(rs.randint(1, 129)), int(rs.randint(1, 7)), int(rs.randint(1, 1500)),
                    int(rs.randint(1, 120)), int(rs.randint(0, 2 ** 31))))
    return out


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("pde_kind,W,H,n_f,n_u,seed", cases())
def test_random_shapes_against_oracle(pde_kind, W, H, n_f, n_u, seed, dtype, record):
    import pinn_native
    from oracle import pde
    rs = np.random.RandomState(seed)
    n_out = 2 if pde_kind == "schrodinger" else 1
    layers = [2] + [W] * H + [n_out]
    P = sum(a * b + b for a, b in zip(layers[:-1], layers[1:]))
    scale = 0.9 / np.sqrt(max(W, 2))
    w = scale * rs.standard_normal(P)
    pts = lambda n: np.column_stack([rs.uniform(LB[0], UB[0], n), rs.uniform(LB[1], UB[1], n)])
    X_f, X_u = pts(n_f), pts(n_u)
    u = rs.standard_normal((n_u, n_out))
    eng = pinn_native.Engine(layers, LB, UB, pde=pde_kind, dtype=dtype)
    if pde_kind == "burgers":
        eng.set_collocation(X_f); eng.set_data(X_u, u); eng.set_pde_params(NU)
        ref = pde.burgers_loss_grad(w, layers, LB, UB, X_f, X_u, u, NU)
        sets = {"X_f": X_f, "X_u": X_u, "u": u, "nu": NU}
    elif pde_kind == "burgers_ide":
        w = np.concatenate([w, [0.6, -4.5]])
        eng.set_data(X_u, u)
        ref = pde.burgers_ide_loss_grad(w, layers, LB, UB, X_u, u)
        sets = {"X_u": X_u, "u": u}
    else:
        n_b = int(rs.randint(1, 40))
        tb = rs.uniform(LB[1], UB[1], (n_b, 1))
        X_lb, X_ub = np.hstack([0 * tb + LB[0], tb]), np.hstack([0 * tb + UB[0], tb])
        eng.set_collocation(X_f); eng.set_data(X_u, u); eng.set_boundary(X_lb, X_ub)
        ref = pde.schrodinger_loss_grad(w, layers, LB, UB, X_f, X_lb, X_ub, X_u, u)
        sets = {"X_f": X_f, "X0": X_u, "uv0": u, "X_lb": X_lb, "X_ub": X_ub}
    judged = ge.judge(pde_kind, w, layers, sets, dtype, LB, UB)
    tl, tg = (1e-11, 1e-10) if dtype == "f64" else (2e-5, 5e-5)
    default = eng.kernel_path()
    tried = 0
    for path in (default, 0, 1, 2, 3, 4, 5, 6, 7, 8):
        if tried and path == default:
            continue
        try:
            eng.set_kernel_path(path)
        except pinn_native.PinnNativeError:
            continue
        tried += 1
        eng.set_weights(w)
        loss, grad, _ = eng.loss_grad()
        assert abs(loss - ref[0]) <= tl * max(abs(ref[0]), 1e-3), (path, loss, ref[0])
        assert rel(grad, ref[1]) <= tg, (path, rel(grad, ref[1]))
        assert_entries(grad, judged, path, layers, dtype, record)
    assert tried >= 1
    eng.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_shape_generic_path_over_several_chunks(dtype):
    """more points than one forward/reverse launch pair covers (32768): the partial rows are accumulated across chunks"""
    import pinn_native
    from oracle import pde
    rs = np.random.RandomState(99)
    layers = [2, 24, 24, 24, 1]
    w = 0.4 * rs.standard_normal(sum(a * b + b for a, b in zip(layers[:-1], layers[1:])))
    pts = lambda n: np.column_stack([rs.uniform(LB[0], UB[0], n), rs.uniform(LB[1], UB[1], n)])
    X_f, X_u = pts(70001), pts(77)
    u = rs.standard_normal((77, 1))
    eng = pinn_native.Engine(layers, LB, UB, pde="burgers", dtype=dtype)
    assert eng.kernel_path() == 4
    eng.set_collocation(X_f); eng.set_data(X_u, u); eng.set_pde_params(NU); eng.set_weights(w)
    loss, grad, _ = eng.loss_grad()
    lo, go, ex = pde.burgers_loss_grad(w, layers, LB, UB, X_f, X_u, u, NU)
    tl, tg = (1e-11, 1e-10) if dtype == "f64" else (2e-5, 5e-5)
    assert abs(loss - lo) <= tl * abs(lo) and rel(grad, go) <= tg
    loss2, grad2, _ = eng.loss_grad()
    assert loss2 == loss and np.array_equal(grad, grad2)            # bit-reproducible
    assert rel(eng.residual(), ex["f"]) <= tg * 10                   # MFMA forward in pinn_residual
    eng.close()


def test_shape_generic_path_trains_like_the_reference_implementation():
    """float64, 2x50^3x1: 60 Adam + 40 L-BFGS iterations on the shape-generic MFMA sweeps and on the one-lane-per-point
    kernels from the same start -- the same trajectory (different summation orders: 1e-9 on the losses)"""
    import pinn_native
    from oracle import init
    rs = np.random.RandomState(5)
    layers = [2, 50, 50, 50, 1]
    pts = lambda n: np.column_stack([rs.uniform(LB[0], UB[0], n), rs.uniform(LB[1], UB[1], n)])
    X_f, X_u = pts(3000), pts(100)
    u = -np.sin(np.pi * X_u[:, 0:1])
    out = {}
    for path in (0, 4):
        eng = pinn_native.Engine(layers, LB, UB, pde="burgers", dtype="f64")
        eng.set_collocation(X_f); eng.set_data(X_u, u); eng.set_pde_params(NU); eng.set_weights(init.glorot_flat(layers))
        eng.set_kernel_path(path)
        eng.adam_init(0.005, 0.9, 0.999, 1e-7)
        la = eng.adam_run(60)
        eng.lbfgs_begin(40, 0.8, 50, float(np.finfo(float).eps))
        _, ll, done = eng.lbfgs_run(40)
        out[path] = (la, ll, done, eng.get_weights())
        eng.close()
    assert out[0][2] == out[4][2]
    assert np.max(np.abs(out[0][0] - out[4][0]) / out[0][0]) < 1e-9
    assert len(out[0][1]) == len(out[4][1]) and np.max(np.abs(out[0][1] - out[4][1]) / out[0][1]) < 1e-7
    assert out[4][0][-1] < out[4][0][0]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("pde_kind", ["burgers", "burgers_ide"])
@pytest.mark.parametrize("H", [4, 6, 10])
@pytest.mark.parametrize("n_pts", [700, 40000])
def test_register_stash_kernels_at_other_depths(dtype, pde_kind, H, n_pts, record):
    """hp["layers"] is free-form in the reference (1d-burgers/inf_cont_burgers.py:23-43): 4x20, 6x20 and 10x20 nets run
    on the register-stash kernels too (k_fused20m: depths 4, 6, 8, 10; k_fused20d: 4, 6, 8 -- its AGPR stash of
    (H - 2) x 40 registers ends at 8), one tile per workgroup (700 points) and persistent multi-tile (40000 points),
    against the oracle and bit-reproducibly; 10x20 in float64 stays on the HBM-stash kernel"""
    import pinn_native
    from oracle import pde
    rs = np.random.RandomState(1000 * H + n_pts % 97)
    layers = [2] + [20] * H + [1]
    P = sum(a * b + b for a, b in zip(layers[:-1], layers[1:]))
    w = 0.9 / np.sqrt(20.0) * rs.standard_normal(P)
    pts = lambda n: np.column_stack([rs.uniform(LB[0], UB[0], n), rs.uniform(LB[1], UB[1], n)])
    eng = pinn_native.Engine(layers, LB, UB, pde=pde_kind, dtype=dtype)
    want_path = 2 if dtype == "f32" else (7 if H <= 8 else 1)
    assert eng.kernel_path() == want_path, (eng.kernel_path(), want_path)
    if pde_kind == "burgers":
        X_f, X_u = pts(n_pts), pts(61)
        u = rs.standard_normal((61, 1))
        eng.set_collocation(X_f); eng.set_data(X_u, u); eng.set_pde_params(NU)
        ref = pde.burgers_loss_grad(w, layers, LB, UB, X_f, X_u, u, NU)
        sets = {"X_f": X_f, "X_u": X_u, "u": u, "nu": NU}
    else:
        w = np.concatenate([w, [0.6, -4.5]])
        X_u = pts(n_pts)
        u = rs.standard_normal((n_pts, 1))
        eng.set_data(X_u, u)
        ref = pde.burgers_ide_loss_grad(w, layers, LB, UB, X_u, u)
        sets = {"X_u": X_u, "u": u}
    eng.set_weights(w)
    loss, grad, _ = eng.loss_grad()
    tl, tg = (1e-11, 1e-10) if dtype == "f64" else (2e-5, 5e-5)
    assert abs(loss - ref[0]) <= tl * abs(ref[0]), (loss, ref[0])
    assert rel(grad, ref[1]) <= tg, rel(grad, ref[1])
    assert_entries(np.array(grad, copy=True), ge.judge(pde_kind, w, layers, sets, dtype, LB, UB), want_path, layers, dtype, record)
    loss2, grad2, _ = eng.loss_grad()
    assert loss2 == loss and np.array_equal(grad, grad2)
    eng.adam_init(0.01); la = eng.adam_run(3)                   # the packed weight image follows the optimiser
    eng.lbfgs_begin(4, 0.8, 50, float(np.finfo(float).eps)); _, ll, done = eng.lbfgs_run(4)
    assert np.all(np.isfinite(la)) and np.all(np.isfinite(ll)) and la[1] != la[0]
    lw, gw, _ = eng.loss_grad()
    eng2 = pinn_native.Engine(layers, LB, UB, pde=pde_kind, dtype=dtype)
    eng2.set_kernel_path(1)
    if pde_kind == "burgers":
        eng2.set_collocation(X_f); eng2.set_data(X_u, u); eng2.set_pde_params(NU)
    else:
        eng2.set_data(X_u, u)
    eng2.set_weights(eng.get_weights())
    l1, g1, _ = eng2.loss_grad()
    assert abs(lw - l1) <= tl * 10 * abs(l1) and rel(gw, g1) <= tg * 10
    eng.close(); eng2.close()


@pytest.mark.parametrize("n_corr", [1, 3, 7, 8, 15, 16, 51, 61])
def test_compact_lbfgs_follows_the_reference_order_kernel_at_any_history_size(n_corr):
    """k_lbc_coef_apply (mode 1) against k_lbfgs_step (mode 0, the reference's operation order) for ring sizes M1 = n_corr
    + 1 that are odd and even (the LDS matrices then carry a pad column, which the unguarded recursion reads), smaller and
    larger than one 8-step chunk, with the ring wrapping (60 iterations): same losses to rounding while the iterates are
    close, same log length, float64"""
    import pinn_native
    from oracle import init
    rs = np.random.RandomState(11)
    layers = [2] + [20] * 4 + [1]
    pts = lambda n: np.column_stack([rs.uniform(LB[0], UB[0], n), rs.uniform(LB[1], UB[1], n)])
    X_f, X_u = pts(2000), pts(64)
    u = -np.sin(np.pi * X_u[:, 0:1])
    out = {}
    for mode in (0, 1):
        eng = pinn_native.Engine(layers, LB, UB, pde="burgers", dtype="f64")
        eng.set_collocation(X_f); eng.set_data(X_u, u); eng.set_pde_params(NU); eng.set_weights(init.glorot_flat(layers))
        eng.lbfgs_set_mode(mode)
        eng.lbfgs_begin(60, 0.8, n_corr, float(np.finfo(float).eps))
        it, ll, done = [], [], 0
        while not done:
            a, b, done = eng.lbfgs_run(13)
            it += a.tolist(); ll += b.tolist()
        out[mode] = (np.array(it), np.array(ll), done, eng.get_weights())
        eng.close()
    assert out[0][2] == out[1][2] and np.array_equal(out[0][0], out[1][0])
    dev = np.abs(out[0][1] - out[1][1]) / np.abs(out[0][1])
    assert np.all(np.isfinite(out[1][1])) and np.all(np.isfinite(out[1][3]))
    assert dev[:15].max() < 1e-9, dev[:15].max()
    assert dev.max() < 1e-3, dev.max()
