"""GPU: the post-training half of the path -- `self.model(X_star)` (utils/neuralnetwork.py:151-153),
f_model at caller-supplied points (1d-burgers/ide_cont_burgers.py:169-172) and the scripts' error metric
(1d-burgers/inf_cont_burgers.py:114-116, utils/logger.py:56-60) -- on the MFMA forward sweeps of
csrc/kernels_predict20.h and the device-side reduction pinn_error_l2, through the C ABI, against the oracle / numpy."""
import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu

NU = 0.01 / np.pi
LB, UB = np.array([-1.0, 0.0]), np.array([1.0, 0.99])


def _net(H, seed, ide=False):
    rs = np.random.RandomState(seed)
    layers = [2] + [20] * H + [1]
    P = sum(a * b + b for a, b in zip(layers[:-1], layers[1:]))
    w = 0.9 / np.sqrt(20.0) * rs.standard_normal(P)
    if ide:
        w = np.concatenate([w, [0.7, -4.0]])
    return layers, w, rs


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("H", [1, 2, 3, 8, 11])
def test_width20_forward_sweeps_any_depth(dtype, H):
    """k_fwd20d / k_fwd20f, value channel and Taylor channels, depths 1..11, ragged point counts incl. > one pass of
    the persistent grid (f32: 8 x 256 workgroups of 64 points = 131072)"""
    import pinn_native
    from oracle import mlp, pde
    layers, w, rs = _net(H, 100 + H)
    eng = pinn_native.Engine(layers, LB, UB, pde="burgers", dtype=dtype)
    eng.set_pde_params(NU)
    eng.set_weights(w)
    tol_u, tol_f = (1e-13, 1e-11) if dtype == "f64" else (3e-6, 1e-4)
    for n in (1, 65, 1000, 140001 if H == 8 else 777):
        X = np.column_stack([rs.uniform(LB[0], UB[0], n), rs.uniform(LB[1], UB[1], n)])
        u = eng.predict(X)
        assert u.shape == (n, 1)
        ref = mlp.forward_value(mlp.unpack(w, layers), X, LB, UB)
        assert np.max(np.abs(u - ref)) <= tol_u * max(1.0, np.max(np.abs(ref))), (n, np.max(np.abs(u - ref)))
        if n <= 1000:
            Xu = X[:1]
            _, _, ex = pde.burgers_loss_grad(w, layers, LB, UB, X, Xu, np.zeros((1, 1)), NU)
            f = eng.residual_at(X)
            scale = max(1.0, np.max(np.abs(ex["f"])))
            assert np.max(np.abs(f - ex["f"])) <= tol_f * scale, (n, np.max(np.abs(f - ex["f"])) / scale)
            eng.set_collocation(X); eng.set_data(Xu, np.zeros((1, 1)))
            assert np.max(np.abs(eng.residual() - ex["f"])) <= tol_f * scale
    eng.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_identification_residual_at_uses_the_lambdas(dtype):
    import pinn_native
    from oracle import pde
    layers, w, rs = _net(8, 7, ide=True)
    X = np.column_stack([rs.uniform(LB[0], UB[0], 300), rs.uniform(LB[1], UB[1], 300)])
    u = rs.standard_normal((300, 1))
    eng = pinn_native.Engine(layers, LB, UB, pde="burgers_ide", dtype=dtype)
    eng.set_data(X, u); eng.set_weights(w)
    _, _, ex = pde.burgers_ide_loss_grad(w, layers, LB, UB, X, u)
    tol = 1e-11 if dtype == "f64" else 1e-4
    scale = max(1.0, np.max(np.abs(ex["f"])))
    assert np.max(np.abs(eng.residual_at(X) - ex["f"])) <= tol * scale
    assert np.max(np.abs(eng.residual() - ex["f"])) <= tol * scale
    eng.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_error_l2_on_the_device_equals_numpy(burgers_sets, dtype, record):
    """pinn_error_l2 against np.linalg.norm on the predicted field (the value the reference's error() returns):
    1e-14 relative in float64 -- both sides are float64 sums of the same 25600 float64 terms -- repeat calls
    (cached grid) bit-identical, and a changed reference field or grid is noticed"""
    import pinn_native
    g = np.load(golden("burgers_eval.npz"))
    r = burgers_sets(100, 10000)
    X_star, u_star, lb, ub = r[5], r[6], r[11], r[10]
    eng = pinn_native.Engine([2] + [20] * 8 + [1], lb, ub, pde="burgers", dtype=dtype)
    eng.set_weights(g["w0"])
    up = eng.predict(X_star)
    want = float(np.linalg.norm(u_star - up, 2) / np.linalg.norm(u_star, 2))
    got = eng.error_l2(X_star, u_star)
    record(dtype=dtype, err_device=got, err_numpy=want, rel_dev=abs(got - want) / want)
    assert abs(got - want) <= 1e-14 * want, (got, want)
    assert abs(got - float(g["err0"])) < (1e-11 if dtype == "f64" else 2e-5)      # the reference's own error at w0
    assert eng.error_l2(X_star, u_star) == got
    u2 = u_star + 0.125
    want2 = float(np.linalg.norm(u2 - up, 2) / np.linalg.norm(u2, 2))
    assert abs(eng.error_l2(X_star, u2) - want2) <= 1e-14 * want2
    n = 1001                                                                      # another grid, ragged
    want3 = float(np.linalg.norm(u_star[:n] - up[:n], 2) / np.linalg.norm(u_star[:n], 2))
    assert abs(eng.error_l2(X_star[:n], u_star[:n]) - want3) <= 1e-14 * want3
    eng.set_weights(g["w0"] * 1.001)                                              # new weights, same cached grid
    up4 = eng.predict(X_star[:n])
    want4 = float(np.linalg.norm(u_star[:n] - up4, 2) / np.linalg.norm(u_star[:n], 2))
    assert abs(eng.error_l2(X_star[:n], u_star[:n]) - want4) <= 1e-14 * want4 and want4 != want3
    eng.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_error_l2_modulus_kind_schrodinger(schrodinger_sets, dtype):
    """|h| = sqrt(u^2 + v^2) against h_star (1dcomplex-schrodinger/inf_cont_schrodinger.py:155-158), two-output net on
    the shape-generic forward sweep + k_pick_values"""
    import json
    import pinn_native
    g = np.load(golden("schrodinger_eval_small.npz"))
    hp = json.loads(str(g["hp"]))
    r = schrodinger_sets(50, 50, 1024)
    X_star, h_star, ub, lb = r[7], r[10], r[12], r[13]
    eng = pinn_native.Engine(hp["layers"], lb, ub, pde="schrodinger", dtype=dtype)
    eng.set_weights(g["w0"])
    uv = eng.predict(X_star)
    h = np.sqrt(uv[:, 0:1] ** 2 + uv[:, 1:2] ** 2)
    want = float(np.linalg.norm(h_star - h, 2) / np.linalg.norm(h_star, 2))
    got = eng.error_l2(X_star, h_star, modulus=True)
    assert abs(got - want) <= 1e-13 * want, (got, want)
    uv_ref = np.concatenate([r[8], r[9]], axis=1)                                  # element-wise kind over [n][2]
    want0 = float(np.linalg.norm(uv_ref - uv) / np.linalg.norm(uv_ref))
    assert abs(eng.error_l2(X_star, uv_ref) - want0) <= 1e-13 * want0
    eng.close()


# ---- forward-only evaluation over shapes: pinn_predict, pinn_residual_at, pinn_residual, pinn_error_l2 ----------------
# (pde, dtype, W, H, n, seed); the comment names the forward kernel (engine.hip forward_chunk).  Width 20 with one output
# (k_fwd20d / k_fwd20f) is test_width20_forward_sweeps_any_depth above.
_FWD = [
    # k_forward<real, JT> (one lane per point; JT = 10 float64, 20 float32): widths below 24 other than Burgers 20
    *[("burgers", dt, W, 1 + i % 3, (65, 777, 1000, 63, 2049, 3001, 1)[i], 10 + i)
      for i, W in enumerate((1, 7, 10, 11, 19, 21, 23)) for dt in ("f64", "f32")],
    ("schrodinger", "f64", 20, 3, 1000, 20),          # k_forward: two outputs, so not k_fwd20d
    ("schrodinger", "f32", 20, 2, 777, 21),           # k_forward
    ("schrodinger", "f64", 23, 2, 513, 22),           # k_forward
    ("schrodinger", "f32", 23, 3, 1000, 23),          # k_forward
    ("burgers_ide", "f64", 13, 3, 800, 24),           # k_forward, lambdas from the weight image
    ("burgers_ide", "f32", 13, 2, 999, 25),           # k_forward
    # k_t16_fwd, NT = 4
    ("burgers", "f64", 24, 3, 1000, 30),              # k_t16_fwd NT 4, weights from L2
    ("burgers_ide", "f64", 40, 2, 1500, 31),          # k_t16_fwd NT 4
    ("schrodinger", "f64", 64, 2, 777, 32),           # k_t16_fwd NT 4
    ("burgers", "f32", 40, 2, 40000, 33),             # k_t16_fwd NT 4: 32768-point chunk with LDS weights, 7232 without
    ("schrodinger", "f32", 64, 3, 600, 34),           # k_t16_fwd NT 4, few groups: weights from L2
    # k_t16_fwd, NT = 8 (float64 and float32: eight waves, weights from L2)
    ("burgers", "f64", 65, 2, 1000, 40),              # k_t16_fwd NT 8
    ("burgers", "f32", 65, 3, 1000, 41),              # k_t16_fwd NT 8
    ("schrodinger", "f64", 100, 2, 1200, 42),         # k_t16_fwd NT 8
    ("schrodinger", "f32", 100, 4, 1000, 43),         # k_t16_fwd NT 8
    ("burgers_ide", "f64", 128, 2, 800, 44),          # k_t16_fwd NT 8
    ("burgers_ide", "f32", 128, 3, 800, 45),          # k_t16_fwd NT 8
    # several 32768-point chunks per call
    ("burgers", "f64", 24, 2, 32769, 50),             # k_t16_fwd NT 4, chunks of 32768 + 64
    ("burgers", "f32", 24, 2, 70001, 51),             # k_t16_fwd NT 4, 2 LDS-weight chunks + one of 4480 points without
    ("schrodinger", "f64", 100, 2, 70001, 52),        # k_t16_fwd NT 8, three chunks
    ("burgers", "f32", 100, 2, 32769, 53),            # k_t16_fwd NT 8, two chunks
]
_BOX = {"burgers": (LB, UB), "burgers_ide": (LB, UB),
        "schrodinger": (np.array([-5.0, 0.0]), np.array([5.0, np.pi / 2]))}


def _fwd_net(pde_kind, W, H, rs):
    layers = [2] + [W] * H + [2 if pde_kind == "schrodinger" else 1]
    w = 0.9 / np.sqrt(W) * rs.standard_normal(sum(a * b + b for a, b in zip(layers[:-1], layers[1:])))
    if pde_kind == "burgers_ide":
        w = np.concatenate([w, [rs.uniform(0.5, 1.5), rs.uniform(-7.0, -4.0)]])
    return layers, w


def _fwd_oracle(pde_kind, layers, w, X, lb, ub, nu):
    """(values [n, n_out], residual [n, n_out]) of oracle/pde.py"""
    from oracle import mlp, pde
    if pde_kind == "schrodinger":
        f_u, f_v, (h, _, _, _), _ = pde.schrodinger_residual(mlp.unpack(w, layers), X, lb, ub)
        return h, np.concatenate([f_u, f_v], axis=1)
    if pde_kind == "burgers_ide":
        f, (u, _, _, _), _ = pde.burgers_residual(mlp.unpack(w[:-2], layers), X, lb, ub, w[-2], np.exp(w[-1]))
    else:
        f, (u, _, _, _), _ = pde.burgers_residual(mlp.unpack(w, layers), X, lb, ub, 1.0, nu)
    return u, f


def _points(rs, n, lb, ub):
    return np.column_stack([rs.uniform(lb[0], ub[0], n), rs.uniform(lb[1], ub[1], n)])


@pytest.mark.parametrize("pde_kind,dtype,W,H,n,seed", _FWD,
                         ids=["%s-%s-W%d-H%d-n%d" % c[:5] for c in _FWD])
def test_forward_only_evaluation_sweep(pde_kind, dtype, W, H, n, seed, record):
    """predict / residual_at / residual / error_l2 and the evaluation-point cache against oracle/pde.py and numpy, on
    every forward kernel the caller-sized dispatch can pick.  Bounds: values f64 1e-12, f32 5e-6; residuals f64 1e-10,
    f32 2e-4, both relative to max(1, max|ref|) (test_gpu_parity.py); error_l2 1e-14 relative against numpy on the
    device's own prediction (test_error_l2_on_the_device_equals_numpy), 1e-13 for the modulus kind
    (test_error_l2_modulus_kind_schrodinger)."""
    import pinn_native
    from oracle import mlp
    rs = np.random.RandomState(seed)
    lb, ub = _BOX[pde_kind]
    layers, w = _fwd_net(pde_kind, W, H, rs)
    nu = rs.uniform(0.001, 0.1)                       # not the default: a viscosity left in place would show
    tol_u, tol_f = (1e-12, 1e-10) if dtype == "f64" else (5e-6, 2e-4)
    tag = "%s-%s-W%d-H%d-n%d" % (pde_kind, dtype, W, H, n)

    def dev(a, ref):
        return np.max(np.abs(a - ref)) / max(1.0, np.max(np.abs(ref)))

    eng = pinn_native.Engine(layers, lb, ub, pde=pde_kind, dtype=dtype)
    try:
        if pde_kind == "burgers":
            eng.set_pde_params(nu)
        eng.set_weights(w)
        X = _points(rs, n, lb, ub)
        u_ref, f_ref = _fwd_oracle(pde_kind, layers, w, X, lb, ub, nu)
        # 1. values, 2. residuals at the caller's points
        u = eng.predict(X)
        f = eng.residual_at(X)
        d_u, d_f = dev(u, u_ref), dev(f, f_ref)
        # 3. the same points as the stored set, behind a data set (and boundary pairs): the residual starts at an offset
        if pde_kind == "burgers_ide":
            eng.set_data(X, rs.standard_normal((n, 1)))
        else:
            if pde_kind == "schrodinger":
                tb = rs.uniform(lb[1], ub[1], (5, 1))
                eng.set_boundary(np.hstack([0 * tb + lb[0], tb]), np.hstack([0 * tb + ub[0], tb]))
            no = layers[-1]
            eng.set_data(_points(rs, 9, lb, ub), rs.standard_normal((9, no)))
            eng.set_collocation(X)
        d_fs = dev(eng.residual(), f_ref)
        record(case=tag, value=d_u, residual=d_f, residual_stored=d_fs)
        assert u.shape == u_ref.shape and f.shape == f_ref.shape
        assert d_u <= tol_u and d_f <= tol_f and d_fs <= tol_f, (d_u, d_f, d_fs)
        # 4. error_l2: element-wise against numpy on the device's own prediction, and against the oracle's prediction
        #    within the triangle inequality; the modulus kind on one- and two-output nets
        ref = u_ref + 0.1 * rs.standard_normal(u_ref.shape)
        e = eng.error_l2(X, ref)
        e_np = np.linalg.norm(ref - u) / np.linalg.norm(ref)
        e_or = np.linalg.norm(ref - u_ref) / np.linalg.norm(ref)
        slack = np.linalg.norm(u - u_ref) / np.linalg.norm(ref)
        href = np.sqrt(np.sum(u_ref ** 2, axis=1)) + 0.1 * np.abs(rs.standard_normal(n))
        em = eng.error_l2(X, href, modulus=True)
        em_np = np.linalg.norm(href - np.sqrt(np.sum(u ** 2, axis=1))) / np.linalg.norm(href)
        record(case=tag, err_l2=abs(e - e_np) / e_np, err_l2_oracle=abs(e - e_or), err_l2_slack=slack,
               err_l2_modulus=abs(em - em_np) / em_np)
        assert abs(e - e_np) <= 1e-14 * e_np, (e, e_np)
        assert abs(e - e_or) <= slack + 1e-14 * e_or, (e, e_or, slack)
        assert abs(em - em_np) <= 1e-13 * em_np, (em, em_np)
        # 5. the evaluation-point cache: same points after new weights, same count with new contents, fewer points
        w2 = w * (1.0 + 0.05 * rs.standard_normal(w.size))
        eng.set_weights(w2)
        p2 = mlp.unpack(w2[:-2] if pde_kind == "burgers_ide" else w2, layers)
        u2 = eng.predict(X)
        d_c1 = dev(u2, mlp.forward_value(p2, X, lb, ub))
        e2 = eng.error_l2(X, ref)
        e2_np = np.linalg.norm(ref - u2) / np.linalg.norm(ref)
        X2 = _points(rs, n, lb, ub)
        d_c2 = dev(eng.predict(X2), mlp.forward_value(p2, X2, lb, ub))
        X3 = X2[:max(1, n // 3)]
        u3_ref, f3_ref = _fwd_oracle(pde_kind, layers, w2, X3, lb, ub, nu)
        d_c3, d_c3f = dev(eng.predict(X3), u3_ref), dev(eng.residual_at(X3), f3_ref)
        record(case=tag, value_new_weights=d_c1, value_new_points=d_c2, value_fewer_points=d_c3,
               residual_fewer_points=d_c3f)
        assert d_c1 <= tol_u and not np.array_equal(u2, u), d_c1
        assert abs(e2 - e2_np) <= 1e-14 * e2_np and e2 != e, (e2, e2_np)
        assert d_c2 <= tol_u and d_c3 <= tol_u and d_c3f <= tol_f, (d_c2, d_c3, d_c3f)
    finally:
        eng.close()


@pytest.mark.parametrize("pde_kind,dtype,W,H,sizes", [
    ("burgers", "f64", 24, 2, (2047, 2048, 2049, 4096, 100003)),        # k_t16_fwd, one output
    ("burgers", "f32", 7, 2, (2047, 2048, 2049, 4096, 100003)),         # k_forward, one output
    ("schrodinger", "f64", 23, 2, (1023, 1024, 1025, 2047, 2048, 2049, 50003)),   # k_forward, two outputs
    ("schrodinger", "f32", 100, 2, (1023, 1024, 1025, 2047, 2048, 2049, 50003)),  # k_t16_fwd NT 8, two outputs
])
def test_error_l2_at_reduction_block_edges(pde_kind, dtype, W, H, sizes, record):
    """k_err_partial sums blocks of 2048 elements: counts that end just before, on and just past a block, two blocks,
    and over 100 000 elements.  The element-wise kind reduces n n_out elements, the modulus kind n.  A two-output net
    has no odd element-wise count, so it takes 2046 / 2048 / 2050 (n = 1023..1025) there and n = 2047..2049 for the
    modulus kind.  Bounds as in test_forward_only_evaluation_sweep."""
    import pinn_native
    rs = np.random.RandomState(W + len(sizes))
    lb, ub = _BOX[pde_kind]
    layers, w = _fwd_net(pde_kind, W, H, rs)
    eng = pinn_native.Engine(layers, lb, ub, pde=pde_kind, dtype=dtype)
    try:
        eng.set_weights(w)
        for n in sizes:
            X = _points(rs, n, lb, ub)
            u = eng.predict(X)
            ref = u + 0.1 * rs.standard_normal(u.shape)
            e, e_np = eng.error_l2(X, ref), np.linalg.norm(ref - u) / np.linalg.norm(ref)
            href = np.sqrt(np.sum(u ** 2, axis=1)) + 0.1 * rs.standard_normal(n)
            em = eng.error_l2(X, href, modulus=True)
            em_np = np.linalg.norm(href - np.sqrt(np.sum(u ** 2, axis=1))) / np.linalg.norm(href)
            record(case="%s-%s-W%d" % (pde_kind, dtype, W), n=n, err_l2=abs(e - e_np) / e_np,
                   err_l2_modulus=abs(em - em_np) / em_np)
            assert abs(e - e_np) <= 1e-14 * e_np, (n, e, e_np)
            assert abs(em - em_np) <= 1e-13 * em_np, (n, em, em_np)
    finally:
        eng.close()


def test_status_records_the_first_nonfinite_evaluation(burgers_sets):
    """SURVEY 5 failure detection: the reference lets a NaN loss propagate (custom_lbfgs.py:154); the engine does the
    same and additionally records WHEN it happened"""
    import pinn_native
    g = np.load(golden("burgers_eval_small.npz"))
    r = burgers_sets(64, 2048)
    X_u, u, X_f, ub, lb = r[7], r[8], r[9], r[10], r[11]
    for dtype in ("f64", "f32"):
        eng = pinn_native.Engine([2] + [20] * 8 + [1], lb, ub, pde="burgers", dtype=dtype)
        eng.set_collocation(X_f); eng.set_data(X_u, u); eng.set_pde_params(NU)
        eng.set_weights(g["w0"])
        eng.loss_grad(); eng.loss_grad()
        assert eng.status() == (2, 0)
        w = g["w0"].copy(); w[100] = np.nan
        eng.set_weights(w)
        loss, _, _ = eng.loss_grad()
        assert not np.isfinite(loss)
        eng.set_weights(g["w0"])
        eng.adam_init(0.03); eng.adam_run(2)
        assert eng.status() == (5, 3)                       # sticky: the FIRST bad evaluation
        eng.close()
