"""GPU: the adr2 kind (PINN_PDE_ADR2: b u_t + (a0 + a1 u) u_x - nu (u_xx + kappa u_tt) + r1 u + r2 u^2 + r3 u^3 = s, three-term
wall points) against its numpy restatement tests/helpers/adr2_ref.py (pinned on the CPU by tests/test_adr2_host.py), on the
kernel paths the kind has: the generic path 0 (float64 and float32, any shape) and the float64 width-20 kernel k_adr2_20d
(path 7: 2-20-...-20-1 with 4, 6 or 8 hidden layers).

Tolerances are the adr family's (tests/test_gpu_adr_source.py).  A float32 bound stands where the helper's own
float32-arithmetic error on that case is at most a quarter of it; otherwise the bound is 4 x that error
(tests/test_gpu_adrd_disc.py's rule)."""
import functools
import os
import sys

import numpy as np
import pytest

from conftest import PKG  # noqa: F401

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import adr2_ref  # noqa: E402
import adr_src_ref  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = {"f64": dict(loss=1e-12, grad=1e-11, res=1e-10), "f32": dict(loss=1e-5, grad=2e-5, res=2e-4)}
LB, UB = np.array([-1.0, 0.0]), np.array([1.0, 1.0])
CONFIGS = [("f64", 0), ("f64", 7), ("f32", 0)]        # (dtype, kernel path)
GENERIC = [("f64", 0), ("f32", 0)]                    # shapes path 7 does not take
NAMES = ["adr", "wave_c2", "wave_c02", "telegraph", "klein_gordon", "helmholtz", "cdr", "all"]


def rel(a, b):
    return np.max(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300)


def layers_of(depth, width=20):
    return [2] + [width] * depth + [1]


def source_of(X):
    return np.sin(3.0 * X[:, 0]) * np.exp(-X[:, 1]) + 0.5


@functools.lru_cache(maxsize=None)
def weights(layers, seed=7, saturate=False):
    """a glorot draw plus 0.05 * standard_normal: biases non-zero.  saturate: the first layer scaled until 10 % of its
    activations at 4096 uniform points of the default box exceed 0.999"""
    from oracle import init
    layers = list(layers)
    w = init.glorot_flat(layers)
    w = w + 0.05 * np.random.RandomState(seed).standard_normal(w.size)
    if saturate:
        n0 = 2 * layers[1] + layers[1]
        X = LB + (UB - LB) * np.random.RandomState(1).uniform(size=(4096, 2))
        H = 2.0 * (X - LB) / (UB - LB) - 1.0
        W0, b0 = w[:2 * layers[1]].reshape(2, -1), w[2 * layers[1]:n0]
        scale = 1.0
        while np.mean(np.abs(np.tanh(scale * (H @ W0 + b0))) > 0.999) < 0.10:
            scale *= 1.25
        w[:n0] *= scale
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def point_sets(N_f, n_0=512, n_b=50, n_w=17, seed=3, box=None):
    """collocation points with their source, initial data, n_b wall pairs, n_w three-term wall points: x alternating between
    the walls, alpha, beta, gamma in U(-1.5, 1.5) with every fifth alpha, every seventh beta and every third gamma 0 (never all
    three), g in U(-1, 1)"""
    lb, ub = (LB, UB) if box is None else (np.array(box[0]), np.array(box[1]))
    rs = np.random.RandomState(seed)
    X_f = lb + (ub - lb) * rs.uniform(size=(N_f, 2))
    x0 = lb[0] + (ub[0] - lb[0]) * rs.uniform(size=n_0)
    X_u = np.column_stack([x0, np.full(n_0, lb[1])])
    u = (x0 * x0 * np.cos(np.pi * x0)).reshape(-1, 1)
    tb = lb[1] + (ub[1] - lb[1]) * rs.uniform(size=n_b)
    X_lo, X_hi = np.column_stack([np.full(n_b, lb[0]), tb]), np.column_stack([np.full(n_b, ub[0]), tb])
    j = np.arange(n_w)
    X_w = np.column_stack([np.where(j % 2, ub[0], lb[0]), lb[1] + (ub[1] - lb[1]) * rs.uniform(size=n_w)])
    alpha, beta, gamma = (rs.uniform(-1.5, 1.5, n_w) for _ in range(3))
    g = rs.uniform(-1, 1, n_w)
    alpha[j % 5 == 4] = 0.0
    beta[j % 7 == 6] = 0.0
    gamma[(j % 3 == 2) & ((alpha != 0.0) | (beta != 0.0))] = 0.0
    assert not np.any((alpha == 0.0) & (beta == 0.0) & (gamma == 0.0))
    s = source_of(X_f)
    out = dict(lb=lb, ub=ub, X_f=X_f, X_u=X_u if n_0 else None, u=u if n_0 else None, X_lo=X_lo if n_b else None,
               X_hi=X_hi if n_b else None, s=s, wall=(X_w, alpha, beta, gamma, g) if n_w else None)
    for a in (X_f, X_u, u, X_lo, X_hi, s, X_w, alpha, beta, gamma, g):
        a.setflags(write=False)
    return out


def helper(w, layers, ps, coeffs, s="set", wall="set", dtype=np.float64):
    s = ps["s"] if isinstance(s, str) else s
    wall = ps["wall"] if isinstance(wall, str) else wall
    return adr2_ref.adr2_loss_grad(w, layers, ps["lb"], ps["ub"], ps["X_f"], ps["X_u"], ps["u"], ps["X_lo"], ps["X_hi"], coeffs,
                                   s, *(wall or ()), dtype=dtype)


@functools.lru_cache(maxsize=None)
def reference(layers, name, key, saturate=False, dtype="f64"):
    """the restatement on a cell: computed once, shared, never written to"""
    return helper(weights(layers, saturate=saturate), list(layers), point_sets(*key), adr2_ref.COEFF_SETS[name],
                  dtype=np.float64 if dtype == "f64" else np.float32)


def make(layers, dtype, path, coeffs, ps, s="set", wall="set", pde="adr2"):
    from pinn_native import Engine
    eng = Engine(list(layers), ps["lb"], ps["ub"], pde=pde, dtype=dtype)
    eng.set_pde_params(*coeffs)
    eng.set_collocation(ps["X_f"])
    if ps["X_u"] is not None:
        eng.set_data(ps["X_u"], ps["u"])
    if ps["X_lo"] is not None:
        eng.set_boundary(ps["X_lo"], ps["X_hi"])
    wall = ps["wall"] if isinstance(wall, str) else wall
    if wall is not None:
        if pde == "adr2":
            eng.set_robin3(*wall)
        else:
            eng.set_robin(wall[0], wall[1], wall[2], wall[4])
    s = ps["s"] if isinstance(s, str) else s
    if s is not None:
        eng.set_source(s)
    eng.set_kernel_path(path)          # no skip: the path must exist for every cell
    assert eng.kernel_path() == path
    return eng


def same_bits(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def bounds(dtype, got64, got32):
    """the family's bounds; in float32 each stands where the helper's own float32 error is at most a quarter of it, and is
    4 x that error otherwise"""
    tol = dict(TOL[dtype])
    if dtype == "f32":
        (l64, g64, e64), (l32, g32, e32) = got64, got32
        own = dict(loss=abs(float(l32) - l64) / l64, grad=rel(g32, g64), res=rel(e32["f"], e64["f"]))
        for k, v in own.items():
            if v > tol[k] / 4.0:
                tol[k] = 4.0 * v
    return tol


def check_cell(record, tag, layers, dtype, path, name, key, saturate=False):
    layers = tuple(layers)
    ps = point_sets(*key)
    eng = make(layers, dtype, path, adr2_ref.COEFF_SETS[name], ps)
    eng.set_weights(weights(layers, saturate=saturate))
    loss, grad, terms = eng.loss_grad()
    f = eng.residual()
    r = eng.robin_residual()
    eng.close()
    ref64 = reference(layers, name, key, saturate)
    tol = bounds(dtype, ref64, reference(layers, name, key, saturate, "f32") if dtype == "f32" else None)
    lo, go, ex = ref64
    n_w = 0 if ps["wall"] is None else len(ps["wall"][0])
    dev = dict(loss=abs(loss - lo) / lo, grad=rel(grad, go), res=rel(f, ex["f"]),
               t_f=abs(terms[0] - ex["mse_f"]) / lo, t_u=abs(terms[1] - ex["mse_u"]) / lo,
               t_b=abs(terms[2] - (ex["mse_b"] + ex["mse_w"])) / lo)
    if n_w:
        dev["rob"] = rel(r, ex["r"])
    print("adr2 %s %s path %d: %s | bounds %s" % (tag, dtype, path, " ".join("%s %.2e" % kv for kv in sorted(dev.items())),
                                                  " ".join("%s %.1e" % kv for kv in sorted(tol.items()))))
    record(tag=tag, dtype=dtype, path=path, **dev)
    assert f.shape == (len(ps["X_f"]), 1) and r.shape == (n_w,)
    assert dev["loss"] < tol["loss"]
    assert dev["grad"] < tol["grad"]
    assert dev["res"] < tol["res"]
    assert dev.get("rob", 0.0) < tol["res"]
    assert max(dev["t_f"], dev["t_u"], dev["t_b"]) < tol["loss"] * 10


# ---- 1. the coefficient vectors ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,path", CONFIGS)
@pytest.mark.parametrize("name", NAMES)
def test_coefficient_vectors(record, name, dtype, path):
    """N_f = 2048, 512 data points, 50 pairs, 17 wall points, a source; depth 4"""
    check_cell(record, "a:" + name, layers_of(4), dtype, path, name, (2048, 512, 50, 17))


@pytest.mark.parametrize("dtype,path", CONFIGS)
def test_kappa_reaches_the_device(dtype, path):
    """two device evaluations, the wave vector and the same with kappa = 0: the losses differ by more than 1 %, three orders
    above the float32 bound, and by what the helper says"""
    layers, ps, co = tuple(layers_of(4)), point_sets(2048, 512, 50, 17), list(adr2_ref.COEFF_SETS["wave_c2"])
    eng = make(layers, dtype, path, co, ps)
    eng.set_weights(weights(layers))
    l1 = eng.loss_grad()[0]
    co[7] = 0.0
    eng.set_pde_params(*co)
    l0 = eng.loss_grad()[0]
    eng.close()
    want = reference(layers, "wave_c2", (2048, 512, 50, 17))[0] - helper(weights(layers), list(layers), ps, co)[0]
    assert abs(l1 - l0) > 1e-2 * l0 and abs((l1 - l0) - want) < 1e-3 * abs(want)


def test_default_path_is_the_fast_kernel_for_float64_width_20():
    from pinn_native import Engine
    for depth in (4, 6, 8):
        eng = Engine(layers_of(depth), LB, UB, pde="adr2", dtype="f64")
        assert eng.kernel_path() == 7
        eng.close()
    for layers, dtype in ((layers_of(8), "f32"), (layers_of(5), "f64"), (layers_of(3, 100), "f64")):
        eng = Engine(layers, LB, UB, pde="adr2", dtype=dtype)
        assert eng.kernel_path() == 0
        eng.close()


# ---- 2. shapes: depths, more than one chunk, the generic widths ---------------------------------------------------------------------
@pytest.mark.parametrize("dtype,path", CONFIGS)
@pytest.mark.parametrize("N_f", [2048, 40000])
@pytest.mark.parametrize("depth", [4, 6, 8])
def test_depths_and_tile_plans(record, depth, N_f, dtype, path):
    """path 7: 2048 is one tile per workgroup, 40000 (627 tiles > 256 compute units) the tile loop; path 0: 40000 points are two
    chunks (the second one's rows are added to the first's)"""
    check_cell(record, "b:d%d:Nf%d" % (depth, N_f), layers_of(depth), dtype, path, "all", (N_f, 512, 50, 17))


@pytest.mark.parametrize("dtype,path", GENERIC)
@pytest.mark.parametrize("layers", [[2, 7, 7, 1], [2, 5, 5, 5, 1], [2, 33, 1], [2, 100, 100, 1]], ids=lambda v: "x".join(map(str, v)))
def test_generic_shapes(record, layers, dtype, path):
    """widths below, at no multiple of and above the kernels' register tiles (JT = 10 / 20, KT = 5 / 10), one hidden layer, and
    width 100 (where every other forward sweep of the engine would take the MFMA kernels, which carry no kappa)"""
    check_cell(record, "c:" + "x".join(map(str, layers)), layers, dtype, path, "all", (300, 40, 5, 7))


def test_unequal_hidden_widths_are_refused_as_for_every_kind():
    """[2, 7, 5, 1]: the engine holds one hidden width (every kind: the flat weight layout assumes it), so create refuses"""
    import pinn_native
    with pytest.raises(pinn_native.PinnNativeError, match="all hidden widths must be equal"):
        pinn_native.Engine([2, 7, 5, 1], LB, UB, pde="adr2", dtype="f64")


@pytest.mark.parametrize("dtype,path", CONFIGS)
@pytest.mark.parametrize("N_f,n_b,n_w,n_0", [(1, 0, 0, 0), (63, 1, 1, 512), (65, 50, 17, 0), (63, 0, 17, 512), (65, 1, 0, 512),
                                             (1, 50, 1, 0)])
def test_index_alignment(record, N_f, n_b, n_w, n_0, dtype, path):
    """every class empty, of one point and of a length that leaves the next class at an odd index"""
    check_cell(record, "d:Nf%d:nb%d:nw%d:n0%d" % (N_f, n_b, n_w, n_0), layers_of(4), dtype, path, "all", (N_f, n_0, n_b, n_w))


@pytest.mark.parametrize("dtype,path", CONFIGS)
def test_other_box(record, dtype, path):
    check_cell(record, "e:box", layers_of(4), dtype, path, "all", (2048, 512, 50, 17, 3, ((0.5, -2.0), (3.0, -1.0))))


@pytest.mark.parametrize("dtype,path", CONFIGS)
def test_saturated_first_layer(record, dtype, path):
    w = weights(tuple(layers_of(4)), saturate=True)
    X = point_sets(2048, 512, 50, 17)["X_f"]
    a = np.tanh((2.0 * (X - LB) / (UB - LB) - 1.0) @ w[:40].reshape(2, 20) + w[40:60])
    assert np.mean(np.abs(a) > 0.999) >= 0.08
    check_cell(record, "f:saturated", layers_of(4), dtype, path, "wave_c2", (2048, 512, 50, 17), saturate=True)


# ---- 3. the adr kind embedded: bits --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", [0, 7])
@pytest.mark.parametrize("N_f", [2048, 40000])
def test_degenerate_vector_equals_an_adr_engine(N_f, path):
    """kappa = 0, b = 1, gamma = 0 against pde "adr" with the same source and Robin points, float64, paths 0 and 7: loss, terms
    and gradient by np.array_equal"""
    layers = tuple(layers_of(4))
    ps = point_sets(N_f, 512, 50, 17)
    X_w, alpha, beta, gamma, g = ps["wall"]
    keep = (alpha != 0.0) | (beta != 0.0)               # (a point with alpha = beta = 0 is no Robin point)
    wall = (X_w[keep], alpha[keep], beta[keep], np.zeros(int(keep.sum())), g[keep])
    co = adr2_ref.COEFF_SETS["adr"]
    two = make(layers, "f64", path, co, ps, wall=wall)
    one = make(layers, "f64", path, co[:6], ps, wall=wall, pde="adr")
    for e in (one, two):
        e.set_weights(weights(layers))
    a, b = two.loss_grad(), one.loss_grad()
    assert a[0] == b[0] and np.array_equal(a[2], b[2]) and np.array_equal(a[1], b[1])
    # (the forward-only residuals agree to rounding, not in bits: at width 20 the adr kind takes them from the MFMA forward kernel)
    assert rel(two.residual(), one.residual()) < 1e-12 and rel(two.robin_residual(), one.robin_residual()) < 1e-12
    # pinn_set_robin on this kind means gamma = 0
    two.set_robin(wall[0], wall[1], wall[2], wall[4])
    assert same_bits(two.loss_grad(), a)
    one.close()
    two.close()


# ---- 4. toggling -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,path", CONFIGS)
def test_removing_the_source_and_the_walls_returns_the_plain_values(dtype, path):
    layers, co = tuple(layers_of(4)), adr2_ref.COEFF_SETS["all"]
    ps = point_sets(2048, 512, 50, 17)
    never = make(layers, dtype, path, co, ps, s=None, wall=None)
    eng = make(layers, dtype, path, co, ps)
    for e in (never, eng):
        e.set_weights(weights(layers))
    ref, f_ref = never.loss_grad(), never.residual()
    full = eng.loss_grad()
    assert same_bits(full, eng.loss_grad()) and full[0] != ref[0]
    eng.set_source(None)
    eng.set_robin3(np.zeros((0, 2)), 0.0, 0.0, 1.0, 0.0)
    assert not eng.has_source and eng.n_w == 0
    assert same_bits(eng.loss_grad(), ref) and np.array_equal(eng.residual(), f_ref)
    assert np.array_equal(eng.residual_at(ps["X_f"]), never.residual_at(ps["X_f"]))
    eng.close()
    never.close()


@pytest.mark.parametrize("dtype,path", CONFIGS)
def test_a_redraw_makes_the_source_stale_until_it_is_set_again(record, dtype, path):
    import pinn_native
    layers, co = tuple(layers_of(4)), adr2_ref.COEFF_SETS["all"]
    ps = point_sets(2048, 512, 50, 17)
    eng = make(layers, dtype, path, co, ps)
    eng.set_weights(weights(layers))
    eng.adam_init(1e-3, 0.9, 0.999, 1e-7)
    eng.loss_grad()
    for n_design, seed in ((2048, 0x5EED0001), (3000, 0x5EED0003)):      # in place, then another length
        eng.lhs_collocation(n_design, seed)
        for call in (eng.loss_grad, lambda: eng.adam_run(1), eng.residual):
            with pytest.raises(pinn_native.PinnNativeError, match="replaced since the source term was set"):
                call()
        X_new = eng.get_collocation()
        assert X_new.shape == (n_design, 2)
        s_new = source_of(X_new)
        eng.set_source(s_new)
        loss, grad, _ = eng.loss_grad()
        got64 = helper(weights(layers), list(layers), dict(ps, X_f=X_new), co, s=s_new)
        got32 = helper(weights(layers), list(layers), dict(ps, X_f=X_new), co, s=s_new, dtype=np.float32) if dtype == "f32" else None
        tol = bounds(dtype, got64, got32)
        dev = dict(loss=abs(loss - got64[0]) / got64[0], grad=rel(grad, got64[1]))
        record(dtype=dtype, path=path, n_design=n_design, **dev)
        assert dev["loss"] < tol["loss"] and dev["grad"] < tol["grad"]
    eng.close()


# ---- 5. residuals -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,dtype,path", [(20,) + c for c in CONFIGS] + [(33,) + c for c in GENERIC])
def test_residuals(record, width, dtype, path):
    """residual, residual_at with and without source=, robin_residual; width 20 is where the forward-only sweeps of the other
    kinds would take the width-20 MFMA kernel"""
    layers, name, key = tuple(layers_of(4 if width == 20 else 3, width)), "klein_gordon", (300, 40, 5, 7)
    ps = point_sets(*key)
    co = adr2_ref.COEFF_SETS[name]
    eng = make(layers, dtype, path, co, ps)
    plain = make(layers, dtype, path, co, ps, s=None)
    for e in (eng, plain):
        e.set_weights(weights(layers))
    f_s, f_0, r = eng.residual(), plain.residual(), eng.robin_residual()
    f_at = eng.residual_at(ps["X_f"], source=ps["s"])
    with pytest.raises(ValueError, match="source"):
        eng.residual_at(ps["X_f"])
    X_new = LB + (UB - LB) * np.random.RandomState(5).uniform(size=(77, 2))
    f_new = plain.residual_at(X_new)
    assert np.array_equal(eng.residual_at(X_new, source=np.zeros(77)), f_new)
    eng.close()
    plain.close()
    ref64 = reference(layers, name, key)
    tol = bounds(dtype, ref64, reference(layers, name, key, False, "f32") if dtype == "f32" else None)["res"]
    ex = ref64[2]
    scale = np.max(np.abs(ex["f"]))
    want_new = adr2_ref.residual(weights(layers), list(layers), LB, UB, X_new, co)
    dev = dict(res=rel(f_s, ex["f"]), minus_s=np.max(np.abs((f_s - f_0).ravel() + ps["s"])) / scale,
               at=np.max(np.abs(f_at - f_s)) / scale, new=rel(f_new, want_new), rob=rel(r, ex["r"]))
    print("adr2 residuals width %d %s: %s (bound %.1e)" % (width, dtype, dev, tol))
    record(dtype=dtype, path=path, width=width, **dev)
    assert max(dev.values()) < tol


# ---- 6. optimisers --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,path", CONFIGS)
def test_ten_adam_steps(record, dtype, path):
    """against oracle.optim.Adam driven by the helper: 1e-10 in float64, 1e-4 in float32 (losses and weights)"""
    from oracle import optim
    layers, co = tuple(layers_of(4)), adr2_ref.COEFF_SETS["telegraph"]
    ps = point_sets(2048, 512, 50, 17)
    w0 = np.array(weights(layers))
    eng = make(layers, dtype, path, co, ps)
    eng.set_weights(w0)
    eng.adam_init(1e-3, 0.9, 0.999, 1e-7)
    losses = eng.adam_run(10)
    w_dev = eng.get_weights()
    eng.close()
    opt, w, ref = optim.Adam(1e-3, 0.9, 0.999, 1e-7), w0.copy(), []
    for _ in range(10):
        l, g, _ = helper(w, list(layers), ps, co)
        ref.append(l)
        w = opt.step(w, g)
    da, dw = float(np.max(np.abs(losses - np.array(ref)) / np.array(ref))), rel(w_dev, w)
    print("adr2 adam %s: loss %.2e w %.2e" % (dtype, da, dw))
    record(dtype=dtype, path=path, adam_loss=da, adam_w=dw)
    bound = 1e-10 if dtype == "f64" else 1e-4
    assert da < bound and dw < bound


@pytest.mark.parametrize("path", [0, 7])
def test_five_lbfgs_iterations(record, path):
    """against oracle.optim.lbfgs driven by the helper, float64: 1e-8"""
    from oracle import optim
    layers, co = tuple(layers_of(4)), adr2_ref.COEFF_SETS["helmholtz"]
    ps = point_sets(2048, 512, 50, 17)
    w0 = np.array(weights(layers))
    eng = make(layers, "f64", path, co, ps)
    eng.set_weights(w0)
    eng.lbfgs_begin(5, 0.8, 50, np.finfo(float).eps)
    lo_all, done = [], 0
    while not done:
        _, lo, done = eng.lbfgs_run(3)
        lo_all.extend(lo.tolist())
    w_model = eng.get_weights()
    eng.close()
    res = optim.lbfgs(lambda w: helper(w, list(layers), ps, co)[:2], w0, 5, 0.8, 50)
    ref_l = np.array([l for _, l in res["logs"]])
    assert len(lo_all) == len(ref_l) and len(ref_l) >= 4          # (five iterations log four entries, in both)
    dl = float(np.max(np.abs(np.array(lo_all) - ref_l) / ref_l))
    dm = rel(w_model, res["x_model"])
    print("adr2 lbfgs: loss %.2e w_model %.2e (%d logged)" % (dl, dm, len(ref_l)))
    record(path=path, lbfgs_loss=dl, lbfgs_w_model=dm)
    assert dl < 1e-8 and dm < 1e-8


# ---- 7. refusals leave the context as it was ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("home", [0, 7])
def test_refusals_leave_a_following_evaluation_bit_identical(home):
    import pinn_native
    from pinn_native import _dp
    layers, co = tuple(layers_of(8)), adr2_ref.COEFF_SETS["all"]      # (2-20-...-20-1, depth 8: the shape the other paths serve)
    ps = point_sets(2048, 512, 50, 17)
    eng = make(layers, "f64", home, co, ps)
    eng.set_weights(weights(layers))
    before = eng.loss_grad()

    def same():
        assert same_bits(eng.loss_grad(), before) and eng.kernel_path() == home
        assert np.array_equal(eng.get_pde_params(), np.array(co))

    def refused(code, call, match):
        with pytest.raises(pinn_native.PinnNativeError, match=match) as ei:
            call()
        assert "(code %d)" % code in str(ei.value)
        same()

    lib, h = eng._lib, eng._h
    UNS, INV = -5, -1
    refused(UNS, eng.pw_set, "point weights")
    refused(UNS, lambda: eng.sa_set_weights(np.ones(512), np.ones(2048)), "self-adaptive weights")
    refused(UNS, lambda: eng.set_pde_trainable(["a1"]), "pinn_set_pde_trainable")
    refused(UNS, lambda: eng.set_coef_fields(np.tile(np.array(co[:6]), (2048, 1))), "coefficient fields")
    refused(UNS, lambda: eng.rad_collocation(2048, 7, 20000), "adr2 kind")
    eng.n_f = 2048
    for p in (1, 2, 3, 4, 5, 6, 8):
        refused(UNS, lambda p=p: eng.set_kernel_path(p), "adr2 kind .*paths 0 and 7 only")
    refused(UNS, lambda: eng.comm_init(pinn_native.Engine.comm_unique_id(), 1, 0), "single-device")
    bad = list(co)
    bad[7] = float("nan")
    refused(INV, lambda: eng.set_pde_params(*bad), "not finite")
    refused(INV, lambda: eng.set_pde_params(*co[:6]), "8 coefficients")
    refused(INV, lambda: eng._check(lib.pinn_get_pde_params(h, _dp(np.empty(6)), 6)), "8 coefficients")
    X1, z, one = np.array([[0.0, 0.5]]), np.zeros(1), np.ones(1)
    refused(INV, lambda: eng._check(lib.pinn_set_robin3(h, _dp(X1), _dp(z), _dp(z), _dp(z), _dp(one), 1, 1)),
            "alpha = beta = gamma = 0")
    with pytest.raises(ValueError, match="constrains nothing"):
        eng.set_robin3(X1, 0.0, 0.0, 0.0, 1.0)
    same()
    assert eng.n_w == 17
    eng.close()
    # ensembles of this kind, and three-term points on another kind
    with pytest.raises(pinn_native.PinnNativeError, match="ensembles") as ei:
        pinn_native.Ensemble(list(layers), LB, UB, 2, pde="adr2")
    assert "(code -5)" in str(ei.value)
    adr = make(layers, "f64", 0, co[:6], ps, wall=None, pde="adr")
    adr.set_weights(weights(layers))
    ref = adr.loss_grad()
    with pytest.raises(pinn_native.PinnNativeError, match="pinn_set_robin3: .*adr2 kind \\(pde 10\\) only"):
        adr.set_robin3(X1, 0.0, 0.0, 1.0, 0.0)
    assert same_bits(adr.loss_grad(), ref)
    adr.close()
