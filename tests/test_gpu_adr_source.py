"""GPU: the source term of the adr kind (pinn_set_source, Engine.set_source) against the numpy restatement
tests/helpers/adr_src_ref.py (pinned on the CPU by tests/test_adr_source_host.py).

  f_i = u_t + (a0 + a1 u) u_x - nu u_xx + r1 u + r2 u^2 + r3 u^3 - s_i,   loss = mean_f f^2 + data, pairs, Robin parts

Float64 on the generic kernels (path 0) and on k_fused20d<PDE_ADR_SRC, H, .> (path 7, one tile per workgroup and tile loop),
float32 on path 0.  Float64 bounds are tests/test_gpu_adr.py's TOL (loss 1e-12, gradient 1e-11, residual 1e-10), float32
1e-5 / 2e-5 / 2e-4, each loss term to 10 x the loss bound.  The sets and weights are tests/test_gpu_adr_robin.py's; the
source is s_i = sin(3 x_i) exp(-t_i) + 0.5, distinct at every point, so a value read at a shifted index fails."""
import functools
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
sys.path.insert(0, os.path.join(PKG, "1d-mms"))
import adr_ref  # noqa: E402
import adr_src_ref  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = {"f64": dict(loss=1e-12, grad=1e-11, res=1e-10), "f32": dict(loss=1e-5, grad=2e-5, res=2e-4)}
LB, UB = np.array([-1.0, 0.0]), np.array([1.0, 1.0])
CONFIGS = [("f64", 0), ("f64", 7), ("f32", 0)]        # (dtype, kernel path)


def rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300)


def layers_of(depth, width=20):
    return [2] + [width] * depth + [1]


def source_of(X):
    return np.sin(3.0 * X[:, 0]) * np.exp(-X[:, 1]) + 0.5


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
    assert len(np.unique(s)) == N_f
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
def reference(depth, name, N_f, n_0, n_b, n_w, with_source=True):
    """the restatement on a cell: computed once, shared, never written to"""
    X_f, X_u, u, X_lo, X_hi, s = point_sets(N_f, n_0, n_b)
    rob = robin_points(n_w) or ()
    return adr_src_ref.src_loss_grad(weights(depth), layers_of(depth), LB, UB, X_f, X_u if n_0 else None, u if n_0 else None,
                                     X_lo if n_b else None, X_hi if n_b else None, adr_ref.COEFF_SETS[name],
                                     s if with_source else None, *rob)


def make(layers, dtype, path, coeffs, X_f, X_u=None, u=None, X_lo=None, X_hi=None, robin=None, s=None, lb=LB, ub=UB):
    from pinn_native import Engine
    eng = Engine(layers, lb, ub, pde="adr", dtype=dtype)
    eng.set_pde_params(*coeffs)
    eng.set_collocation(X_f)
    if X_u is not None and len(X_u):
        eng.set_data(X_u, u)
    if X_lo is not None and len(X_lo):
        eng.set_boundary(X_lo, X_hi)
    if robin is not None:
        eng.set_robin(*robin)
    if s is not None:
        eng.set_source(s)
    eng.set_kernel_path(path)          # no skip: paths 0 and 7 must exist for every cell
    assert eng.kernel_path() == path
    return eng


def make_cell(depth, dtype, path, name, N_f, n_0, n_b, n_w, with_source=True):
    X_f, X_u, u, X_lo, X_hi, s = point_sets(N_f, n_0, n_b)
    eng = make(layers_of(depth), dtype, path, adr_ref.COEFF_SETS[name], X_f, X_u if n_0 else None, u,
               X_lo if n_b else None, X_hi, robin_points(n_w), s if with_source else None)
    eng.set_weights(weights(depth))
    return eng


def same_bits(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def check_cell(record, tag, depth, dtype, path, name, N_f, n_0, n_b, n_w=0):
    eng = make_cell(depth, dtype, path, name, N_f, n_0, n_b, n_w)
    assert eng.has_source
    loss, grad, terms = eng.loss_grad()
    f = eng.residual()
    r = eng.robin_residual()
    eng.close()
    lo, go, ex = reference(depth, name, N_f, n_0, n_b, n_w)
    l_plain = reference(depth, name, N_f, n_0, n_b, n_w, False)[0]
    tol = TOL[dtype]
    dev = dict(loss=abs(loss - lo) / lo, grad=rel(grad, go), res=rel(f, ex["f"]),
               t_f=abs(terms[0] - ex["mse_f"]) / lo, t_u=abs(terms[1] - ex["mse_u"]) / lo,
               t_b=abs(terms[2] - (ex["mse_b"] + ex["mse_w"])) / lo)
    if n_w:
        dev["rob"] = rel(r, ex["r"])
    print("adr source %s %s path %d: %s" % (tag, dtype, path, " ".join("%s %.2e" % kv for kv in sorted(dev.items()))))
    record(tag=tag, dtype=dtype, path=path, **dev)
    assert abs(lo - l_plain) / l_plain > 1e-3          # the source matters: nine orders above the float64 bound
    assert f.shape == (N_f, 1) and r.shape == (n_w,)
    assert dev["loss"] < tol["loss"]
    assert dev["grad"] < tol["grad"]
    assert dev["res"] < tol["res"]
    assert dev.get("rob", 0.0) < tol["res"]
    assert max(dev["t_f"], dev["t_u"], dev["t_b"]) < tol["loss"] * 10


# ---- 1. kernel variants: depths x one tile per workgroup (2048) / tile loop (40000: 627 tiles > 256) -----------------------
@pytest.mark.parametrize("dtype,path", CONFIGS)
@pytest.mark.parametrize("N_f", [2048, 40000])
@pytest.mark.parametrize("depth", [4, 6, 8])
def test_variants_depths_and_tile_plans(record, depth, N_f, dtype, path):
    check_cell(record, "a:d%d:Nf%d" % (depth, N_f), depth, dtype, path, "all_nonzero", N_f, 512, 0)


# ---- 2. index alignment: 2 n_b + n_0 points stand in front of the collocation block, so its start moves through the
# 16-point waves and 64-point tiles (offsets 0, 1, 50, 14, 15, 64); the block itself is shorter than a wave, straddles
# waves and tiles, or fills 32 tiles ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,path", CONFIGS)
@pytest.mark.parametrize("n_0", [0, 1, 50])
@pytest.mark.parametrize("n_b", [0, 7])
@pytest.mark.parametrize("N_f", [1, 15, 17, 63, 65, 2048])
def test_index_alignment(record, N_f, n_b, n_0, dtype, path):
    check_cell(record, "b:Nf%d:nb%d:n0%d" % (N_f, n_b, n_0), 8, dtype, path, "all_nonzero", N_f, n_0, n_b)


# ---- 3. with Robin points behind the block: g_j and s_i share tgt and must not cross --------------------------------------
@pytest.mark.parametrize("dtype,path", CONFIGS)
@pytest.mark.parametrize("N_f", [2048, 40000])
@pytest.mark.parametrize("n_w", [1, 65])
def test_with_robin_points(record, n_w, N_f, dtype, path):
    check_cell(record, "c:nw%d:Nf%d" % (n_w, N_f), 8, dtype, path, "all_nonzero", N_f, 512, 7, n_w)
    a = make_cell(8, dtype, path, "all_nonzero", N_f, 512, 7, n_w)
    b = make_cell(8, dtype, path, "all_nonzero", N_f, 512, 7, n_w, with_source=False)
    ra, rb = a.robin_residual(), b.robin_residual()
    a.close()
    b.close()
    assert np.array_equal(ra, rb)


# ---- 4. equations x set kinds ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,path", CONFIGS)
@pytest.mark.parametrize("kind", ["source", "source+data", "source+pairs", "source+robin"])
@pytest.mark.parametrize("name", sorted(adr_ref.COEFF_SETS))
def test_equations_and_set_kinds(record, name, kind, dtype, path):
    n_0 = 512 if kind == "source+data" else 0
    n_b = 50 if kind == "source+pairs" else 0
    n_w = 50 if kind == "source+robin" else 0
    check_cell(record, "d:%s:%s" % (name, kind), 8, dtype, path, name, 2048, n_0, n_b, n_w)


# ---- 5. bits ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,path", CONFIGS)
@pytest.mark.parametrize("N_f", [10000, 40000])
def test_bit_identity_and_reproducibility(N_f, dtype, path):
    X_f, X_u, u, X_lo, X_hi, s = point_sets(N_f, 512, 200)
    never = make_cell(8, dtype, path, "allen_cahn", N_f, 512, 200, 0, with_source=False)
    eng = make_cell(8, dtype, path, "allen_cahn", N_f, 512, 200, 0, with_source=False)
    ref, f_ref = never.loss_grad(), never.residual()
    # (a) a source of zeros: the plain kernels' bits from the source kernels
    eng.set_source(np.zeros(N_f))
    assert eng.has_source
    assert same_bits(eng.loss_grad(), ref) and np.array_equal(eng.residual(), f_ref)
    # (b) a real source: two evaluations are bit-identical, and differ from the plain ones
    eng.set_source(s)
    one, two = eng.loss_grad(), eng.loss_grad()
    assert same_bits(one, two) and one[0] != ref[0]
    assert np.array_equal(eng.residual(), eng.residual())
    # (c) removed: every bit is that of a context that never had one
    eng.set_source(None)
    assert not eng.has_source
    assert same_bits(eng.loss_grad(), ref) and np.array_equal(eng.residual(), f_ref)
    assert np.array_equal(eng.residual_at(X_f), never.residual_at(X_f))
    eng.close()
    never.close()


# ---- 6. in-place replacement ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,path", CONFIGS)
def test_replacing_the_source_in_place_equals_a_fresh_context(dtype, path):
    X_f, X_u, u, X_lo, X_hi, s = point_sets(2048, 512, 50)
    b_src = np.cos(2.0 * X_f[:, 0]) - X_f[:, 1]
    eng = make_cell(8, dtype, path, "all_nonzero", 2048, 512, 50, 17)
    first = eng.loss_grad()                          # the set is assembled: the next set_source is one copy
    eng.set_source(b_src)
    got, f_got, r_got = eng.loss_grad(), eng.residual(), eng.robin_residual()
    eng.close()
    fresh = make(layers_of(8), dtype, path, adr_ref.COEFF_SETS["all_nonzero"], X_f, X_u, u, X_lo, X_hi, robin_points(17), b_src)
    fresh.set_weights(weights(8))
    want, f_want, r_want = fresh.loss_grad(), fresh.residual(), fresh.robin_residual()
    fresh.close()
    assert same_bits(got, want) and np.array_equal(f_got, f_want) and np.array_equal(r_got, r_want)
    assert got[0] != first[0]


# ---- 7. residuals --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,path", CONFIGS)
def test_residuals_with_and_without_the_source(record, dtype, path):
    X_f, X_u, u, X_lo, X_hi, s = point_sets(2048, 512, 50)
    eng = make_cell(8, dtype, path, "all_nonzero", 2048, 512, 50, 0)
    plain = make_cell(8, dtype, path, "all_nonzero", 2048, 512, 50, 0, with_source=False)
    f_s, f_0 = eng.residual(), plain.residual()
    f_at = eng.residual_at(X_f, source=s)
    with pytest.raises(ValueError, match="source"):
        eng.residual_at(X_f)
    # the library call itself keeps returning the operator part
    assert np.array_equal(eng.residual_at(X_f, source=np.zeros(len(X_f))), plain.residual_at(X_f))
    eng.close()
    plain.close()
    ex = reference(8, "all_nonzero", 2048, 512, 50, 0)[2]
    tol, scale = TOL[dtype]["res"], np.max(np.abs(ex["f"]))
    dev = dict(res=rel(f_s, ex["f"]), minus_s=np.max(np.abs((f_s - f_0).ravel() + s)) / scale,
               at=np.max(np.abs(f_at - f_s)) / scale)
    record(dtype=dtype, path=path, **dev)
    assert dev["res"] < tol and dev["minus_s"] < tol and dev["at"] < tol


# ---- 8. redraws: the stale rule --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,path", CONFIGS)
def test_redraws_make_the_source_stale_until_it_is_set_again(record, dtype, path):
    import pinn_native
    layers, w, co = layers_of(8), weights(8), adr_ref.COEFF_SETS["all_nonzero"]
    X_f, X_u, u, X_lo, X_hi, s = point_sets(2048, 512, 50)
    rob = robin_points(17)
    eng = make_cell(8, dtype, path, "all_nonzero", 2048, 512, 50, 17)
    eng.adam_init(1e-3, 0.9, 0.999, 1e-7)
    eng.lbfgs_begin(5, 0.8, 50, np.finfo(float).eps)
    eng.set_weights(w)
    before = eng.loss_grad()
    # the adaptive draw is refused by name and changes nothing
    with pytest.raises(pinn_native.PinnNativeError, match="pinn_rad_collocation: .*source term.*pinn_set_source"):
        eng.rad_collocation(2048, 0x5EED0002, 20000, k=1, c=1.0)
    eng.n_f = 2048
    assert same_bits(eng.loss_grad(), before)

    def refused():
        for call in (eng.loss_grad, lambda: eng.adam_run(1), lambda: eng.adam_enqueue(1),
                     lambda: eng.lbfgs_begin(5, 0.8, 50, np.finfo(float).eps), lambda: eng.lbfgs_run(1),
                     lambda: eng.lbfgs_enqueue(1), eng.residual):
            with pytest.raises(pinn_native.PinnNativeError, match="pinn_set_source") as ei:
                call()
            assert "replaced since the source term was set" in str(ei.value)

    def evaluates_on(X_new, tag):
        s_new = source_of(X_new)
        eng.set_source(s_new)
        loss, grad, terms = eng.loss_grad()
        f = eng.residual()
        lo, go, ex = adr_src_ref.src_loss_grad(w, layers, LB, UB, X_new, X_u, u, X_lo, X_hi, co, s_new, *rob)
        tol = TOL[dtype]
        dev = dict(loss=abs(loss - lo) / lo, grad=rel(grad, go), res=rel(f, ex["f"]))
        record(tag=tag, dtype=dtype, path=path, **dev)
        assert dev["loss"] < tol["loss"] and dev["grad"] < tol["grad"] and dev["res"] < tol["res"]

    # an in-place Latin hypercube (same count), then one of another length, then points handed over
    for n_design, seed in ((2048, 0x5EED0001), (3000, 0x5EED0003)):
        eng.lhs_collocation(n_design, seed)
        refused()
        X_new = eng.get_collocation()                # still works while stale: this is how the caller gets the points
        assert X_new.shape == (n_design, 2) and not np.array_equal(X_new[:5], X_f[:5])
        refused()
        evaluates_on(X_new, "lhs%d" % n_design)
    eng.set_collocation(X_f[:1000])
    refused()
    with pytest.raises(pinn_native.PinnNativeError, match="pinn_set_source: 3000 values for 1000"):
        eng._check(eng._lib.pinn_set_source(eng._h, pinn_native._dp(np.zeros(3000)), 3000))
    refused()
    evaluates_on(eng.get_collocation(), "set1000")
    # n = 0 clears the state as well
    eng.set_collocation(X_f)
    refused()
    eng.set_source(None)
    plain = make_cell(8, dtype, path, "all_nonzero", 2048, 512, 50, 17, with_source=False)
    assert same_bits(eng.loss_grad(), plain.loss_grad())
    eng.close()
    plain.close()


# ---- 9. trajectories ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", [0, 7])
def test_adam_and_lbfgs_trajectories(record, path):
    """30 Adam steps (lr 1e-3) and 25 L-BFGS iterations (N_f = 2048, 512 data points, 50 pairs, 17 Robin points, the source)
    against oracle.optim driven by adr_src_ref, float64, at the 1e-8 the README states for trajectories"""
    from oracle import optim
    layers = layers_of(8)
    X_f, X_u, u, X_lo, X_hi, s = point_sets(2048, 512, 50)
    rob = robin_points(17)
    co = adr_ref.COEFF_SETS["all_nonzero"]
    w0 = np.array(weights(8))

    def fg(w):
        l, g, _ = adr_src_ref.src_loss_grad(w, layers, LB, UB, X_f, X_u, u, X_lo, X_hi, co, s, *rob)
        return l, g

    eng = make_cell(8, "f64", path, "all_nonzero", 2048, 512, 50, 17)
    eng.set_weights(w0)
    eng.adam_init(1e-3, 0.9, 0.999, 1e-7)
    losses = eng.adam_run(30)
    w_dev = eng.get_weights()
    opt, w, ref = optim.Adam(1e-3, 0.9, 0.999, 1e-7), w0.copy(), []
    for _ in range(30):
        l, g = fg(w)
        ref.append(l)
        w = opt.step(w, g)
    da, dw = float(np.max(np.abs(losses - np.array(ref)) / np.array(ref))), rel(w_dev, w)
    eng.set_weights(w0)
    eng.lbfgs_begin(25, 0.8, 50, np.finfo(float).eps)
    lo_all, done = [], 0
    while not done:
        it, lo, done = eng.lbfgs_run(7)
        lo_all.extend(lo.tolist())
    w_model = eng.get_weights()
    eng.close()
    res = optim.lbfgs(fg, w0, 25, 0.8, 50)
    ref_l = np.array([l for _, l in res["logs"]])
    n = min(len(lo_all), len(ref_l))
    dl = float(np.max(np.abs(np.array(lo_all[:n]) - ref_l[:n]) / ref_l[:n]))
    dm = rel(w_model, res["x_model"])
    print("adr source trajectories path %d: adam loss %.2e w %.2e | lbfgs loss %.2e w_model %.2e (%d logged)" % (path, da, dw, dl, dm, n))
    record(path=path, adam_loss=da, adam_w=dw, lbfgs_loss=dl, lbfgs_w_model=dm)
    assert n >= 20 and len(lo_all) == len(ref_l)
    assert da < 1e-8 and dw < 1e-8
    assert dl < 1e-8 and dm < 1e-8


# ---- 10. refusals leave the context usable -----------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable():
    import pinn_native
    layers, w = layers_of(8), weights(8)
    X_f, X_u, u, X_lo, X_hi, s = point_sets(2048, 512, 50)
    eng = make_cell(8, "f64", 7, "allen_cahn", 2048, 512, 50, 0)       # (no Robin points: their own refusal of pw_set comes first)
    before = eng.loss_grad()

    def same(e=eng, ref=before, path=7):
        assert same_bits(e.loss_grad(), ref)
        assert e.kernel_path() == path

    # another length than the collocation set, through the library itself (Engine.set_source would stop it first)
    with pytest.raises(pinn_native.PinnNativeError, match="pinn_set_source: 100 values for 2048"):
        eng._check(eng._lib.pinn_set_source(eng._h, pinn_native._dp(np.zeros(100)), 100))
    with pytest.raises(ValueError, match="one value per collocation point"):
        eng.set_source(np.zeros(100))
    assert eng._lib.pinn_set_source(eng._h, pinn_native._dp(np.full(2048, np.nan)), 2048) == -1
    same()
    with pytest.raises(pinn_native.PinnNativeError, match="pinn_pw_set: point weights are not combined with a source term"):
        eng.pw_set()
    same()
    for path in (4, 1, 2, 3, 5, 6, 8):
        with pytest.raises(pinn_native.PinnNativeError, match="adr kind .*paths 0 and 7 only"):
            eng.set_kernel_path(path)
        same()
    eng.close()
    # point weights on: set_source is refused, the weighted results stay
    pw = make_cell(8, "f64", 7, "allen_cahn", 2048, 512, 50, 0, with_source=False)
    pw.pw_set(np.full(len(X_u), 2.0), None, None)
    ref = pw.loss_grad()
    with pytest.raises(pinn_native.PinnNativeError, match="pinn_set_source: point weights are not combined with a source term"):
        pw.set_source(s)
    assert not pw.has_source
    same(pw, ref)
    pw.close()
    # the adr_ide kind, named
    ide = pinn_native.Engine(layers, LB, UB, pde="adr_ide", dtype="f64")
    ide.set_pde_params(*adr_ref.ALLEN_CAHN)
    ide.set_collocation(X_f)
    ide.set_data(X_u, u)
    ide.set_weights(np.concatenate([w, ide.get_weights()[-6:]]))
    ref = ide.loss_grad()
    with pytest.raises(pinn_native.PinnNativeError, match="pinn_set_source: .*adr kind \\(pde 5\\) only.*adr_ide"):
        ide.set_source(s)
    same(ide, ref, ide.kernel_path())
    ide.close()
    # kinds 0, 1, 2
    for pde, lay in (("burgers", layers), ("burgers_ide", layers), ("schrodinger", [2, 20, 20, 20, 20, 2])):
        other = pinn_native.Engine(lay, LB, UB, pde=pde, dtype="f64")
        other.n_f = 2048
        with pytest.raises(pinn_native.PinnNativeError, match="pinn_set_source: .*adr kind \\(pde 5\\) only"):
            other.set_source(s)
        assert not other.has_source
        other.close()


# ---- 11. the script -------------------------------------------------------------------------------------------------------------------
LINE = re.compile(r"^(tf_epoch|nt_epoch) =\s+(\d+)\s+elapsed = \d\d:\d\d \(\+\d\d\.\d\)  loss = (\S+)  ")
END = re.compile(r"^Training finished \(epoch (\d+)\): duration = \d\d:\d\d  error = (\S+)  ")
SHORT_HP = {"equation": "fisher_kpp", "N_0": 128, "N_w": 64, "N_f": 2048, "layers": layers_of(8), "seed": 1234,
            "tf_epochs": 10, "tf_lr": 0.003, "tf_b1": 0.9, "tf_eps": None,
            "nt_epochs": 10, "nt_lr": 0.8, "nt_ncorr": 50, "log_frequency": 5}


@pytest.mark.parametrize("walls", ["dirichlet", "periodic"])
def test_script_runs_and_its_first_logged_loss_is_the_restatements(tmp_path, walls):
    """inf_cont_mms.py with a short hp as a child process: Logger lines in the existing format, a finite final error, the
    residual line, a result folder.  Its first logged loss is the restatement's on the same sets (rebuilt here from the same
    hp and seeds) and initial weights, to the four digits the log prints."""
    hp = dict(SHORT_HP, walls=walls)
    hp_file = tmp_path / "hp.json"
    hp_file.write_text(json.dumps(hp))
    env = dict(os.environ, MPLBACKEND="Agg")
    env.pop("PINN_NO_PLOT", None)
    res = subprocess.run([sys.executable, os.path.join(PKG, "1d-mms", "inf_cont_mms.py"), str(hp_file)],
                         cwd=PKG, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    out = res.stdout
    assert "-- Starting Adam optimization --" in out and "-- Starting LBFGS optimization --" in out
    rows = [(m.group(1), int(m.group(2)), m.group(3)) for m in map(LINE.match, out.splitlines()) if m]
    assert [r[:2] for r in rows[:2]] == [("tf_epoch", 0), ("tf_epoch", 5)]
    assert any(r[0] == "nt_epoch" for r in rows)
    assert all(np.isfinite(float(r[2])) for r in rows)
    ends = [m for m in map(END.match, out.splitlines()) if m]
    assert len(ends) == 1 and int(ends[0].group(1)) == 20 and np.isfinite(float(ends[0].group(2)))
    line = re.search(r"^Residual with the source: max \|N\[u\] - s\| = (\S+) over 2048 points \(fisher_kpp, %s walls\)" % walls,
                     out, re.M)
    assert line and np.isfinite(float(line.group(1)))
    m = re.search(r"Saving results to directory\s+(\S+)", out)
    assert m and os.path.isfile(os.path.join(m.group(1), "hp.json")) and os.path.isfile(os.path.join(m.group(1), "weights.npy"))

    # the number behind the first line
    sys.path.insert(0, os.path.join(PKG, "utils"))
    import mmsutil as mu
    import neuralnetwork as nn
    from logger import Logger
    np.random.seed(1234)
    (x, t, X, T, Exact_u, X_star, u_star, X_u, u, X_f, wall, ub, lb) = mu.prep_data(hp["N_0"], hp["N_w"], hp["N_f"], walls=walls)

    class Model(nn.NeuralNetwork):
        pde = "adr"

    pinn = Model(dict(hp), Logger(dict(hp, log_frequency=10 ** 9)), ub, lb)
    w0 = np.asarray(pinn.get_weights()).ravel()
    pinn._engine.close()
    co = mu.adr_coeffs(hp["equation"])
    pairs = wall[1:] if walls == "periodic" else (None, None)
    rob = wall[1:] if walls == "dirichlet" else ()
    lo, _, ex = adr_src_ref.src_loss_grad(w0, hp["layers"], lb, ub, X_f, X_u, u, pairs[0], pairs[1], co, mu.source(X_f, co), *rob)
    l_plain = adr_src_ref.src_loss_grad(w0, hp["layers"], lb, ub, X_f, X_u, u, pairs[0], pairs[1], co, None, *rob)[0]
    print("first loss: restatement %.17g (without the source %.4e) printed %s" % (lo, l_plain, rows[0][2]))
    assert (ex["mse_w"] > 0) == (walls == "dirichlet") and (ex["mse_b"] > 0) == (walls == "periodic")
    assert "%.4e" % l_plain != "%.4e" % lo
    assert rows[0][2] == "%.4e" % lo
