"""GPU: per-point coefficient fields of the adr kind (pinn_set_coef_fields, Engine.set_coef_fields) against the numpy
restatement tests/helpers/adr_var_ref.py (pinned on the CPU by tests/test_adr_var_host.py).

  f_i = u_t + (a0_i + a1_i u) u_x - nu_i u_xx + r1_i u + r2_i u^2 + r3_i u^3 - s_i,   loss = mean_f f^2 + data, pairs, Robin

Float64 on the generic kernels (path 0) and on k_fused20d<PDE_ADR_VAR, H, .> (path 7, one tile per workgroup and tile loop),
float32 on path 0.  Float64 bounds are tests/test_gpu_adr.py's TOL (loss 1e-12, gradient 1e-11, residual 1e-10), float32
1e-5 / 2e-5 / 2e-4, each loss term to 10 x the loss bound.  Sets, weights, cells and the test fields are
tests/helpers/adr_var_cells.py's (the sets and weights of tests/test_gpu_adr_source.py): six columns distinct at every point,
so a shifted index, a swapped column or a read of the constants fails; every cell's loss moves by at least 10 % against the
constant set (asserted on the CPU for the same cells, and here again from the shared restatement)."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
sys.path.insert(0, os.path.join(PKG, "utils"))
import adr_ref  # noqa: E402
import adr_var_cells as cells  # noqa: E402
import adr_var_ref  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = {"f64": dict(loss=1e-12, grad=1e-11, res=1e-10), "f32": dict(loss=1e-5, grad=2e-5, res=2e-4)}
LB, UB = cells.LB, cells.UB
CONFIGS = [("f64", 0), ("f64", 7), ("f32", 0)]        # (dtype, kernel path)
layers_of, weights, point_sets, robin_points, fields_of, source_of = (
    cells.layers_of, cells.weights, cells.point_sets, cells.robin_points, cells.fields_of, cells.source_of)


def rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300)


def make(layers, dtype, path, coeffs, X_f, X_u=None, u=None, X_lo=None, X_hi=None, robin=None, s=None, K=None, lb=LB, ub=UB):
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
    if K is not None:
        eng.set_coef_fields(K)
    eng.set_kernel_path(path)          # no skip: paths 0 and 7 must exist for every cell
    assert eng.kernel_path() == path
    return eng


def make_cell(depth, dtype, path, name, N_f, n_0, n_b, n_w, with_source=True, fields=True):
    X_f, X_u, u, X_lo, X_hi, s = point_sets(N_f, n_0, n_b)
    K = (cells.cell_fields(name, N_f, n_0, n_b) if fields is True else fields) if fields is not False else None
    eng = make(layers_of(depth), dtype, path, adr_ref.COEFF_SETS[name], X_f, X_u if n_0 else None, u,
               X_lo if n_b else None, X_hi, robin_points(n_w), s if with_source else None, K)
    eng.set_weights(weights(depth))
    return eng


def same_bits(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def check_cell(record, dtype, path, tag, depth, name, N_f, n_0, n_b, n_w, with_source):
    eng = make_cell(depth, dtype, path, name, N_f, n_0, n_b, n_w, with_source)
    assert eng.has_coef_fields and eng.has_source == with_source
    loss, grad, terms = eng.loss_grad()
    f = eng.residual()
    r = eng.robin_residual()
    eng.close()
    lo, go, ex = cells.reference(depth, name, N_f, n_0, n_b, n_w, with_source)
    l_const = cells.constant_loss(depth, name, N_f, n_0, n_b, n_w, with_source)
    tol = TOL[dtype]
    dev = dict(loss=abs(loss - lo) / lo, grad=rel(grad, go), res=rel(f, ex["f"]),
               t_f=abs(terms[0] - ex["mse_f"]) / lo, t_u=abs(terms[1] - ex["mse_u"]) / lo,
               t_b=abs(terms[2] - (ex["mse_b"] + ex["mse_w"])) / lo)
    if n_w:
        dev["rob"] = rel(r, ex["r"])
    print("adr fields %s %s path %d: %s" % (tag, dtype, path, " ".join("%s %.2e" % kv for kv in sorted(dev.items()))))
    record(tag=tag, dtype=dtype, path=path, **dev)
    assert abs(lo - l_const) / l_const >= 0.10          # the fields matter: a read of the constants fails the loss check
    assert f.shape == (N_f, 1) and r.shape == (n_w,)
    assert dev["loss"] < tol["loss"]
    assert dev["grad"] < tol["grad"]
    assert dev["res"] < tol["res"]
    assert dev.get("rob", 0.0) < tol["res"]
    assert max(dev["t_f"], dev["t_u"], dev["t_b"]) < tol["loss"] * 10


# ---- 1. kernel variants: depths x one tile per workgroup (2048) / tile loop (40000: 627 tiles > 256) -----------------------
@pytest.mark.parametrize("dtype,path", CONFIGS)
@pytest.mark.parametrize("cell", cells.variant_cells(), ids=lambda c: c[0])
def test_variants_depths_and_tile_plans(record, cell, dtype, path):
    check_cell(record, dtype, path, *cell)


# ---- 2. index alignment: 2 n_b + n_0 points stand in front of the collocation block, so table row 0 sits at every lane
# position (offsets 0, 1, 14, 15, 50, 64); the block is shorter than a wave, fills one, straddles waves and tiles, or fills
# 32 tiles -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,path", CONFIGS)
@pytest.mark.parametrize("cell", cells.alignment_cells(), ids=lambda c: c[0])
def test_index_alignment(record, cell, dtype, path):
    check_cell(record, dtype, path, *cell)


# ---- 3. Robin points behind the block (0, 1, 50), with and without a source: the table ends where the Robin block begins ----
@pytest.mark.parametrize("dtype,path", CONFIGS)
@pytest.mark.parametrize("cell", cells.robin_cells(), ids=lambda c: c[0])
def test_with_robin_points_and_source(record, cell, dtype, path):
    check_cell(record, dtype, path, *cell)
    tag, depth, name, N_f, n_0, n_b, n_w, src = cell
    if n_w:
        a = make_cell(depth, dtype, path, name, N_f, n_0, n_b, n_w, src)
        b = make_cell(depth, dtype, path, name, N_f, n_0, n_b, n_w, src, fields=False)
        ra, rb = a.robin_residual(), b.robin_residual()
        a.close()
        b.close()
        assert np.array_equal(ra, rb)


# ---- 4. the five equations --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,path", CONFIGS)
@pytest.mark.parametrize("cell", cells.equation_cells(), ids=lambda c: c[0])
def test_equations(record, cell, dtype, path):
    check_cell(record, dtype, path, *cell)


# ---- 5. the bit rule ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,path", CONFIGS)
@pytest.mark.parametrize("N_f", [2048, 40000])
@pytest.mark.parametrize("n_w", [0, 17])
def test_constant_rows_removal_and_reproducibility_bit_for_bit(n_w, N_f, dtype, path):
    name = "all_nonzero"
    co = adr_ref.COEFF_SETS[name]
    X_f, X_u, u, X_lo, X_hi, s = point_sets(N_f, 512, 200)
    never = make_cell(8, dtype, path, name, N_f, 512, 200, n_w, with_source=False, fields=False)
    ref, f_ref, r_ref = never.loss_grad(), never.residual(), never.robin_residual()
    eng = make_cell(8, dtype, path, name, N_f, 512, 200, n_w, with_source=False, fields=False)
    # (a) every row the constant set, no source: the bits of the context without fields, from the field kernels
    eng.set_coef_fields(adr_var_ref.constant_rows(co, N_f))
    assert eng.has_coef_fields
    assert same_bits(eng.loss_grad(), ref) and np.array_equal(eng.residual(), f_ref) and np.array_equal(eng.robin_residual(), r_ref)
    # (b) and a source of zeros
    eng.set_source(np.zeros(N_f))
    assert same_bits(eng.loss_grad(), ref) and np.array_equal(eng.residual(), f_ref)
    # (c) constant rows with a real source: the bits of the source kernels
    eng.set_source(s)
    with_s = make_cell(8, dtype, path, name, N_f, 512, 200, n_w, with_source=True, fields=False)
    assert same_bits(eng.loss_grad(), with_s.loss_grad()) and np.array_equal(eng.residual(), with_s.residual())
    with_s.close()
    eng.set_source(None)
    # (d) while fields are present the constants are not read: other constants, the same bits; they count again after removal
    eng.set_pde_params(9.0, 9.0, 9.0, 9.0, 9.0, 9.0)
    assert same_bits(eng.loss_grad(), ref) and np.array_equal(eng.residual(), f_ref)
    assert list(eng.get_pde_params()) == [9.0] * 6
    eng.set_pde_params(*co)
    # (e) real fields: two evaluations are bit-identical, and differ from the plain ones
    eng.set_coef_fields(cells.cell_fields(name, N_f, 512, 200))
    one, two = eng.loss_grad(), eng.loss_grad()
    assert same_bits(one, two) and one[0] != ref[0]
    assert np.array_equal(eng.residual(), eng.residual())
    # (f) removed: every bit is that of a context that never had them
    eng.set_coef_fields(None)
    assert not eng.has_coef_fields
    assert same_bits(eng.loss_grad(), ref) and np.array_equal(eng.residual(), f_ref) and np.array_equal(eng.robin_residual(), r_ref)
    assert np.array_equal(eng.residual_at(X_f[:100]), never.residual_at(X_f[:100]))
    eng.close()
    never.close()


# ---- 6. in-place replacement ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,path", CONFIGS)
def test_replacing_the_fields_in_place_equals_a_fresh_context(dtype, path):
    X_f, X_u, u, X_lo, X_hi, s = point_sets(2048, 512, 50)
    K_b = fields_of(X_f[::-1], adr_ref.COEFF_SETS["fisher_kpp"])
    eng = make_cell(8, dtype, path, "all_nonzero", 2048, 512, 50, 17)
    first = eng.loss_grad()                          # the set is assembled: the next set_coef_fields is one copy
    eng.set_coef_fields(K_b)
    got, f_got, r_got = eng.loss_grad(), eng.residual(), eng.robin_residual()
    eng.close()
    fresh = make(layers_of(8), dtype, path, adr_ref.COEFF_SETS["all_nonzero"], X_f, X_u, u, X_lo, X_hi, robin_points(17), s, K_b)
    fresh.set_weights(weights(8))
    want, f_want, r_want = fresh.loss_grad(), fresh.residual(), fresh.robin_residual()
    fresh.close()
    assert same_bits(got, want) and np.array_equal(f_got, f_want) and np.array_equal(r_got, r_want)
    assert got[0] != first[0]


# ---- 7. the fields survive the other setters ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,path", CONFIGS)
def test_fields_survive_the_other_setters(dtype, path):
    X_f, X_u, u, X_lo, X_hi, s = point_sets(2048, 512, 50)
    eng = make_cell(8, dtype, path, "all_nonzero", 2048, 0, 0, 0, with_source=False)
    eng.loss_grad()
    eng.set_data(X_u, u)
    eng.set_boundary(X_lo, X_hi)
    eng.set_robin(*robin_points(17))
    eng.set_source(s)
    eng.set_pde_params(*adr_ref.COEFF_SETS["burgers"])
    assert eng.has_coef_fields
    loss, grad, terms = eng.loss_grad()
    f = eng.residual()
    eng.close()
    lo, go, ex = cells.reference(8, "all_nonzero", 2048, 512, 50, 17, True)
    tol = TOL[dtype]
    assert abs(loss - lo) / lo < tol["loss"] and rel(grad, go) < tol["grad"] and rel(f, ex["f"]) < tol["res"]


# ---- 8. redraws: the stale rule --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,path", CONFIGS)
def test_redraws_make_the_fields_stale_until_they_are_set_again(record, dtype, path):
    import pinn_native
    layers, w, co = layers_of(8), weights(8), adr_ref.COEFF_SETS["all_nonzero"]
    X_f, X_u, u, X_lo, X_hi, s = point_sets(2048, 512, 50)
    rob = robin_points(17)
    eng = make_cell(8, dtype, path, "all_nonzero", 2048, 512, 50, 17, with_source=False)
    eng.adam_init(1e-3, 0.9, 0.999, 1e-7)
    eng.lbfgs_begin(5, 0.8, 50, np.finfo(float).eps)
    eng.set_weights(w)
    before = eng.loss_grad()
    # the adaptive draw is refused by name, first: it changes nothing and makes nothing stale
    with pytest.raises(pinn_native.PinnNativeError, match="pinn_rad_collocation: .*coefficient fields.*pinn_set_coef_fields"):
        eng.rad_collocation(2048, 0x5EED0002, 20000, k=1, c=1.0)
    eng.n_f = 2048
    assert same_bits(eng.loss_grad(), before)
    with pytest.raises(pinn_native.PinnNativeError, match="pinn_residual_at: .*coefficient fields.*foreign points"):
        eng.residual_at(X_f[:10])

    def refused(both=False):
        w_dev = eng.get_weights()
        for call in (eng.loss_grad, lambda: eng.adam_run(1), lambda: eng.adam_enqueue(1),
                     lambda: eng.lbfgs_begin(5, 0.8, 50, np.finfo(float).eps), lambda: eng.lbfgs_run(1),
                     lambda: eng.lbfgs_enqueue(1), eng.residual):
            with pytest.raises(pinn_native.PinnNativeError, match="pinn_set_coef_fields") as ei:
                call()
            msg = str(ei.value)
            assert msg.endswith("(code -3)")                       # PINN_ESTATE
            if both:
                assert "the source term and the coefficient fields" in msg and "pinn_set_source" in msg
            else:
                assert "replaced since the coefficient fields were set" in msg and "pinn_set_source" not in msg
        assert np.array_equal(eng.get_weights(), w_dev)            # no optimiser state moved

    def evaluates_on(X_new, tag, s_new=None):
        K_new = fields_of(X_new, co)
        eng.set_coef_fields(K_new)
        loss, grad, terms = eng.loss_grad()
        f = eng.residual()
        lo, go, ex = adr_var_ref.var_loss_grad(w, layers, LB, UB, X_new, X_u, u, X_lo, X_hi, K_new, s_new, *rob)
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
    with pytest.raises(pinn_native.PinnNativeError, match="pinn_set_coef_fields: 3000 rows for 1000"):
        eng._check(eng._lib.pinn_set_coef_fields(eng._h, pinn_native._dp(np.zeros((3000, 6))), 3000))
    refused()
    evaluates_on(eng.get_collocation(), "set1000")
    # a source and fields both stale: the message names both; each is cleared by its own setter
    eng.set_collocation(X_f)
    eng.set_coef_fields(fields_of(X_f, co))
    eng.set_source(s)
    eng.lhs_collocation(2048, 0x5EED0005)
    refused(both=True)
    X_new = eng.get_collocation()
    eng.set_source(source_of(X_new))
    refused()                                        # the fields are still stale, the source no longer
    evaluates_on(X_new, "both", source_of(X_new))
    eng.lhs_collocation(2048, 0x5EED0006)
    eng.set_coef_fields(fields_of(eng.get_collocation(), co))
    with pytest.raises(pinn_native.PinnNativeError, match="replaced since the source term was set"):
        eng.loss_grad()
    eng.set_source(None)
    eng.loss_grad()
    # n = 0 clears the state as well
    eng.set_collocation(X_f)
    refused()
    eng.set_coef_fields(None)
    plain = make_cell(8, dtype, path, "all_nonzero", 2048, 512, 50, 17, with_source=False, fields=False)
    assert same_bits(eng.loss_grad(), plain.loss_grad())
    eng.close()
    plain.close()


@pytest.mark.parametrize("dtype,path", CONFIGS)
def test_lhs_redraw_with_fields_is_the_draw_of_a_context_without(dtype, path):
    a = make_cell(8, dtype, path, "all_nonzero", 2048, 512, 50, 0)
    b = make_cell(8, dtype, path, "all_nonzero", 2048, 512, 50, 0, with_source=False, fields=False)
    a.loss_grad()
    b.loss_grad()
    for n_design, seed in ((2048, 0x5EED0011), (3000, 0x5EED0012)):      # in place, then re-assembled
        a.lhs_collocation(n_design, seed)
        b.lhs_collocation(n_design, seed)
        assert np.array_equal(a.get_collocation(), b.get_collocation())
    a.close()
    b.close()


# ---- 9. through NeuralNetwork: a callable follows the redraws ------------------------------------------------------------------
def test_a_callable_through_neuralnetwork_follows_two_redraws():
    import neuralnetwork as nn
    from logger import Logger
    co = adr_ref.COEFF_SETS["all_nonzero"]
    X_f, X_u, u, X_lo, X_hi, s = point_sets(2048, 512, 50)
    hp = {"layers": layers_of(8), "tf_epochs": 25, "tf_lr": 1e-3, "tf_b1": 0.9, "tf_eps": None, "nt_epochs": 2, "nt_lr": 0.8,
          "nt_ncorr": 50, "log_frequency": 10 ** 9, "resample_every": 10, "resample_seed": 77}
    seen = []

    def k_of(X):
        seen.append(np.array(X))
        return fields_of(X, co)

    class Model(nn.NeuralNetwork):
        pde = "adr"

    logger = Logger(dict(hp))
    logger.set_error_fn(lambda: 0.0)
    pinn = Model(dict(hp), logger, UB, LB)
    eng = pinn._engine
    eng.set_pde_params(*co)
    pinn._set_collocation(X_f)
    pinn._set_boundary(X_lo, X_hi)
    pinn._set_coef_fields({"a0": lambda X: k_of(X)[:, 0], "nu": lambda X: fields_of(X, co)[:, 2]})
    pinn._set_source(source_of)
    pinn.fit(X_u, u)
    assert len(seen) == 3                                   # at the first points and after the redraws at epochs 10 and 20
    X_cur = eng.get_collocation()
    assert np.array_equal(seen[0], X_f) and np.array_equal(seen[2], X_cur) and not np.array_equal(seen[1], seen[2])
    assert not np.array_equal(seen[0], seen[1])
    K = np.tile(co, (2048, 1))
    K[:, 0], K[:, 2] = fields_of(X_cur, co)[:, 0], fields_of(X_cur, co)[:, 2]
    w = eng.get_weights()
    loss, grad, _ = eng.loss_grad()
    lo, go, _ = adr_var_ref.var_loss_grad(w, hp["layers"], LB, UB, X_cur, X_u, u, X_lo, X_hi, K, source_of(X_cur))
    eng.close()
    assert abs(loss - lo) / lo < TOL["f64"]["loss"] and rel(grad, go) < TOL["f64"]["grad"]


# ---- 10. trajectories ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", [0, 7])
def test_adam_and_lbfgs_trajectories(record, path):
    """30 Adam steps (lr 1e-3) and 25 L-BFGS iterations (N_f = 2048, 512 data points, 50 pairs, 17 Robin points, the fields and
    the source) against oracle.optim driven by adr_var_ref, float64, at the 1e-8 the README states for trajectories"""
    from oracle import optim
    layers = layers_of(8)
    X_f, X_u, u, X_lo, X_hi, s = point_sets(2048, 512, 50)
    rob = robin_points(17)
    K = cells.cell_fields("all_nonzero", 2048, 512, 50)
    w0 = np.array(weights(8))

    def fg(w):
        l, g, _ = adr_var_ref.var_loss_grad(w, layers, LB, UB, X_f, X_u, u, X_lo, X_hi, K, s, *rob)
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
    print("adr fields trajectories path %d: adam loss %.2e w %.2e | lbfgs loss %.2e w_model %.2e (%d logged)" % (path, da, dw, dl, dm, n))
    record(path=path, adam_loss=da, adam_w=dw, lbfgs_loss=dl, lbfgs_w_model=dm)
    assert n >= 20 and len(lo_all) == len(ref_l)
    assert da < 1e-8 and dw < 1e-8
    assert dl < 1e-8 and dm < 1e-8


# ---- 11. refusals leave the context usable -----------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable():
    import pinn_native
    layers, w = layers_of(8), weights(8)
    X_f, X_u, u, X_lo, X_hi, s = point_sets(2048, 512, 50)
    K = cells.cell_fields("allen_cahn", 2048, 512, 50)
    eng = make_cell(8, "f64", 7, "allen_cahn", 2048, 512, 50, 0, with_source=False)   # (no Robin points, no source: their own
    before = eng.loss_grad()                                                           #  refusals of pw_set come first)

    def same(e=eng, ref=before, path=7):
        assert same_bits(e.loss_grad(), ref)
        assert e.kernel_path() == path

    # another length than the collocation set, through the library itself (Engine.set_coef_fields would stop it first)
    with pytest.raises(pinn_native.PinnNativeError, match="pinn_set_coef_fields: 100 rows for 2048"):
        eng._check(eng._lib.pinn_set_coef_fields(eng._h, pinn_native._dp(np.zeros((100, 6))), 100))
    with pytest.raises(ValueError, match="one row per collocation point"):
        eng.set_coef_fields(np.zeros((100, 6)))
    bad = np.array(K)
    bad[2047, 5] = np.nan
    assert eng._lib.pinn_set_coef_fields(eng._h, pinn_native._dp(bad), 2048) == -1
    same()
    with pytest.raises(pinn_native.PinnNativeError, match="pinn_pw_set: point weights are not combined with coefficient fields"):
        eng.pw_set()
    same()
    for path in (4, 1, 2, 3, 5, 6, 8):
        with pytest.raises(pinn_native.PinnNativeError, match="adr kind .*paths 0 and 7 only"):
            eng.set_kernel_path(path)
        same()
    # pw_set's pinned refusals still come first: the source's, then Robin's
    eng.set_source(s)
    with pytest.raises(pinn_native.PinnNativeError, match="pinn_pw_set: point weights are not combined with a source term"):
        eng.pw_set()
    eng.set_source(None)
    eng.set_robin(*robin_points(17))
    with pytest.raises(pinn_native.PinnNativeError, match="pinn_pw_set: point weights do not cover Robin points"):
        eng.pw_set()
    eng.set_robin(np.zeros((0, 2)), np.zeros(0), np.zeros(0), np.zeros(0))
    same()
    eng.close()
    # point weights on: set_coef_fields is refused, the weighted results stay
    pw = make_cell(8, "f64", 7, "allen_cahn", 2048, 512, 50, 0, with_source=False, fields=False)
    pw.pw_set(np.full(len(X_u), 2.0), None, None)
    ref = pw.loss_grad()
    with pytest.raises(pinn_native.PinnNativeError, match="pinn_set_coef_fields: point weights are not combined with coefficient fields"):
        pw.set_coef_fields(K)
    assert not pw.has_coef_fields
    same(pw, ref)
    pw.close()
    # fields present: no communicator is attached (the other order is the next test)
    eng = make_cell(8, "f64", 7, "allen_cahn", 2048, 512, 50, 0, with_source=False)
    with pytest.raises(pinn_native.PinnNativeError, match="pinn_comm_init: coefficient fields are single-device"):
        eng.comm_init(b"\0" * 128, 1, 0)
    same(eng)
    with pytest.raises(pinn_native.PinnNativeError, match="pinn_comm_xgmi_export: coefficient fields are single-device"):
        eng.comm_xgmi_export(1, 0)
    same(eng)
    eng.close()
    # the adr_ide kind, named
    ide = pinn_native.Engine(layers, LB, UB, pde="adr_ide", dtype="f64")
    ide.set_pde_params(*adr_ref.ALLEN_CAHN)
    ide.set_collocation(X_f)
    ide.set_data(X_u, u)
    ide.set_weights(np.concatenate([w, ide.get_weights()[-6:]]))
    ref = ide.loss_grad()
    with pytest.raises(pinn_native.PinnNativeError, match="pinn_set_coef_fields: .*adr kind \\(pde 5\\) only.*adr_ide"):
        ide.set_coef_fields(K)
    same(ide, ref, ide.kernel_path())
    ide.close()
    # kinds 0, 1, 2
    for pde, lay in (("burgers", layers), ("burgers_ide", layers), ("schrodinger", [2, 20, 20, 20, 20, 2])):
        other = pinn_native.Engine(lay, LB, UB, pde=pde, dtype="f64")
        other.n_f = 2048
        with pytest.raises(pinn_native.PinnNativeError, match="pinn_set_coef_fields: .*adr kind \\(pde 5\\) only"):
            other.set_coef_fields(K)
        assert not other.has_coef_fields
        other.close()


@pytest.mark.parametrize("how", ["comm_init", "comm_xgmi_export"])
def test_a_context_with_a_communicator_refuses_the_fields(how):
    """PINN_EUNSUPPORTED for an attached communicator: one rank (the only size one device allows), by RCCL or with the
    exported mailbox; loss, gradient, terms and path stay what they were"""
    import pinn_native
    K = cells.cell_fields("allen_cahn", 2048, 512, 50)
    eng = make_cell(8, "f64", 7, "allen_cahn", 2048, 512, 50, 0, with_source=False, fields=False)
    if how == "comm_init":
        eng.comm_init(pinn_native.Engine.comm_unique_id(), 1, 0)
    else:
        eng.comm_xgmi_export(1, 0)
    before = eng.loss_grad()
    with pytest.raises(pinn_native.PinnNativeError, match="pinn_set_coef_fields: coefficient fields are single-device; this context has a communicator"):
        eng.set_coef_fields(K)
    assert not eng.has_coef_fields
    assert same_bits(eng.loss_grad(), before) and eng.kernel_path() == 7
    eng.close()


# ---- 12. the script -------------------------------------------------------------------------------------------------------------------
LINE = re.compile(r"^(tf_epoch|nt_epoch) =\s+(\d+)\s+elapsed = \d\d:\d\d \(\+\d\d\.\d\)  loss = (\S+)  ")
END = re.compile(r"^Training finished \(epoch (\d+)\): duration = \d\d:\d\d  error = (\S+)  ")
SHORT_HP = {"N_0": 128, "N_w": 64, "N_f": 2048, "layers": layers_of(8), "seed": 1234,
            "tf_epochs": 10, "tf_lr": 0.003, "tf_b1": 0.9, "tf_eps": None,
            "nt_epochs": 10, "nt_lr": 0.8, "nt_ncorr": 50, "log_frequency": 5}


@pytest.mark.parametrize("medium,walls", [("graded_rod", "dirichlet"), ("shear_flow", "periodic"), ("graded_reaction", "dirichlet")])
def test_script_runs_and_its_first_logged_loss_is_the_restatements(tmp_path, medium, walls):
    """inf_cont_mms_var.py with a short hp as a child process: Logger lines in the existing format, a finite final error, the
    residual line, a result folder.  Its first logged loss is the restatement's on the same sets (rebuilt here from the same
    hp and seeds), fields, source and initial weights, to the four digits the log prints -- and not the loss of the medium's
    mean coefficients."""
    hp = dict(SHORT_HP, medium=medium, walls=walls)
    hp_file = tmp_path / "hp.json"
    hp_file.write_text(json.dumps(hp))
    env = dict(os.environ, MPLBACKEND="Agg")
    env.pop("PINN_NO_PLOT", None)
    res = subprocess.run([sys.executable, os.path.join(PKG, "1d-mms", "inf_cont_mms_var.py"), str(hp_file)],
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
    line = re.search(r"^Residual with the fields and the source: max \|N_K\[u\] - s\| = (\S+) over 2048 points \(%s, %s walls\)"
                     % (medium, walls), out, re.M)
    assert line and np.isfinite(float(line.group(1)))
    m = re.search(r"Saving results to directory\s+(\S+)", out)
    assert m and os.path.isfile(os.path.join(m.group(1), "hp.json")) and os.path.isfile(os.path.join(m.group(1), "weights.npy"))

    # the number behind the first line
    sys.path.insert(0, os.path.join(PKG, "1d-mms"))
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
    K = mu.medium_fields(X_f, medium)
    s = mu.source_var(X_f, K)
    pairs = wall[1:] if walls == "periodic" else (None, None)
    rob = wall[1:] if walls == "dirichlet" else ()
    lo, _, ex = adr_var_ref.var_loss_grad(w0, hp["layers"], lb, ub, X_f, X_u, u, pairs[0], pairs[1], K, s, *rob)
    K_mean = np.tile(K.mean(axis=0), (len(X_f), 1))
    l_mean = adr_var_ref.var_loss_grad(w0, hp["layers"], lb, ub, X_f, X_u, u, pairs[0], pairs[1], K_mean, s, *rob)[0]
    print("first loss: restatement %.17g (with the mean coefficients %.4e) printed %s" % (lo, l_mean, rows[0][2]))
    assert (ex["mse_w"] > 0) == (walls == "dirichlet") and (ex["mse_b"] > 0) == (walls == "periodic")
    assert "%.4e" % l_mean != "%.4e" % lo
    assert rows[0][2] == "%.4e" % lo
