"""GPU: every kernel family on domains other than x in [-1, 1], t from 0 (tests/helpers/boxes.py).

Every kernel takes the domain as lbx, lbt, sx, st and writes out its own copy of the first layer and of the derivative seeds.
The rest of the suite runs them where sx = 1 and lb_t = 0 (Burgers, adr, discrete time) or lb_t = 0 (Schrodinger), where a
dropped lb_t, a hard-wired lb_x = -1, sx once in u_xx and a Robin u_x without sx are the right numbers.  Here each family runs on
boxes A ... D (2-D) and [0.3, 2.1], [-4, -3.5] (1-D) against the references evaluated on the box, with the bounds the suite
already has: nothing here is looser than the test it borrows from, and tests/test_boxes_host.py shows that those bounds reject
each of the wrong maps.

  1. loss and gradient on every kernel path (default, 0 ... 8), both dtypes, boxes A ... D: the loss and whole-vector bounds of
     tests/test_gpu_fuzz.py and assert_entries with grad_entries.judge(..., lb, ub) and grad_entries.K.
     Box D in float32: coordinates near 100 over a width of 1 cost float32 7 bits before any kernel runs, so the fixed bounds
     (made for boxes at the 32 u floor) give way to the box's own yardstick: entries as everywhere, the loss within K x
     max(plain float32 error of the loss, 32 u).
  2. predict, residual_at, residual, error_l2 on k_fwd20d / k_fwd20f, k_forward and k_t16_fwd (NT 4 and 8), boxes A ... C, with
     the bounds of test_forward_only_evaluation_sweep.
  3. the adr family on paths 0 and 7 (float32: path 0), boxes A ... C: pairs, Robin points (robin_residual too), source, fields,
     adr_ide, fixed point weights, against adr_fuzz.restate_adr / adr_ide_ref / adr_pw_ref on the box, adr_fuzz's yardsticks.
  4. SA Burgers against sa_ref on box B; Ensemble and AdrEnsemble, K = 3, per-member sets, against the oracle on box C.
  5. the discrete-time models on both 1-D boxes, as test_shape_sweep_against_oracle judges them.
  6. lhs_collocation on A ... D, bit for bit; one rad_collocation draw on B, bit for bit.

What it found.  pinn_lhs_collocation was not the restatement's design off the old boxes: k_lhs_fill wrote lb + r * v with
__dadd_rn / __dmul_rn, which are inline + and * that hipcc contracts into one fma after inlining (v_fmac_f64 in the kernel's
code).  With lb_t = 0 and ub_x - lb_x = 2 the fma and the two roundings agree, so the Burgers tests saw nothing; on the
Schrodinger box tests/test_gpu_rad.py had met it and read the pool back from the device instead.  Fixed in
csrc/kernels_sampling.h (plain operators under "#pragma clang fp contract(off)", both kernels); the draws on x in [-1, 1], t
from 0 keep their bits.  In exact arithmetic the fused form moves 19 of 1000 x coordinates of the design on box A and 70 of
1000 on box B by one ulp, none on C and D (widths 0.5 and 1: r * v is exact).  Nothing else failed: the map is applied
correctly on every path.

Measured on an MI355X (profiles/boxes_measured.jsonl), largest ratio entry_dev / yardstick per family and dtype, with the K
it is held to; none is above K / 3, and K does not move:

  family dtype  K    largest ratio: path, shape, box, entry
  w20    f32    9    2.36  2, burgers 10x20 470 + 43, D, W4[5,10]
  w20    f64    8    1.85  1, burgers 10x20 470 + 43, B, W8[16,10]
  wide   f32    7    1.73  0, schrodinger 4x100 150 + 50 + 7 pairs, B, W1[1,60]
  wide   f64    6    0.91  8, schrodinger 4x100, C, W0[1,70]
  t16    f32    20   1.79  0, burgers 3x24 333 + 17, A, W1[18,23]
  t16    f64    20   2.00  4, burgers 10x20 470 + 43, C, W5[1,12]
  adr family: gradient 0.88 (f64, path 7), 1.09 (f32); f 0.77 / 1.18; r 0.20 / 0.19; loss 0.07 / 0.09
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import adr_fuzz as af  # noqa: E402
import adr_ide_ref  # noqa: E402
import adr_pw_ref  # noqa: E402
import boxes  # noqa: E402
import disc_cases  # noqa: E402
import grad_entries as ge  # noqa: E402
import rad_ref  # noqa: E402
import sa_ref  # noqa: E402
from test_gpu_adr import TOL as ADR_TOL  # noqa: E402
from test_gpu_disc import TOL as DISC_TOL  # noqa: E402
from test_gpu_fuzz import assert_entries, rel  # noqa: E402
from test_gpu_predict import _fwd_net, _fwd_oracle  # noqa: E402

pytestmark = pytest.mark.gpu

NU = 0.01 / np.pi
BOX_NAMES = sorted(boxes.BOXES)


def need_longdouble(dtype):
    if dtype == "f64" and not ge.longdouble_is_wider():
        pytest.skip("np.longdouble is no wider than float64 here")


# ---- 1. loss and gradient on every path -----------------------------------------------------------------------------------------
# (kind, W, H, n_f, n_u, n_b): between them every family -- k_fused20m / k_fused20 / k_fused20d (8x20, 4x20, 6x20), the tile loop
# (16 600 points: 260 tiles), the generic kernels (2x7, 10x20 in float64 on k_fused20), k_wide_* and k_t16_fused (the Schrodinger
# net), k_t16_* and their halves (3x24, 2x65).  Ragged counts; 449 and 513 points leave one live lane in the last tile.
SHAPES = [("burgers", 20, 8, 65, 40, 0), ("burgers", 20, 4, 16500, 100, 0), ("burgers_ide", 20, 6, 0, 449, 0),
          ("schrodinger", 100, 4, 150, 50, 7), ("burgers", 24, 3, 333, 17, 0), ("burgers_ide", 65, 2, 0, 300, 0),
          ("burgers", 7, 2, 700, 30, 0), ("burgers", 20, 10, 470, 43, 0)]


@functools.lru_cache(maxsize=None)
def shape_case(i, name):
    kind, W, H, n_f, n_u, n_b = SHAPES[i]
    lb, ub = boxes.BOXES[name]
    layers = [2] + [W] * H + [2 if kind == "schrodinger" else 1]
    w, sets = ge.make_case(kind, layers, n_f, n_u, n_b, (0.6, -4.5), np.random.RandomState(5000 + 10 * i + ord(name)), lb, ub)
    return layers, w, sets


@functools.lru_cache(maxsize=None)
def shape_judged(i, name, dtype):
    """the reference in the wider type, once per case (read-only arrays), and the plain error of the loss"""
    kind = SHAPES[i][0]
    lb, ub = boxes.BOXES[name]
    layers, w, sets = shape_case(i, name)
    judged = ge.judge(kind, w, layers, sets, dtype, lb, ub)
    plain_loss = float(ge.restate(kind, w, layers, lb, ub, sets, ge.DTYPES[dtype])[0])
    return judged, abs(plain_loss - judged[0]) / abs(judged[0])


def feed(eng, kind, sets):
    if kind == "burgers":
        eng.set_collocation(sets["X_f"]); eng.set_data(sets["X_u"], sets["u"]); eng.set_pde_params(sets["nu"])
    elif kind == "burgers_ide":
        eng.set_data(sets["X_u"], sets["u"])
    else:
        eng.set_collocation(sets["X_f"]); eng.set_data(sets["X0"], sets["uv0"]); eng.set_boundary(sets["X_lb"], sets["X_ub"])


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", BOX_NAMES)
@pytest.mark.parametrize("i", range(len(SHAPES)), ids=["%s-%dx%d-f%d-u%d" % (s[0], s[2], s[1], s[3], s[4]) for s in SHAPES])
def test_loss_and_gradient_on_every_path(i, name, dtype, record):
    import pinn_native
    need_longdouble(dtype)
    kind = SHAPES[i][0]
    lb, ub = boxes.BOXES[name]
    layers, w, sets = shape_case(i, name)
    judged, plain_loss = shape_judged(i, name, dtype)
    ref_loss, ref_grad = judged[0], judged[1]
    u = ge.unit_roundoff(ge.DTYPES[dtype])
    tl, tg = (1e-11, 1e-10) if dtype == "f64" else (2e-5, 5e-5)
    own_yardstick = name == "D" and dtype == "f32"
    eng = pinn_native.Engine(layers, lb, ub, pde=kind, dtype=dtype)
    try:
        feed(eng, kind, sets)
        default = eng.kernel_path()
        tried = []
        for path in (default, 0, 1, 2, 3, 4, 5, 6, 7, 8):
            if tried and path == default:
                continue
            try:
                eng.set_kernel_path(path)
            except pinn_native.PinnNativeError:
                continue
            tried.append(path)
            eng.set_weights(w)
            loss, grad, _ = eng.loss_grad()
            d_loss = abs(loss - ref_loss) / max(abs(ref_loss), 1e-3)
            record(box=name, shape=i, dtype=dtype, path=path, loss=d_loss, grad=rel(grad, ref_grad), yard_u=judged[3] / u)
            if own_yardstick:
                k = ge.K[(ge.family_of(path, layers, dtype), dtype)]
                assert abs(loss - ref_loss) <= k * max(plain_loss, ge.FLOOR_ULPS * u) * abs(ref_loss), (path, loss, ref_loss)
            else:
                assert d_loss <= tl, (path, loss, ref_loss)
                assert rel(grad, ref_grad) <= tg, (path, rel(grad, ref_grad))
            assert_entries(grad, judged, path, layers, dtype, record)
        assert default in tried and 0 in tried
    finally:
        eng.close()


# ---- 2. forward only --------------------------------------------------------------------------------------------------------------
# (kind, W, H, n): the forward kernel in the comment (engine.hip forward_chunk)
FWD = [("burgers", 20, 3, 777),            # k_fwd20d / k_fwd20f
       ("burgers", 20, 8, 1001),           # k_fwd20d / k_fwd20f
       ("burgers", 7, 2, 65),              # k_forward
       ("schrodinger", 23, 2, 513),        # k_forward, two outputs
       ("burgers", 24, 3, 1000),           # k_t16_fwd NT 4
       ("burgers_ide", 65, 2, 333)]        # k_t16_fwd NT 8


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", boxes.FLOAT32_BOXES)
@pytest.mark.parametrize("kind,W,H,n", FWD, ids=["%s-W%d-H%d-n%d" % c for c in FWD])
def test_forward_only_evaluation(kind, W, H, n, name, dtype, record):
    """bounds of test_forward_only_evaluation_sweep: values f64 1e-12 / f32 5e-6, residuals f64 1e-10 / f32 2e-4, relative to
    max(1, max|ref|); error_l2 1e-14 against numpy on the device's own prediction, 1e-13 for the modulus kind"""
    import pinn_native
    lb, ub = boxes.BOXES[name]
    rs = np.random.RandomState(100 * W + H + ord(name))
    layers, w = _fwd_net(kind, W, H, rs)
    nu = rs.uniform(0.001, 0.1)
    tol_u, tol_f = (1e-12, 1e-10) if dtype == "f64" else (5e-6, 2e-4)
    dev = lambda a, ref: np.max(np.abs(a - ref)) / max(1.0, np.max(np.abs(ref)))      # noqa: E731
    eng = pinn_native.Engine(layers, lb, ub, pde=kind, dtype=dtype)
    try:
        if kind == "burgers":
            eng.set_pde_params(nu)
        eng.set_weights(w)
        X = boxes.points(rs, n, lb, ub)
        u_ref, f_ref = _fwd_oracle(kind, layers, w, X, lb, ub, nu)
        u, f = eng.predict(X), eng.residual_at(X)
        if kind == "burgers_ide":
            eng.set_data(X, rs.standard_normal((n, 1)))
        else:
            if kind == "schrodinger":
                eng.set_boundary(*boxes.walls(rs, 5, lb, ub))
            eng.set_data(boxes.points(rs, 9, lb, ub), rs.standard_normal((9, layers[-1])))
            eng.set_collocation(X)
        d_u, d_f, d_fs = dev(u, u_ref), dev(f, f_ref), dev(eng.residual(), f_ref)
        ref = u_ref + 0.1 * rs.standard_normal(u_ref.shape)
        e, e_np = eng.error_l2(X, ref), np.linalg.norm(ref - u) / np.linalg.norm(ref)
        href = np.sqrt(np.sum(u_ref ** 2, axis=1)) + 0.1 * np.abs(rs.standard_normal(n))
        em = eng.error_l2(X, href, modulus=True)
        em_np = np.linalg.norm(href - np.sqrt(np.sum(u ** 2, axis=1))) / np.linalg.norm(href)
        record(box=name, kind=kind, W=W, H=H, dtype=dtype, value=d_u, residual=d_f, residual_stored=d_fs,
               err_l2=abs(e - e_np) / e_np, err_l2_modulus=abs(em - em_np) / em_np)
        assert u.shape == u_ref.shape and f.shape == f_ref.shape
        assert d_u <= tol_u and d_f <= tol_f and d_fs <= tol_f, (d_u, d_f, d_fs)
        assert abs(e - e_np) <= 1e-14 * e_np and abs(em - em_np) <= 1e-13 * em_np, (e, e_np, em, em_np)
    finally:
        eng.close()


# ---- 3. the adr family ------------------------------------------------------------------------------------------------------------
# name -> (depth, n_b, n_0, n_f, n_w, source, fields)
ADR = {"pairs": (4, 9, 40, 333, 0, False, False), "robin": (8, 3, 30, 449, 17, False, False),
       "source": (6, 0, 65, 500, 0, True, False), "fields-robin": (8, 5, 20, 300, 9, False, True),
       "ide": (6, 7, 50, 410, 0, False, False), "pw": (4, 6, 33, 700, 0, False, False)}
IDE_MASK = 0b101101
ADR_CONFIGS = [("f64", 0), ("f64", 7), ("f32", 0)]


@functools.lru_cache(maxsize=None)
def adr_case(case, name):
    depth, n_b, n_0, n_f, n_w, source, fields = ADR[case]
    lb, ub = boxes.BOXES[name]
    layers = af.layers_of(depth)
    rs = np.random.RandomState(6000 + 10 * sorted(ADR).index(case) + ord(name))
    x = boxes.adr_inputs(rs, layers, lb, ub, n_b, n_0, n_f, n_w, source, fields)
    if case == "ide":
        x["w"] = adr_ide_ref.pack(x["w"], boxes.ADR_COEFFS)
    if case == "pw":
        x["lam"] = tuple(rs.uniform(0.2, 3.0, n) for n in (n_0, n_f, n_b))
    return layers, x


def adr_restate(case, layers, x, lb, ub, dtype):
    """-> the dict of adr_fuzz.restate_adr, for every case but the point weights"""
    if case == "ide":
        lo, g, A, ex = adr_ide_ref.restate(x["w"], layers, lb, ub, x["X_f"], x["X_u"], x["u"], x["X_lo"], x["X_hi"], IDE_MASK, dtype)
        return {"loss": lo, "terms": (ex["mse_f"], ex["mse_u"], ex["mse_b"]), "grad": g, "A": A, "f": ex["f"],
                "A_f": af._ide_scale(layers, x["w"], x["X_f"], dtype, lb, ub), "r": np.zeros(0), "A_r": np.zeros(0)}
    return af.restate_adr(layers, x["w"], boxes.ADR_COEFFS, x["X_f"], x["X_u"], x["u"], x["X_lo"], x["X_hi"], x["robin"], x["s"],
                          x["K"], dtype, lb=lb, ub=ub)


@functools.lru_cache(maxsize=None)
def adr_reference(case, name, dtype):
    """-> (restatement in the wider type, yardsticks {quantity: max(plain error, 32 u)}): adr_fuzz.yardsticks on a box"""
    lb, ub = boxes.BOXES[name]
    layers, x = adr_case(case, name)
    ref = adr_restate(case, layers, x, lb, ub, ge.wider(ge.DTYPES[dtype]))
    plain = af.deviations(adr_restate(case, layers, x, lb, ub, ge.DTYPES[dtype]), ref)
    u = ge.unit_roundoff(ge.DTYPES[dtype])
    return ref, {q: max(plain[q], ge.FLOOR_ULPS * u) for q in af.QUANTITIES}


def adr_engine(case, layers, x, lb, ub, dtype, path):
    from pinn_native import Engine
    eng = Engine(layers, lb, ub, pde="adr_ide" if case == "ide" else "adr", dtype=dtype)
    eng.set_kernel_path(path)
    assert eng.kernel_path() == path
    eng.set_pde_params(*boxes.ADR_COEFFS)
    eng.set_collocation(x["X_f"]); eng.set_data(x["X_u"], x["u"]); eng.set_boundary(x["X_lo"], x["X_hi"])
    if case == "ide":
        eng.set_pde_trainable(IDE_MASK)
    else:
        eng.set_source(x["s"]); eng.set_coef_fields(x["K"])
        if x["robin"] is not None:
            eng.set_robin(*x["robin"])
    eng.set_weights(x["w"])
    if case == "pw":
        eng.pw_set(*x["lam"])
    return eng


@pytest.mark.parametrize("name", boxes.FLOAT32_BOXES)
@pytest.mark.parametrize("case", sorted(ADR))
def test_adr_family_on_paths_0_and_7(case, name, record):
    need_longdouble("f64")
    lb, ub = boxes.BOXES[name]
    layers, x = adr_case(case, name)
    n_f, n_w = ADR[case][3], ADR[case][4]
    for dtype, path in ([("f64", 7)] if case == "pw" else ADR_CONFIGS):
        eng = adr_engine(case, layers, x, lb, ub, dtype, path)
        try:
            loss, grad, terms = eng.loss_grad()
            f = eng.residual()
            r = eng.robin_residual() if case != "ide" else np.zeros(0)
        finally:
            eng.close()
        assert f.shape == (n_f, 1) and r.shape == (n_w,)
        if case == "pw":                         # adr_pw_ref is float64 only: TOL of tests/test_gpu_adr.py, as adr_fuzz does
            lo, go, tr, _ = adr_pw_ref.loss_grad(x["w"], layers, lb, ub, x["X_f"], x["X_u"], x["u"], x["X_lo"], x["X_hi"],
                                                 boxes.ADR_COEFFS, *x["lam"])
            fr = af.restate_adr(layers, x["w"], boxes.ADR_COEFFS, x["X_f"], lb=lb, ub=ub)["f"]
            d = {"loss": abs(loss - lo) / lo, "terms": max(abs(a - b) for a, b in zip(terms, tr)) / lo, "grad": rel(grad, go),
                 "f": rel(f, fr)}
            record(box=name, case=case, dtype=dtype, path=path, **d)
            tol = ADR_TOL[dtype]
            assert d["loss"] < tol["loss"] and d["terms"] < tol["loss"] * 10 and d["grad"] < tol["grad"] and d["f"] < tol["res"], d
            continue
        ref, yard = adr_reference(case, name, dtype)
        dev = af.deviations({"loss": loss, "grad": grad, "terms": tuple(terms), "f": f, "r": r}, ref)
        k = ge.K[(ge.family_of(path, layers, dtype), dtype)]
        ratio = {q: dev[q] / yard[q] for q in af.QUANTITIES}
        record(box=name, case=case, dtype=dtype, path=path, K=k, **{"ratio_" + q: ratio[q] for q in af.QUANTITIES})
        for q in af.QUANTITIES:
            assert dev[q] <= k * yard[q], "%s of %s on box %s (%s, path %d): %.2f x the yardstick, allowance %g" % (
                q, case, name, dtype, path, ratio[q], k)


# ---- 4. SA and ensembles ------------------------------------------------------------------------------------------------------------
def test_sa_burgers_with_random_weights_on_box_b(record):
    """bounds of tests/test_gpu_sa.py test_random_weights_match_the_restatement"""
    import pinn_native
    lb, ub = boxes.BOXES["B"]
    layers = [2] + [20] * 8 + [1]
    rs = np.random.RandomState(71)
    w, sets = ge.make_case("burgers", layers, 1345, 100, 0, None, rs, lb, ub)         # 1445 points: 22 tiles and 37 lanes
    lam_u, lam_f = rs.uniform(0.5, 2.0, 100), rs.uniform(0.5, 2.0, 1345)
    eng = pinn_native.Engine(layers, lb, ub, pde="burgers", dtype="f64")
    try:
        assert eng.kernel_path() == 7
        feed(eng, "burgers", sets)
        eng.set_weights(w)
        eng.sa_set_weights(lam_u, lam_f)
        loss, grad, terms = eng.loss_grad()
    finally:
        eng.close()
    lo, go, (mf, mu), _, _ = sa_ref.loss_grad(w, layers, lb, ub, sets["X_f"], sets["X_u"], sets["u"], NU, lam_u, lam_f)
    record(loss=abs(loss - lo) / lo, grad=rel(grad, go), mse_f=abs(terms[0] - mf) / mf, mse_u=abs(terms[1] - mu) / mu)
    assert abs(loss - lo) <= 1e-12 * lo and np.max(np.abs(grad - go)) <= 1e-11 * np.max(np.abs(go))
    assert abs(terms[0] - mf) <= 1e-12 * mf and abs(terms[1] - mu) <= 1e-12 * mu


def test_burgers_ensemble_against_the_oracle_on_box_c(record):
    """K = 3, a point set, data and viscosity per member; float64 bounds of tests/test_gpu_fuzz.py and the entries.  (That an
    ensemble member equals a solo engine, tests/test_gpu_ensemble_sets.py, cannot see a map error the two share.)"""
    import pinn_native
    from oracle import pde
    need_longdouble("f64")
    lb, ub = boxes.BOXES["C"]
    layers = [2] + [20] * 6 + [1]
    cases = [ge.make_case("burgers", layers, 500, 61, 0, None, np.random.RandomState(80 + k), lb, ub) for k in range(3)]
    nus = [NU * (1.0 + 0.5 * k) for k in range(3)]
    ens = pinn_native.Ensemble(layers, lb, ub, 3, pde="burgers")
    try:
        ens.set_collocation(np.stack([s["X_f"] for _, s in cases]))
        ens.set_data(np.stack([s["X_u"] for _, s in cases]), np.stack([s["u"] for _, s in cases]))
        ens.set_pde_params(np.array(nus))
        ens.set_weights(np.stack([w for w, _ in cases]))
        losses, grads, _ = ens.loss_grad()
    finally:
        ens.close()
    for k, (w, s) in enumerate(cases):
        s = dict(s, nu=nus[k])
        lo, go, _ = pde.burgers_loss_grad(w, layers, lb, ub, s["X_f"], s["X_u"], s["u"], nus[k])
        assert abs(losses[k] - lo) <= 1e-11 * max(abs(lo), 1e-3) and rel(grads[k], go) <= 1e-10, k
        assert_entries(grads[k], ge.judge("burgers", w, layers, s, "f64", lb, ub), 7, layers, "f64", record)


def test_adr_ensemble_against_the_restatement_on_box_c(record):
    """K = 3, own sets, pairs and coefficients; adr_fuzz's rule: every quantity within K x max(plain error, 32 u)"""
    from pinn_native import AdrEnsemble
    need_longdouble("f64")
    lb, ub = boxes.BOXES["C"]
    layers = af.layers_of(8)
    rs = np.random.RandomState(90)
    xs = [boxes.adr_inputs(rs, layers, lb, ub, 9, 61, 300) for _ in range(3)]
    coeffs = [[c * (1.0 + 0.3 * k) for c in boxes.ADR_COEFFS] for k in range(3)]
    ens = AdrEnsemble(layers, lb, ub, 3)
    try:
        ens.set_collocation(np.stack([x["X_f"] for x in xs]))
        ens.set_data(np.stack([x["X_u"] for x in xs]), np.stack([x["u"] for x in xs]))
        ens.set_boundary(np.stack([x["X_lo"] for x in xs]), np.stack([x["X_hi"] for x in xs]))
        ens.set_pde_params(np.asarray(coeffs))
        ens.set_weights(np.stack([x["w"] for x in xs]))
        losses, grads, terms = ens.loss_grad()
    finally:
        ens.close()
    u = ge.unit_roundoff(np.float64)
    k_allow = ge.K[("w20", "f64")]
    for k, x in enumerate(xs):
        run = lambda dt: af.restate_adr(layers, x["w"], coeffs[k], x["X_f"], x["X_u"], x["u"], x["X_lo"], x["X_hi"], dtype=dt,      # noqa: E731
                                        lb=lb, ub=ub)
        ref, plain = run(np.longdouble), run(np.float64)
        got = {"loss": losses[k], "grad": grads[k], "terms": tuple(terms[k]), "f": plain["f"], "r": np.zeros(0)}      # f: no ensemble call
        dev, pl = af.deviations(got, ref), af.deviations(plain, ref)
        for q in ("grad", "loss"):
            yard = max(pl[q], ge.FLOOR_ULPS * u)
            record(member=k, quantity=q, ratio=dev[q] / yard, K=k_allow)
            assert dev[q] <= k_allow * yard, (k, q, dev[q] / yard)


# ---- 5. discrete time -----------------------------------------------------------------------------------------------------------------
# (model, dtype, layers, q, n0, n1): ragged sets; width 100 is the NT = 8 instantiation (float32 only)
DISC = [("burgers_disc", "f64", [1, 32, 32, 21], 20, 37, 21), ("burgers_disc", "f32", [1, 32, 32, 21], 20, 37, 21),
        ("burgers_disc", "f32", [1, 100, 100, 21], 20, 33, 17),
        ("burgers_disc_ide", "f64", [1, 24, 24, 24, 30], 30, 41, 19), ("burgers_disc_ide", "f32", [1, 24, 24, 24, 30], 30, 41, 19)]


@pytest.mark.parametrize("name", sorted(boxes.BOXES_1D))
@pytest.mark.parametrize("model,dtype,layers,q,n0,n1", DISC, ids=[disc_cases.case_id(c + (0,)) for c in DISC])
def test_discrete_time_models_on_1d_boxes(model, dtype, layers, q, n0, n1, name, record):
    """loss_grad, predict and disc_predict of both sets against oracle/disc.py on the box: TOL of tests/test_gpu_disc.py, the
    lambda bound and the value bounds of test_shape_sweep_against_oracle (values f64 1e-12 / f32 5e-6, stage predictions f64
    1e-10 / f32 1e-3, relative to max(1, max|ref|))"""
    import pinn_native
    from oracle import disc, mlp
    assert disc_cases.accepted(model, dtype, layers, q, n0, n1)
    lb, ub = boxes.BOXES_1D[name]
    identify = model == "burgers_disc_ide"
    sets, w, nu = disc_cases.build(model, layers, q, n0, n1, 300 + q + ord(name), lb[0], ub[0])
    tl, tg = DISC_TOL[dtype]
    tag = "%s-%s" % (disc_cases.case_id((model, dtype, layers, q, n0, n1, 0)), name)
    eng = pinn_native.Engine(layers, lb, ub, pde=model, dtype=dtype)
    try:
        for s, (x, t, M) in enumerate(sets):
            eng.disc_set_stage(s, x, t, M)
        if not identify:
            eng.set_pde_params(nu)
        eng.set_weights(w)
        loss, grad, terms = eng.loss_grad()
        lo, go, ex = disc.disc_loss_grad(w, layers, lb, ub, sets, nu=nu, identify=identify)
        d_loss, d_grad = abs(loss - lo) / abs(lo), rel(grad, go)
        d_terms = max(abs(terms[0] - ex["sse"][0]), abs(terms[1] - ex["sse"][1])) / abs(lo)
        d_lam = (np.max(np.abs(grad[-2:] - go[-2:])) / np.max(np.abs(go[-2:]))) if identify else 0.0
        record(case=tag, loss=d_loss, grad=d_grad, terms=d_terms, lam=d_lam)
        assert d_loss <= tl and d_grad <= tg and d_terms <= tl, (d_loss, d_grad, d_terms)
        if identify:
            assert d_lam <= (1e-9 if dtype == "f64" else 5e-3), d_lam
        params = mlp.unpack(w[:-2] if identify else w, layers)
        c1, c2 = (w[-2], np.exp(w[-1])) if identify else (1.0, nu)
        rs = np.random.RandomState(q)
        xs = np.sort(boxes.points_1d(rs, 37, lb, ub), axis=0)
        U, ref = eng.predict(xs), mlp.forward_value(params, xs, lb, ub)
        d_val = np.max(np.abs(U - ref)) / max(1.0, np.max(np.abs(ref)))
        assert U.shape == ref.shape and d_val <= (1e-12 if dtype == "f64" else 5e-6), d_val
        xs = boxes.points_1d(rs, 53, lb, ub)
        d_st = []
        for s, (_, _, M) in enumerate(sets):
            P = eng.disc_predict(s, xs[:, 0])
            pred = disc.stage_prediction(params, xs, lb, ub, M, c1, c2)[0]
            d_st.append(np.max(np.abs(P - pred)) / max(1.0, np.max(np.abs(pred))))
            assert d_st[-1] <= (1e-10 if dtype == "f64" else 1e-3), (s, d_st[-1])
        record(case=tag, value=d_val, stage0=d_st[0], stage1=d_st[1])
    finally:
        eng.close()


# ---- 6. sampling ------------------------------------------------------------------------------------------------------------------------
def lhs_engine(lb, ub, dtype):
    import pinn_native
    return pinn_native.Engine([2, 20, 20, 20, 20, 1], lb, ub, pde="burgers", dtype=dtype)


@pytest.mark.parametrize("n", [1, 1000, 4097])
@pytest.mark.parametrize("name", BOX_NAMES)
def test_device_lhs_is_the_restatement_on_every_box(name, n):
    """bit for bit in float64, the exact float32 rounding in float32, one point per stratum inside the box (the fix of
    k_lhs_fill in this file's docstring is what this test is for)"""
    from oracle import lhs
    lb, ub = boxes.BOXES[name]
    seed = 0x1234ABCD5678 + n
    ref, (p0, p1) = lhs.lhs_points(n, seed, lb, ub)
    assert np.array_equal(np.sort(p0), np.arange(n, dtype=np.uint64)) and np.array_equal(np.sort(p1), np.arange(n, dtype=np.uint64))
    for dtype in ("f64", "f32"):
        eng = lhs_engine(lb, ub, dtype)
        try:
            eng.lhs_collocation(n, seed=seed)
            X = eng.get_collocation()
        finally:
            eng.close()
        want = ref if dtype == "f64" else ref.astype(np.float32).astype(np.float64)
        assert np.array_equal(X, want), (dtype, int(np.sum(X != want)))
        if dtype == "f64":
            assert np.all(X >= lb) and np.all(X <= ub)
            for d in range(2):
                strata = np.floor((X[:, d] - lb[d]) / (ub[d] - lb[d]) * n).astype(np.int64)
                assert np.array_equal(np.sort(np.clip(strata, 0, n - 1)), np.arange(n))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_rad_draw_on_box_b_is_the_restatement(dtype):
    """one draw, bit for bit against rad_ref fed with residual_at at the oracle's pool -- which, on this box, is the device's
    pool only since k_lhs_fill rounds every operation"""
    lb, ub = boxes.BOXES["B"]
    layers = [2] + [20] * 8 + [1]
    rs = np.random.RandomState(3)
    w, sets = ge.make_case("burgers", layers, 700, 100, 0, None, rs, lb, ub)
    import pinn_native
    eng = pinn_native.Engine(layers, lb, ub, pde="burgers", dtype=dtype)
    try:
        feed(eng, "burgers", sets)
        eng.set_weights(w)
        n_pool, seed = 5003, 0x5EED0B0B
        eng.lhs_collocation(n_pool, seed)
        P = eng.get_collocation()
        assert np.array_equal(P, rad_ref.pool_points(n_pool, seed, lb, ub, dtype))
        f = eng.residual_at(P)
        eng.rad_collocation(1000, seed, n_pool, k=2, c=0.5)
        got = eng.get_collocation()
    finally:
        eng.close()
    want, idx = rad_ref.rad_draw(P, f, seed, 0, 1000, 2, 0.5)
    assert got.shape == (1000, 2) and np.array_equal(got, want), int(np.sum(np.any(got != want, axis=1)))
    assert len(np.unique(idx)) > 1
