"""Host: the comparators of tests/test_gpu_boxes.py see the domain map.

Every kernel family writes out its own copy of the first layer, h = s (X - lb) - 1, and of the derivative seeds h_x = sx,
h_t = st.  On [-1, 1] x [0, 1] four ways of getting that wrong compute the right numbers (asserted below: that is why the
boxes of tests/helpers/boxes.py exist).  Here, for each box and each kind, wrong gradients are built with the restatements
themselves and the bound the GPU test asserts -- K x max(plain error, 32 u), K unchanged -- has to reject every one:

  a  lb_t taken as 0                         d  sx and st exchanged
  b  lb_x taken as -1                        e  the Robin term beta u_x without sx (adr)
  c  u_xx carrying sx once                   f  one pad slot, a point at (lb_x, lb_t), counted as a collocation point

a, b and d are the right map of another box (boxes.lbt_as_zero ...); c is grad_entries.restate(uxx_scale = 1 / sx), for the adr
kind nu / sx; e is beta / sx; f is one more row with the denominator kept.  The mutants are computed in float64 for both
dtypes: they stand orders of magnitude above a bound of a few hundred u, so their own rounding does not matter.  K: the
largest allowance any kernel path has on any shape (grad_entries.K: 20), so the margins printed hold for every path.

The 1-D boxes: oracle/disc.py with the max-norm bounds of tests/test_gpu_disc.py (TOL; float32, the loosest).  A k_disc_fwd
whose first layer seeds zp = w0 instead of w0 sx is the oracle on [-1, 1] at the mapped points.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import adr_fuzz as af  # noqa: E402
import boxes  # noqa: E402
import disc_cases  # noqa: E402
import grad_entries as ge  # noqa: E402

K_MAX = {d: max(k for (_, dd), k in ge.K.items() if dd == d) for d in ("f32", "f64")}
KINDS = ("burgers", "burgers_ide", "schrodinger", "adr")
ALL_BOXES = dict(boxes.BOXES, NARROW=boxes.NARROW, OLD=boxes.OLD)
INVISIBLE_ON_OLD = ("a", "b", "c", "e")
ADR_LAYERS = [2, 20, 20, 20, 20, 1]


def need_longdouble(dtype):
    if dtype == "f64" and not ge.longdouble_is_wider():
        pytest.skip("np.longdouble is no wider than float64 on this host: plain float64 has nothing to be judged against")


def case_of(kind, lb, ub):
    """-> (layers, w, sets) of grad_entries' kinds: Burgers 4x20 on 300 + 40 points, identification on 300, the Schrodinger
    net 4x100 on 150 + 30 points and 7 pairs"""
    rs = np.random.RandomState(4242)
    if kind == "burgers":
        layers, n = [2, 20, 20, 20, 20, 1], (300, 40, 0)
    elif kind == "burgers_ide":
        layers, n = [2, 20, 20, 20, 20, 1], (0, 300, 0)
    else:
        layers, n = [2, 100, 100, 100, 100, 2], (150, 30, 7)
    w, sets = ge.make_case(kind, layers, n[0], n[1], n[2], (0.6, -4.5), rs, lb, ub)
    return layers, w, sets


def with_pad_point(kind, sets, lb):
    pad = np.array([[lb[0], lb[1]]])
    s = dict(sets)
    if kind == "burgers_ide":
        s["n_u"] = sets["X_u"].shape[0]
        s["X_u"], s["u"] = np.vstack([sets["X_u"], pad]), np.vstack([sets["u"], np.zeros((1, 1))])
    else:
        s["n_f"] = sets["X_f"].shape[0]
        s["X_f"] = np.vstack([sets["X_f"], pad])
    return s


def mutants_of(kind, layers, w, sets, lb, ub):
    """-> {name: wrong gradient (float64)}"""
    run = lambda lb_, ub_, s=sets, **kw: np.asarray(ge.restate(kind, w, layers, lb_, ub_, s, np.float64, **kw)[1])      # noqa: E731
    return {"a": run(*boxes.lbt_as_zero(lb, ub)), "b": run(*boxes.lbx_as_minus_one(lb, ub)),
            "c": run(lb, ub, uxx_scale=1.0 / boxes.scales(lb, ub)[0]), "d": run(*boxes.scales_swapped(lb, ub)),
            "f": run(lb, ub, with_pad_point(kind, sets, lb))}


def adr_run(x, lb, ub, dtype=np.float64, coeffs=boxes.ADR_COEFFS, **kw):
    y = dict(x, **{k: v for k, v in kw.items() if k in x})
    tot = {k: v for k, v in kw.items() if k not in x}
    return af.restate_adr(ADR_LAYERS, y["w"], coeffs, y["X_f"], y["X_u"], y["u"], y["X_lo"], y["X_hi"], y["robin"], y["s"], y["K"],
                          dtype, lb=lb, ub=ub, **tot)


def adr_case(lb, ub):
    """the adr kind with pairs, data, a source and Robin points: 4x20, 300 + 40 points, 5 pairs, 9 Robin points"""
    return boxes.adr_inputs(np.random.RandomState(4243), ADR_LAYERS, lb, ub, 5, 40, 300, n_w=9, source=True)


def adr_mutants(x, lb, ub):
    sx = boxes.scales(lb, ub)[0]
    c = list(boxes.ADR_COEFFS)
    c[2] /= sx
    X_w, al, be, g = x["robin"]
    pad = np.array([[lb[0], lb[1]]])
    out = {"a": adr_run(x, *boxes.lbt_as_zero(lb, ub)), "b": adr_run(x, *boxes.lbx_as_minus_one(lb, ub)),
           "c": adr_run(x, lb, ub, coeffs=c), "d": adr_run(x, *boxes.scales_swapped(lb, ub)),
           "e": adr_run(x, lb, ub, robin=(X_w, al, be / sx, g)),
           "f": adr_run(x, lb, ub, X_f=np.vstack([x["X_f"], pad]), s=np.append(x["s"], 0.0), n_f_total=len(x["X_f"]))}
    return {k: np.asarray(v["grad"]) for k, v in out.items()}


def judged(kind, name, dtype):
    """-> (reference gradient, A, yardstick, layout, mutants, the plain float64 gradient)"""
    lb, ub = ALL_BOXES[name]
    if kind == "adr":
        x = adr_case(lb, ub)
        wide = ge.wider(ge.DTYPES[dtype])
        ref, plain = adr_run(x, lb, ub, wide), adr_run(x, lb, ub, ge.DTYPES[dtype])
        layout = ge.blocks(ADR_LAYERS, "adr")
        yard = max(af._scaled(plain["grad"], ref["grad"], ref["A"]), ge.FLOOR_ULPS * ge.unit_roundoff(ge.DTYPES[dtype]))
        return (np.asarray(ref["grad"], dtype=np.float64), ref["A"], yard, layout, adr_mutants(x, lb, ub),
                np.asarray(adr_run(x, lb, ub)["grad"]))
    layers, w, sets = case_of(kind, lb, ub)
    _, g_ref, A, yard, layout = ge.judge(kind, w, layers, sets, dtype, lb, ub)
    return g_ref, A, yard, layout, mutants_of(kind, layers, w, sets, lb, ub), np.asarray(
        ge.restate(kind, w, layers, lb, ub, sets, np.float64)[1])


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["A", "B", "C", "D", "NARROW"])
def test_every_wrong_map_is_above_the_bound(name, kind, dtype):
    """the margins (mutant deviation / bound) are printed; the smallest per box and dtype is above 1.  NARROW is float64 only:
    its float32 yardstick is measured and printed, nothing is judged by it"""
    need_longdouble(dtype)
    g_ref, A, yard, layout, muts, _ = judged(kind, name, dtype)
    u = ge.unit_roundoff(ge.DTYPES[dtype])
    print("box %s %s %s: yardstick %.0f u" % (name, kind, dtype, yard / u))
    if name == "NARROW" and dtype == "f32":
        assert yard > 1000 * u                       # coordinates near 1000 over a width of 0.01: no float32 case
        return
    if name in boxes.FLOAT32_BOXES or dtype == "f64":
        assert yard <= 2 * ge.FLOOR_ULPS * u, yard / u                # at (or next to) the floor
    bound = K_MAX[dtype] * yard
    assert set(muts) == set("abcdf") | ({"e"} if kind == "adr" else set())
    margins = {}
    for m, g in sorted(muts.items()):
        dev, block, rc = ge.entry_dev(g, g_ref, A, layout)
        margins[m] = dev / bound
        if m == "d" and name in boxes.EQUAL_SCALES:
            assert dev <= bound                      # sx == st on this box: nothing to exchange (boxes.EQUAL_SCALES)
            del margins[m]
            continue
        assert dev > bound, "box %s %s %s: mutant %s (worst at %s%s, %.3e of its scale) passes the bound %.3e" % (
            name, kind, dtype, m, block, rc, dev, bound)
    print("box %s %s %s: margins %s; smallest %.1f" % (name, kind, dtype, " ".join("%s %.3g" % kv for kv in sorted(margins.items())),
                                                      min(margins.values())))


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("kind", KINDS)
def test_on_the_old_box_four_of_them_are_the_right_gradient(kind, dtype):
    """the recorded reason for the boxes: on [-1, 1] x [0, 1] a dropped lb_t, lb_x = -1, sx once in u_xx and beta u_x without
    sx give the restatement's gradient bit for bit, so no bound can reject them; exchanged scales and a counted pad point are
    seen there too"""
    need_longdouble(dtype)
    g_ref, A, yard, layout, muts, plain64 = judged(kind, "OLD", dtype)
    bound = K_MAX[dtype] * yard
    for m in INVISIBLE_ON_OLD:
        if m in muts:
            assert np.array_equal(muts[m], plain64), m
            assert ge.entry_dev(muts[m], g_ref, A, layout)[0] <= bound, m
    for m in ("d", "f"):
        assert ge.entry_dev(muts[m], g_ref, A, layout)[0] > bound, m


def test_float32_yardsticks_of_the_offset_boxes():
    """what INTEGRATION.md section 4 quotes (Burgers 4x20, 300 + 40 points, plain float32 against float64, in u = 2^-24 of an
    entry's scale): A, B and C below the floor of 32 u, D above them (36 u on this draw, 43 u on the Schrodinger case above;
    the figure moves with the draw: up to about 110 u), NARROW about 10 000 u"""
    u = ge.unit_roundoff(np.float32)
    got = {}
    for name, (lb, ub) in sorted(ALL_BOXES.items()):
        layers, w, sets = case_of("burgers", lb, ub)
        _, g, _ = ge.restate("burgers", w, layers, lb, ub, sets, np.float32)
        _, gw, A = ge.restate("burgers", w, layers, lb, ub, sets, np.float64)
        got[name] = ge.dev_against_wide(g, gw, A, ge.blocks(layers, "burgers"))[0] / u
    print("plain float32 error in u: " + " ".join("%s %.0f" % kv for kv in sorted(got.items())))
    assert all(got[k] <= 2 * ge.FLOOR_ULPS for k in ("A", "B", "C", "OLD"))
    assert max(got[k] for k in ("A", "B", "C", "OLD")) < got["D"] < 400
    assert got["NARROW"] > 1000


# ---- the 1-D boxes ------------------------------------------------------------------------------------------------------------
# tests/test_gpu_disc.py: TOL (loss, gradient by its largest entry) and the stage-prediction bound
DISC_TOL = {"f64": (1e-12, 1e-11, 1e-10), "f32": (2e-5, 2e-4, 1e-3)}
DISC = [("burgers_disc", [1, 32, 32, 21], 20, 37, 20), ("burgers_disc_ide", [1, 24, 24, 24, 30], 30, 33, 15)]


def rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300)


def disc_eval(model, layers, w, nu, sets, lb, ub, xs):
    from oracle import disc, mlp
    ide = model == "burgers_disc_ide"
    lo, go, _ = disc.disc_loss_grad(w, layers, lb, ub, sets, nu=nu, identify=ide)
    c1, c2 = (w[-2], np.exp(w[-1])) if ide else (1.0, nu)
    st = disc.stage_prediction(mlp.unpack(w[:-2] if ide else w, layers), xs, lb, ub, sets[0][2], c1, c2)[0]
    return lo, go, st


def disc_mutants(model, layers, w, nu, sets, lb, ub, xs):
    """-> {name: (loss, gradient, stage prediction of set 0)} of
      seed  zp = w0 in the first layer (u_x short of sx, u_xx of sx^2): the oracle on [-1, 1] at the mapped points
      b     lb_x taken as -1
      c     u_xx carrying sx once: nu / sx (identification: lambda_2 - log sx)"""
    sx = 2.0 / (ub[0] - lb[0])
    xi = lambda x: sx * (x - lb[0]) - 1.0      # noqa: E731
    mapped = [(xi(x), t, M) for x, t, M in sets]
    one = (np.array([-1.0]), np.array([1.0]))
    w_c, nu_c = w, nu
    if model == "burgers_disc_ide":
        w_c = w.copy()
        w_c[-1] -= np.log(sx)
    else:
        nu_c = nu / sx
    return {"seed": disc_eval(model, layers, w, nu, mapped, one[0], one[1], xi(xs)),
            "b": disc_eval(model, layers, w, nu, sets, np.array([-1.0]), np.array([-1.0 + (ub[0] - lb[0])]), xs),
            "c": disc_eval(model, layers, w_c, nu_c, sets, lb, ub, xs)}


@pytest.mark.parametrize("model,layers,q,n0,n1", DISC, ids=["inf", "ide"])
@pytest.mark.parametrize("name", ["p", "n", "old"])
def test_discrete_time_bounds_see_the_map(name, model, layers, q, n0, n1):
    """the unseeded first layer (zp = w0) and lb_x = -1 exceed float32 TOL, the loosest, on the loss and on the gradient.  u_xx with sx once is another matter: it enters through nu u_xx with nu = 0.001 ... 0.1 (or
    e^lambda_2, lambda_2 in (-7, -4)), and on [0.3, 2.1], where sx is 1.11, it moves the identification gradient by 2e-5 of
    its largest entry: max-norm float32 bounds cannot see it.  The float64 bounds do, by six orders of magnitude and more,
    and every discrete-time case of tests/test_gpu_boxes.py but the width-100 one runs in float64 too."""
    lb, ub = boxes.BOXES_1D[name] if name != "old" else (np.array([-1.0]), np.array([1.0]))
    sets, w, nu = disc_cases.build(model, layers, q, n0, n1, 77, lb[0], ub[0])
    xs = boxes.points_1d(np.random.RandomState(78), 53, lb, ub)
    lo, go, st = disc_eval(model, layers, w, nu, sets, lb, ub, xs)
    for m, (lm, gm, sm) in sorted(disc_mutants(model, layers, w, nu, sets, lb, ub, xs).items()):
        dev = (abs(lm - lo) / abs(lo), rel(gm, go), np.max(np.abs(sm - st)) / max(1.0, np.max(np.abs(st))))
        margin = {d: [x / t for x, t in zip(dev, DISC_TOL[d])] for d in DISC_TOL}
        print("1-D box %s %s mutant %s: loss, gradient, stage over their bounds: float32 %s, float64 %s" % (
            name, model, m, " ".join("%.3g" % v for v in margin["f32"]), " ".join("%.3g" % v for v in margin["f64"])))
        if name == "old":                            # sx = 1, lb_x = -1: the same numbers (to the rounding of the mapping)
            assert max(dev) <= 1e-13, m
            continue
        assert min(margin["f64"]) > 1, (m, margin["f64"])
        if m != "c":
            assert min(margin["f32"][:2]) > 1, (m, margin["f32"])      # TOL; the float32 stage bound, 1e-3, is met at 0.92 once
