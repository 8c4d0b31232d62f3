"""Host: the tanh range probe of tests/helpers/tanh_probe.py checked on its own -- the probe net really returns tanh(c x)
(oracle/mlp.py in float64, the gradient test's restatement in float32), the grid and the products c x_k are exact, the
numpy restatements of the three tanh forms meet the bounds derived for them, and the assertions that
tests/test_gpu_tanh_range.py makes on the kernels reject a wrong tanh: an exponential with a seam, a clamp in the tail, a
result above 1, a lost sign."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import grad_entries as ge  # noqa: E402
import tanh_probe as tp  # noqa: E402

needs_longdouble = pytest.mark.skipif(not tp.longdouble_is_wider(),
                                      reason="np.longdouble is no wider than float64 on this host: no reference")


def test_the_scales_are_the_listed_ones():
    assert len(tp.K_GRID) == 4097 == 64 * 64 + 1 and tp.K_GRID[tp.N_GRID] == 0
    for d, top in (("f64", 1023), ("f32", 127)):
        sc = tp.scales(d)
        assert sorted({e for _, e in sc}) == sorted(tp.EXPONENTS[d])
        assert [m for m, e in sc if e == top] == [1] and all([m for m, e in sc if e == x] == [1, 3, 5]
                                                             for x in tp.EXPONENTS[d] if x != top)
        assert all(np.isfinite(tp.DTYPES[d](tp.scale_value(m, e))) and tp.DTYPES[d](tp.scale_value(m, e)) > 0 for m, e in sc)
        rs = tp.residual_scales(d)
        assert {e for _, e in rs} == {e for e in tp.EXPONENTS[d] if e <= 9} and set(rs) <= set(sc)
    assert tp.EXPONENTS["f64"] == (-1060, -600, -60, -30, -12, -3, 0, 2, 4, 5, 6, 9, 600, 1023)
    assert tp.EXPONENTS["f32"] == (-140, -100, -30, -12, -3, 0, 2, 4, 5, 6, 100, 127)
    assert set(tp.FORM) == {(W, d) for W in (20, 7, 24, 65) for d in ("f32", "f64")}


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_grid_and_products_are_exact(dtype):
    """(x + 1) - 1 == x and c x_k without rounding, in the type, against rational arithmetic; the one exception is float32
    at e = -140, whose products lie below the subnormal spacing: there z is within 2^-150 of c x_k"""
    dt = tp.DTYPES[dtype]
    X = tp.points()
    assert X.shape == (4097, 2) and np.all(X[:, 1] == 0.5)
    x = X[:, 0].astype(dt)
    assert np.array_equal(x.astype(np.float64), X[:, 0]) and np.array_equal((x + dt(1)) - dt(1), x)
    assert [Fraction(float(v)) for v in x[::257]] == [Fraction(int(k), 2048) for k in tp.K_GRID[::257]]
    tiny = Fraction(float(np.finfo(dt).smallest_subnormal))
    inexact = []
    for m, e in tp.scales(dtype):
        z = tp.preactivation(m, e, dtype)
        assert z.dtype == dt and np.all(np.isfinite(z))
        c = Fraction(m) * Fraction(2) ** e
        assert Fraction(float(dt(tp.scale_value(m, e)))) == c
        want = [c * Fraction(int(k), 2048) for k in tp.K_GRID[::97]]
        got = [Fraction(float(v)) for v in z[::97]]
        if Fraction(2) ** e / 2048 >= tiny:                          # the grid step times the power of two in c
            assert got == want, (m, e)
        else:
            inexact.append(e)
            assert max(abs(g - w) for g, w in zip(got, want)) <= tiny / 2
        if tp.longdouble_is_wider():
            assert [Fraction(*map(int, float(v).as_integer_ratio())) for v in tp.exact_preactivation(m, e)[::97]
                    if np.isfinite(float(v)) and (v == 0 or abs(float(v)) >= 1e-300)] == \
                   [w for w in want if w == 0 or abs(w) >= Fraction(1, 10 ** 300)]
    assert set(inexact) == ({-140} if dtype == "f32" else set())


def test_probe_net_is_tanh_cx_through_the_oracle_in_float64():
    from oracle import mlp
    X = tp.points()
    for W in tp.WIDTHS:
        layers = [2, W, 1]
        for m, e in ((1, -3), (3, 0), (5, 2), (1, 5), (1, 600)):
            w = tp.weights(W, tp.scale_value(m, e), seed=W)
            assert w.size == 2 * W + W + W + 1 and w[0] == tp.scale_value(m, e) and np.all(w[1:W] != 0)
            u = mlp.forward_value(mlp.unpack(w, layers), X, tp.LB, tp.UB)
            assert np.array_equal(u.ravel(), np.tanh(tp.preactivation(m, e, "f64")))


def test_probe_net_is_tanh_cx_through_the_restatement_in_float32():
    """the gradient test's float32 sweep on the probe net: the value channel is tanhf(c x), bit for bit, and so is the
    residual's closed form to float32 rounding"""
    X = tp.points()
    for W, (m, e) in zip(tp.WIDTHS, ((1, -3), (3, 0), (5, 2), (1, 5))):
        w = tp.weights(W, tp.scale_value(m, e), seed=W)
        params = ge._unpack(w, [2, W, 1], np.float32)
        s = (2 / (tp.UB - tp.LB)).astype(np.float32)
        (h, p, q, r), _ = ge._forward(params, X.astype(np.float32), tp.LB.astype(np.float32), s, False)
        a = np.tanh(tp.preactivation(m, e, "f32"))
        assert h.dtype == np.float32 and np.array_equal(h.ravel(), a) and not np.any(q)
        f = (q + h * p - np.float32(tp.NU) * r).ravel()
        want = tp.formula_residual("lib", m, e, "f32")
        assert np.max(np.abs(f - want)) <= 8 * tp.unit_roundoff("f32") * np.max(np.abs(want))


@needs_longdouble
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("form", ["q", "r5", "lib"])
def test_numpy_restatements_meet_their_derived_bounds(form, dtype):
    """the worst absolute error of each form over every scale, against longdouble, within the bound derived in the
    helper's docstring; the device is allowed 4 x the worst error measured here.  The two hand-written forms also pass
    every other assertion of the probe (finite, |a| <= 1, +-1 past saturation, oddness), and the residual's closed form
    in the type stays within its propagated bound."""
    worst, z = tp.host_error(form, dtype)
    print("%s %s: worst %.3f u at z = %r; derived bound %.0f u, device bound %.2f u" % (
        form, dtype, worst, z, tp.HOST_BOUND_U[form], tp.device_bound_u(form, dtype)))
    assert 0.25 <= worst <= tp.HOST_BOUND_U[form]
    assert tp.device_bound_u(form, dtype) == 4 * worst
    for m, e in tp.scales(dtype):
        a = tp.formula(form, tp.preactivation(m, e, dtype))
        assert a.dtype == tp.DTYPES[dtype]
        if form != "lib":
            out = tp.check_values(a, m, e, dtype, form, tp.HOST_BOUND_U[form])
            assert out["worst_u"] <= worst
    for m, e in tp.residual_scales(dtype):
        assert tp.check_residual(tp.formula_residual(form, m, e, dtype), m, e, dtype, tp.HOST_BOUND_U[form]) <= 1


def _seamed_exp(x):
    """an exponential with a 2^-40 relative step at every multiple of ln 2 / 2: a range reduction whose pieces do not meet"""
    return np.exp(x) * (1.0 + 2.0 ** -40 * (np.floor(x / (np.log(2.0) / 2)) % 2))


@needs_longdouble
def test_wrong_tanh_is_rejected():
    """float64, through the assertions of the GPU test at the GPU test's bound (4 x the measured worst error of the form)"""
    bound = tp.device_bound_u("q", "f64")
    scales = [(m, e) for m, e in tp.scales("f64") if -3 <= e <= 9]
    good = {s: tp.formula("q", tp.preactivation(s[0], s[1], "f64")) for s in scales}
    for s in scales:
        tp.check_values(good[s], s[0], s[1], "f64", "q", bound)
    # a seam in exp: the absolute error is what catches it, at moderate z
    caught = 0
    for s in scales:
        try:
            tp.check_values(tp.formula("q", tp.preactivation(s[0], s[1], "f64"), exp=_seamed_exp), s[0], s[1], "f64", "q", bound)
        except AssertionError as err:
            assert "off by" in str(err)
            caught += 1
    assert caught >= len(scales) - 3                                   # every scale that reaches |z| ~ 0.2
    # a clamp at |z| > 20 to 1 - 2^-30: the exact +-1 past saturation
    s = (1, 5)
    z = tp.preactivation(1, 5, "f64")
    a = np.where(np.abs(z) > 20, np.copysign(1 - 2.0 ** -30, z), good[s])
    with pytest.raises(AssertionError, match="not \\+-1"):
        tp.check_values(a, 1, 5, "f64", "q", bound)
    # one value a unit above 1; one sign lost; one NaN; a(0) = 2^-60
    for k, v, what in ((4000, np.nextafter(1.0, 2.0), "> 1"), (3000, -good[s][3000], "a\\(-z\\)"),
                       (100, np.nan, "not finite"), (tp.N_GRID, 2.0 ** -60, "at z = 0.0")):
        a = good[s].copy()
        a[k] = v
        with pytest.raises(AssertionError, match=what):
            tp.check_values(a, 1, 5, "f64", "q", bound)
    # the residual: d1 from an a that is one unit off next to 1 (1 - a^2 doubles there)
    f = tp.formula_residual("q", 1, 4, "f64")
    tp.check_residual(f, 1, 4, "f64", bound)
    a = good[(1, 4)]
    k = int(np.argmax((a < 1) & (a > 1 - 2.0 ** -40)))
    assert 0 < 1 - a[k] < 2.0 ** -40
    a2 = a.copy()
    a2[k] = a[k] - 2.0 ** -48                                          # 32 units: far outside the tanh bound
    c = tp.scale_value(1, 4)
    d1 = 1 - a2 * a2
    with pytest.raises(AssertionError, match="residual off"):
        tp.check_residual(a2 * (d1 * c) + 2 * tp.NU * a2 * d1 * c * c, 1, 4, "f64", bound)


@needs_longdouble
def test_float32_formula_loses_its_relative_accuracy_in_the_tail():
    """what the issue is about, on the host: tanh_r5 is absolute-accurate (within its 7 u), and at a = -1 + 2 e^{2z} that
    is a relative error in 1 - a^2 of order u / (1 - a^2): the residual's closed form is pinned by the propagated bound
    all the same, since the bound carries the same factor"""
    m, e = 5, 0
    a = tp.formula("r5", tp.preactivation(m, e, "f32")).astype(np.float64)
    ref = tp.reference(m, e)
    tail = np.abs(tp.exact_preactivation(m, e)) > 4
    d1, d1_ref = 1 - a * a, (1 - ref) * (1 + ref)
    assert float(np.max(np.abs(d1[tail] - d1_ref[tail]) / d1_ref[tail])) > 64 * tp.unit_roundoff("f32")
    assert tp.check_residual(tp.formula_residual("r5", m, e, "f32"), m, e, "f32", tp.HOST_BOUND_U["r5"]) <= 1
