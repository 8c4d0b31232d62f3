"""A range probe of the kernels' tanh through the forward kernels (test infrastructure, numpy only).

The net [2, W, 1] on the box lb = (-1, 0), ub = (1, 1) (so s_x = 1, s_t = 2) with

    W0[0, 0] = c,  W0[0, 1:] small random,  W0[1, :] = 0,  b0 = 0,  W1 = e_0,  b1 = 0

returns exactly tanh(c x): the first pre-activation of unit 0 is c ((x + 1) - 1) + 0 + 0, every other unit is multiplied by
zero on the way out.  On the grid x_k = k / 2048, k = -2048 ... 2048, at t = 0.5 (4097 points: 64 full tiles of 64 and one
point) and for c = m 2^e, m in {1, 3, 5}, both (x + 1) - 1 and c x_k are exact in float32 and float64: x_k has 12
significant bits, m three.  Two corrections to that statement, both at the ends of the exponent range and both harmless:
m 2^e overflows for m = 3, 5 at e = 1023 (127), so those scales take m = 1 only; and in float32 at e = -140 the products
k m 2^-151 lie below the subnormal spacing 2^-149, so z is c x_k rounded (off by at most 2^-150, nothing on the scale u of
the assertions, which are absolute).  The reference is np.tanh in np.longdouble at the exact product.

Which tanh a forward kernel has (pinn_predict / pinn_residual_at, engine.hip forward_taylor):

    W   kernel                 float64                     float32
    20  k_fwd20d / k_fwd20f    "q"   tanh_d                "r5"  tanh_r5
     7  k_forward              "lib" tanh()                "lib" tanhf()
    24  k_t16_fwd NT 4         "q"   tanh_mm = tanh_d      "lib" tanh_mm = tanhf
    65  k_t16_fwd NT 8         "q"                         "lib"

The forms, with u the unit roundoff of the type (every rounding is a relative error of at most u; all bounds are absolute, in
u, on a result of magnitude at most 1), E u the relative error of the exponential:

  "q"    sign(z) (1 - t) / (1 + t), t = e^{-2|z|} in (0, 1].  -2|z| is exact.  |da/dt| t = 2 t / (1 + t)^2 <= 1/2, so the
         exponential gives E / 2; 1 - t, 1 + t and the quotient round once each and the result is at most 1: 3 more.
         E = 2 (an exponential good to one unit in the last place): 4 u.  Odd by construction, 0 at 0, and never above 1:
         1 - t <= 1 + t and a correctly rounded quotient of x <= y is at most 1.
  "r5"   1 - 2 / (1 + e), e = e^{2z}.  For z < 0 the quotient q = 2 / (1 + e) lies in (1, 2]: the sum and the division
         give 2 u relative, the exponential E e / (1 + e) <= E / 2, all times q <= 2: 4 + E; the last subtraction rounds
         once more on a result of at most 1.  E = 2: 7 u (for z > 0 the quotient is below 1 and the error smaller).  Not
         odd: the two sides of 0 round differently, so oddness and a(0) are asked for within twice the bound only.
  "lib"  the library's tanh: 2 units in the last place (what the C library's manual lists for tanh and tanhf), which
         below 1 are 2 u.

These are the bounds the numpy restatements of the three forms (formula()) must meet on the probe's own grid
(HOST_BOUND_U; tests/test_tanh_probe_host.py).  The device replaces three correctly rounded operations by approximate
ones: exp by v_exp_f32 behind a multiplication by log2 e, or by the device library's exp; the quotient by v_rcp_f32 and a
multiplication, or by v_rcp_f64 and Newton steps.  The kernel guides document the cost of these instructions, not their
accuracy, so the device's bound is not derived from them but taken from a measurement: the worst error of the same formula
in numpy, in the same type, on the same grid, against longdouble (host_error()), times 4 -- each of the three approximate
operations stands in for one correctly rounded one (device_bound_u()).

Past the type's saturation point the result must be +-1 exactly: 1 - tanh z < u / 2 from z = 13 ln 2 = 9.011 (float32),
27.5 ln 2 = 19.062 (float64); asserted from 9.02 and 19.07, where 1 - tanh z is 2 % below u / 2 -- far more than any
relative error of an exponential moves it.

The residual at the same points, viscosity nu = 2^-10: W0[1, :] = 0 makes u_t = 0, u_x = d1 c, u_xx = -2 a d1 c^2 with
d1 = 1 - a^2, so

    f = u u_x - nu u_xx = a c d1 + 2 nu a d1 c^2 = (c + 2 nu c^2) g(a),   g(a) = a - a^3,  g'(a) = 1 - 3 a^2.

An error delta in a moves f by (|c| + 2 nu c^2) (|1 - 3 a^2| + 6 |a| delta) delta (first order, with the second-order
term so that the point a^2 = 1/3 is covered); the products and d1 = fma(-a, a, 1) round a few times, each relative to
its own term: 4 u (|a c d1| + |2 nu a d1 c^2|).  residual_bound() is the sum with delta = the tanh bound.  This is where
1 - a^2 at a one or two units below 1 is pinned: there g' = -2, so a d1 formed from a wrong a or as a cancelling
difference of rounded squares shows at full size.  The residual is checked at the scales where 2 nu c^2 is finite in
the type (beyond, u_xx itself overflows).
"""
import functools

import numpy as np

LB, UB = np.array([-1.0, 0.0]), np.array([1.0, 1.0])
NU = 2.0 ** -10
N_GRID = 2048
K_GRID = np.arange(-N_GRID, N_GRID + 1)
WIDTHS = (20, 7, 24, 65)
EXPONENTS = {"f64": (-1060, -600, -60, -30, -12, -3, 0, 2, 4, 5, 6, 9, 600, 1023),
             "f32": (-140, -100, -30, -12, -3, 0, 2, 4, 5, 6, 100, 127)}
DTYPES = {"f32": np.float32, "f64": np.float64}
FORM = {(20, "f64"): "q", (20, "f32"): "r5", (7, "f64"): "lib", (7, "f32"): "lib",
        (24, "f64"): "q", (24, "f32"): "lib", (65, "f64"): "q", (65, "f32"): "lib"}
KERNEL = {(20, "f64"): "k_fwd20d", (20, "f32"): "k_fwd20f", (7, "f64"): "k_forward", (7, "f32"): "k_forward",
          (24, "f64"): "k_t16_fwd NT 4", (24, "f32"): "k_t16_fwd NT 4", (65, "f64"): "k_t16_fwd NT 8",
          (65, "f32"): "k_t16_fwd NT 8"}
HOST_BOUND_U = {"q": 4.0, "r5": 7.0, "lib": 2.0}
DEVICE_FACTOR = 4.0
SATURATION = {"f32": 9.02, "f64": 19.07}
SMALL_Z = 2.0 ** -10


def unit_roundoff(dtype_name):
    return float(np.finfo(DTYPES[dtype_name]).eps) / 2.0


def longdouble_is_wider():
    return float(np.finfo(np.longdouble).eps) <= 1e-18


def scales(dtype_name):
    """-> [(m, e)]: c = m 2^e, finite in the type"""
    big = float(np.finfo(DTYPES[dtype_name]).max)
    return [(m, e) for e in EXPONENTS[dtype_name] for m in (1, 3, 5) if m * 2.0 ** e <= big]


def scale_value(m, e):
    return float(np.ldexp(float(m), e))


def points():
    """[4097, 2]: x_k = k / 2048 at t = 0.5"""
    return np.column_stack([K_GRID / float(N_GRID), np.full(K_GRID.size, 0.5)])


def weights(W, c, seed=0):
    """flat float64 weights of the probe net [2, W, 1] (layout: W0 [2, W] row-major, b0, W1 [W, 1], b1)"""
    rs = np.random.RandomState(seed)
    W0 = np.zeros((2, W))
    W0[0, :] = 2.0 ** -4 * rs.standard_normal(W)
    W0[0, 0] = c
    W1 = np.zeros((W, 1))
    W1[0, 0] = 1.0
    return np.concatenate([W0.ravel(), np.zeros(W), W1.ravel(), np.zeros(1)])


def preactivation(m, e, dtype_name):
    """z_k = c x_k as the kernels form it, in the type: c ((x + 1) - 1)"""
    dt = DTYPES[dtype_name]
    x = (K_GRID / float(N_GRID)).astype(dt)
    h = (x + dt(1)) - dt(1)
    with np.errstate(under="ignore"):
        return h * dt(scale_value(m, e))


def exact_preactivation(m, e):
    """c x_k in longdouble (exact: 3 + 12 significant bits, exponent range of the 80-bit format)"""
    return np.ldexp(np.asarray(m * K_GRID, dtype=np.longdouble), e - 11)


@functools.lru_cache(maxsize=None)
def reference(m, e):
    """tanh(c x_k) in longdouble (computed once, read-only)"""
    a = np.tanh(exact_preactivation(m, e))
    a.setflags(write=False)
    return a


def formula(form, z, exp=np.exp):
    """the form in numpy, every operation in z's type"""
    one = z.dtype.type(1)
    with np.errstate(over="ignore", under="ignore"):
        if form == "q":
            az = np.abs(z)
            t = exp(-(az + az))
            return np.copysign((one - t) / (one + t), z)
        if form == "r5":
            return one - (one + one) / (one + exp(z + z))
        if form == "lib":
            return np.tanh(z)
    raise ValueError(form)


def abs_error_u(a, m, e, dtype_name):
    """-> (worst |a - tanh(c x)| in u, its z)"""
    err = np.abs(np.asarray(a, dtype=np.float64).ravel().astype(np.longdouble) - reference(m, e))
    err = np.where(np.isfinite(np.asarray(a, dtype=np.float64).ravel()), err, np.inf)
    k = int(np.argmax(err))
    return float(err[k]) / unit_roundoff(dtype_name), float(exact_preactivation(m, e)[k])


@functools.lru_cache(maxsize=None)
def host_error(form, dtype_name):
    """-> (worst absolute error of the numpy restatement of `form` over every scale of the type, in u, its z)"""
    worst = (0.0, 0.0)
    for m, e in scales(dtype_name):
        worst = max(worst, abs_error_u(formula(form, preactivation(m, e, dtype_name)), m, e, dtype_name))
    return worst


def device_bound_u(form, dtype_name):
    return DEVICE_FACTOR * host_error(form, dtype_name)[0]


def check_values(a, m, e, dtype_name, form, bound_u):
    """the assertions on one scale's 4097 values a (as returned: float64 holding values of the type) ->
    {"worst_u", "worst_z", "rel_small"} (rel_small: worst relative error over 0 < |z| <= 2^-10, recorded, not asserted: the
    quotient forms are accurate absolutely, by design)"""
    tag = "%s %s c = %d * 2^%d" % (form, dtype_name, m, e)
    a = np.asarray(a, dtype=np.float64).ravel()
    assert a.shape == K_GRID.shape, a.shape
    z = exact_preactivation(m, e)
    ref = reference(m, e)
    assert np.all(np.isfinite(a)), "%s: not finite at z = %r" % (tag, float(z[~np.isfinite(a)][0]))
    assert np.all(np.abs(a) <= 1.0), "%s: |a| > 1 at z = %r" % (tag, float(z[np.abs(a) > 1.0][0]))
    assert np.array_equal(a.astype(DTYPES[dtype_name]).astype(np.float64), a), "%s: not values of the type" % tag
    sat = np.abs(z) >= SATURATION[dtype_name]
    bad = sat & (a != np.sign(z).astype(np.float64))
    assert not bad.any(), "%s: a = %r, not +-1, at z = %r" % (tag, a[bad][0], float(z[bad][0]))
    mid = N_GRID
    u = unit_roundoff(dtype_name)
    if form == "r5":
        odd = np.max(np.abs(a + a[::-1])) / u
        assert odd <= 2 * bound_u and abs(a[mid]) <= 2 * bound_u * u, "%s: a(z) + a(-z) up to %.2f u, a(0) = %r" % (
            tag, odd, a[mid])
    else:
        assert np.array_equal(a, -a[::-1]), "%s: a(-z) != -a(z) at z = %r" % (tag, float(z[a != -a[::-1]][0]))
        assert a[mid] == 0.0, "%s: a(0) = %r" % (tag, a[mid])
    worst_u, worst_z = abs_error_u(a, m, e, dtype_name)
    assert worst_u <= bound_u, "%s: off by %.2f u at z = %r, bound %.2f u" % (tag, worst_u, worst_z, bound_u)
    small = (np.abs(z) <= SMALL_Z) & (z != 0)
    rel = np.abs(a.astype(np.longdouble)[small] - ref[small]) / np.abs(ref[small])
    return {"worst_u": worst_u, "worst_z": worst_z, "rel_small": float(rel.max()) if rel.size else 0.0}


# ---- residual -------------------------------------------------------------------------------------------------------
def residual_scales(dtype_name):
    """the scales at which 2 c^2 (the largest intermediate of u_xx) is finite in the type"""
    big = np.longdouble(np.finfo(DTYPES[dtype_name]).max)
    return [(m, e) for m, e in scales(dtype_name) if np.ldexp(np.longdouble(m * m), 2 * e + 1) <= big]


@functools.lru_cache(maxsize=None)
def residual_reference(m, e):
    """-> (f, |term 1|, |term 2|) of f = a c d1 + 2 nu a d1 c^2 in longdouble"""
    a = reference(m, e)
    c = np.ldexp(np.longdouble(m), e)
    d1 = (1 - a) * (1 + a)
    t1, t2 = a * c * d1, 2 * np.longdouble(NU) * a * d1 * c * c
    return t1 + t2, np.abs(t1), np.abs(t2)


def residual_bound(m, e, dtype_name, tanh_bound_u):
    """the tanh bound propagated through f to first order (see above) plus 4 u on the magnitude of each term, per point"""
    u = np.longdouble(unit_roundoff(dtype_name))
    a = np.abs(reference(m, e))
    c = np.ldexp(np.longdouble(m), e)
    delta = tanh_bound_u * u
    _, t1, t2 = residual_reference(m, e)
    return (c + 2 * np.longdouble(NU) * c * c) * (np.abs(1 - 3 * a * a) + 6 * a * delta) * delta + 4 * u * (t1 + t2)


def check_residual(f, m, e, dtype_name, tanh_bound_u):
    """-> worst |f - closed form| / bound over the grid; asserts finite and <= 1"""
    tag = "%s c = %d * 2^%d" % (dtype_name, m, e)
    f = np.asarray(f, dtype=np.float64).ravel()
    assert f.shape == K_GRID.shape, f.shape
    z = exact_preactivation(m, e)
    assert np.all(np.isfinite(f)), "%s: residual not finite at z = %r" % (tag, float(z[~np.isfinite(f)][0]))
    ref, _, _ = residual_reference(m, e)
    bound = residual_bound(m, e, dtype_name, tanh_bound_u)
    assert np.all(bound[z != 0] > 0)
    ratio = np.where(bound > 0, np.abs(f.astype(np.longdouble) - ref) / np.where(bound > 0, bound, 1), 0)
    ratio = np.where((bound == 0) & (f != 0), np.inf, ratio)
    k = int(np.argmax(ratio))
    assert ratio[k] <= 1, "%s: residual off by %.3e at z = %r (a = %r), bound %.3e" % (
        tag, abs(float(f[k]) - float(ref[k])), float(z[k]), float(reference(m, e)[k]), float(bound[k]))
    return float(ratio[k])


def formula_residual(form, m, e, dtype_name):
    """the forward kernels' residual of the probe net in numpy, every operation in the type: d1 = 1 - a a (not fused: the
    harsher of the two), u_x = d1 c, u_xx = d1 ((-2 a c) c), f = u u_x - nu u_xx"""
    dt = DTYPES[dtype_name]
    a = formula(form, preactivation(m, e, dtype_name))
    c = dt(scale_value(m, e))
    with np.errstate(under="ignore", over="ignore"):
        d1 = dt(1) - a * a
        return a * (d1 * c) - dt(NU) * (d1 * ((dt(-2) * a * c) * c))
