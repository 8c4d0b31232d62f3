"""Fuzz cases of the advection-diffusion-reaction family and their restatement in any dtype (test infrastructure, numpy only).

The parity files of the family (tests/test_gpu_adr*.py) share one weight regime (a perturbed Glorot draw: no hidden
pre-activation leaves the linear part of tanh), a fixed lattice of shapes and five named coefficient sets.  Here the shapes,
the features present, the coefficients and the weight regime are drawn, the edges of the launch plan are placed by hand, and a
share of the nets is pushed into the tail of tanh (grad_entries.make_case: gain0, gain).

  restate(case, dtype)        the adr kind with any subset of {pairs, data, Robin points, source, coefficient fields}, all
                              arithmetic in `dtype`, on grad_entries._forward / _backward; statements and their order are those
                              of adr_var_ref.var_loss_grad and adr_robin_ref.  The adr_ide kind: adr_ide_ref.restate as it is;
                              point weights: adr_pw_ref.loss_grad (float64 only).
                              -> dict: loss, terms (mse_f, mse_u, mse_b + mse_w), grad, A (grad_entries' entrywise scale, every
                              term of the loss, Robin included), f, A_f, r, A_r
  cases(n_cu)                 fixed edge cases, the launch-plan boundary at n_cu tiles, random draws; deterministic
  yardsticks(case, dtype)     per quantity max(plain error of restate(dtype) against the wider type, 32 u) on its own scale
  refusal, first_admitted_seed, SEEDS    admission as grad_entries does it, and its record
  mutants(case)               wrong results a comparator has to catch

Scales.  Gradient entries: A.  f: A_f = |u_t| + |a0 u_x| + |a1 u u_x| + |nu u_xx| + |r1 u| + |r2 u^2| + |r3 u^3| + |s|.
r: A_r = |alpha u| + |beta u_x| + |g|.  The loss and each of its terms: the loss itself.

N_f = 0.  The kind accepts a set without collocation points (pairs, data, Robin points only): mse_f = 0 and no sweep, as the
engine computes it (1 / N_f is taken as 0).
"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adr_ide_ref  # noqa: E402
import adr_pw_ref  # noqa: E402
import adr_var_cells as cells  # noqa: E402
import grad_entries as ge  # noqa: E402

LB, UB = cells.LB, cells.UB
HOST_N_CU = 256                    # the host tests' compute-unit count (an MI355X has 256 too)
MAX_POINTS = 16600
GAIN0, GAIN = ge.GAIN0, 3.0
CLASSES = ("ungained", "gain0", "gain")
QUANTITIES = ("grad", "f", "r", "loss")


# ---- the restatement ------------------------------------------------------------------------------------------------------
def _col(v, n, dt):
    return np.asarray(v, dtype=np.float64).astype(dt).reshape(n, 1)


def restate_adr(layers, w, coeffs, X_f, X_u=None, u=None, X_lo=None, X_hi=None, robin=None, s=None, K=None, dtype=np.float64,
                n_f_total=None, n_u_total=None, n_b_total=None, n_w_total=None, lb=LB, ub=UB):
    """adr_var_ref.var_loss_grad + adr_robin_ref.robin_loss_grad, statement for statement, in `dtype`.  K [N_f, 6] or None (the
    constants `coeffs` then stand where the columns would: the same IEEE operation per element); s [N_f] or None; robin =
    (X_w, alpha, beta, g) or None.  n_*_total: the denominators of a set that has lost points (mutants)."""
    dt = np.dtype(dtype).type
    wide = np.longdouble if dt is np.longdouble else np.float64
    lbd = np.asarray(lb, dtype=wide)
    sc = (2 / (np.asarray(ub, dtype=wide) - lbd)).astype(dt)            # the engine: 2 / (ub - lb) in float64, then cast
    lbd = lbd.astype(dt)
    cast = lambda x, cols: np.asarray(x, dtype=np.float64).astype(dt).reshape(-1, cols)      # noqa: E731
    params = ge._unpack(np.asarray(w, dtype=np.float64), layers, dt)
    G = [[np.zeros(W.shape, dt), np.zeros(b.shape, dt)] for W, b in params]
    A = [[np.zeros(W.shape), np.zeros(b.shape)] for W, b in params]
    zero = lambda x: np.zeros_like(x)      # noqa: E731
    X_f = cast(X_f, 2)
    n = X_f.shape[0]
    mse_f = mse_u = mse_b = mse_w = dt(0)
    f, A_f = np.zeros((0, 1), dt), np.zeros((0, 1))
    if n:
        if K is not None:
            K = np.asarray(K, dtype=np.float64)
            assert K.shape == (n, 6), K.shape
            a0, a1, nu, r1, r2, r3 = (_col(K[:, j], n, dt) for j in range(6))
        else:
            a0, a1, nu, r1, r2, r3 = (dt(v) for v in coeffs)
        N_f = dt(n if n_f_total is None else n_f_total)
        (h, p, q, r), cache = ge._forward(params, X_f, lbd, sc, False)
        f = q + (a0 + a1 * h) * p - nu * r + r1 * h + r2 * h * h + r3 * h * h * h
        A_f = (ge._abs64(q) + ge._abs64(a0 * p) + ge._abs64(a1 * h * p) + ge._abs64(nu * r) + ge._abs64(r1 * h)
               + ge._abs64(r2 * h * h) + ge._abs64(r3 * h * h * h))
        if s is not None:
            sv = _col(s, n, dt)
            f = f - sv
            A_f = A_f + ge._abs64(sv)
        mse_f = np.sum(f * f) / N_f
        fb = dt(2) * f / N_f
        ge._backward(params, cache, fb * (a1 * p + r1 + dt(2) * r2 * h + dt(3) * r3 * h * h), fb * (a0 + a1 * h), fb, -nu * fb,
                     G, A)
    if X_u is not None and len(X_u):
        X_u, uu = cast(X_u, 2), cast(u, 1)
        N_u = dt(X_u.shape[0] if n_u_total is None else n_u_total)
        (hu, _, _, _), cu = ge._forward(params, X_u, lbd, sc, False)
        d = hu - uu
        mse_u = np.sum(d * d) / N_u
        ge._backward(params, cu, dt(2) * d / N_u, zero(d), zero(d), zero(d), G, A)
    if X_lo is not None and len(X_lo):
        X_lo, X_hi = cast(X_lo, 2), cast(X_hi, 2)
        N_b = dt(X_lo.shape[0] if n_b_total is None else n_b_total)
        (hl, pl, _, _), cl = ge._forward(params, X_lo, lbd, sc, False)
        (hh, ph, _, _), ch = ge._forward(params, X_hi, lbd, sc, False)
        dh, dp = hl - hh, pl - ph
        mse_b = (np.sum(dh * dh) + np.sum(dp * dp)) / N_b
        ge._backward(params, cl, dt(2) * dh / N_b, dt(2) * dp / N_b, zero(dh), zero(dh), G, A)
        ge._backward(params, ch, dt(-2) * dh / N_b, dt(-2) * dp / N_b, zero(dh), zero(dh), G, A)
    loss = mse_f + mse_u + mse_b
    rr, A_r = np.zeros(0, dt), np.zeros(0)
    if robin is not None and len(robin[0]):
        X_w = cast(robin[0], 2)
        m = X_w.shape[0]
        N_w = dt(m if n_w_total is None else n_w_total)
        al, be, gg = (_col(np.broadcast_to(np.asarray(v, dtype=np.float64).reshape(-1), (m,)), m, dt) for v in robin[1:])
        (h, p, _, _), cache = ge._forward(params, X_w, lbd, sc, False)
        rw = al * h + be * p - gg
        mse_w = np.sum(rw * rw) / N_w
        ge._backward(params, cache, dt(2) * rw * al / N_w, dt(2) * rw * be / N_w, zero(rw), zero(rw), G, A)
        loss = loss + mse_w
        rr, A_r = rw.ravel(), (ge._abs64(al * h) + ge._abs64(be * p) + ge._abs64(gg)).ravel()
    flat = lambda T: np.concatenate([np.concatenate([W.ravel(), b.ravel()]) for W, b in T])      # noqa: E731
    grad = flat(G)
    assert grad.dtype == np.dtype(dt), grad.dtype                      # nothing was promoted on the way
    return {"loss": loss, "terms": (mse_f, mse_u, mse_b + mse_w), "mse_b": mse_b, "mse_w": mse_w, "grad": grad, "A": flat(A),
            "f": f, "A_f": A_f, "r": rr, "A_r": A_r}


def _ide_scale(layers, theta, X_f, dtype, lb=LB, ub=UB):
    """A_f of the adr_ide kind at its current coefficients (adr_ide_ref.restate returns f only)"""
    dt = np.dtype(dtype).type
    nn = adr_ide_ref.n_net(layers)
    params = ge._unpack(np.asarray(theta[:nn], dtype=np.float64), layers, dt)
    lb, ub = np.asarray(lb, dtype=np.float64), np.asarray(ub, dtype=np.float64)
    sc = (2 / (ub - lb)).astype(dt)
    (h, p, q, r), _ = ge._forward(params, np.asarray(X_f, dtype=np.float64).astype(dt), lb.astype(dt), sc, False)
    a0, a1, lnu, r1, r2, r3 = (dt(v) for v in theta[nn:])
    nu = np.exp(lnu)
    return (ge._abs64(q) + ge._abs64(a0 * p) + ge._abs64(a1 * h * p) + ge._abs64(nu * r) + ge._abs64(r1 * h)
            + ge._abs64(r2 * h * h) + ge._abs64(r3 * h * h * h))


def restate(case, dtype, inp=None, **totals):
    """the case's kind in `dtype` -> the dict of restate_adr.  inp: other inputs than the case's own (mutants, a rank's block);
    totals: n_f_total, n_u_total, n_b_total, n_w_total (the kinds without Robin points take no n_w_total but None)"""
    x = inputs(case["id"]) if inp is None else inp
    L = case["layers"]
    none = lambda a: a if a is not None and len(a) else None      # noqa: E731
    if case["kind"] == "adr":
        return restate_adr(L, x["w"], case["coeffs"], x["X_f"], x["X_u"], x["u"], x["X_lo"], x["X_hi"], x["robin"], x["s"],
                           x["K"], dtype, **totals)
    assert totals.pop("n_w_total", None) in (None, 0)
    if case["kind"] == "adr_ide":
        lo, g, A, ex = adr_ide_ref.restate(x["w"], L, LB, UB, x["X_f"], none(x["X_u"]), x["u"], none(x["X_lo"]), x["X_hi"],
                                           case["mask"], dtype, **totals)
        return {"loss": lo, "terms": (ex["mse_f"], ex["mse_u"], ex["mse_b"]), "grad": g, "A": A, "f": ex["f"],
                "A_f": _ide_scale(L, x["w"], x["X_f"], dtype), "r": np.zeros(0), "A_r": np.zeros(0)}
    assert case["kind"] == "adr_pw" and np.dtype(dtype) == np.float64
    lo, g, terms, _ = adr_pw_ref.loss_grad(x["w"], L, LB, UB, x["X_f"], none(x["X_u"]), x["u"], none(x["X_lo"]), x["X_hi"],
                                           case["coeffs"], none(x["lam"][0]), x["lam"][1], none(x["lam"][2]), **totals)
    return {"loss": lo, "terms": terms, "grad": g, "A": None, "f": None, "A_f": None, "r": np.zeros(0), "A_r": np.zeros(0)}


def layout(case):
    return adr_ide_ref.layout(case["layers"]) if case["kind"] == "adr_ide" else ge.blocks(case["layers"], "adr")


# ---- cases ------------------------------------------------------------------------------------------------------------------
def layers_of(depth, width=20):
    return [2] + [width] * depth + [1]


def n_points(case):
    return 2 * case["n_b"] + case["n_0"] + case["n_f"] + case["n_w"]


def n_tiles(case):
    """64-point tiles of the assembled set: the Robin block counts (engine.hip, ensure_sets: n_pad)"""
    return (n_points(case) + 63) // 64


def plan_of(case, n_cu):
    """what fused20d_launch_any takes on kernel path 7: the one-tile kernel iff n_wg = min(tiles, n_cu) >= tiles"""
    return "one-tile" if n_tiles(case) <= n_cu else "tile-loop"


def _spec(tag, kind, layers, n_b, n_0, n_f, n_w, seed, coeffs, source=False, fields=False, cls="ungained", mask=None,
          plan=None):
    width, depth = layers[1], len(layers) - 2
    on7 = width == 20 and depth in (4, 6, 8)
    if kind == "adr_pw":
        paths = {"f64": (7,)}
    elif on7:
        paths = {"f64": (0, 7), "f32": (0,)}
    else:
        paths = {"f64": (0,), "f32": (0,)}                              # off-shape nets: the generic kernels only
    cid = "%s-%s-%dx%d-b%d-u%d-f%d-w%d%s%s%s" % (tag, kind, depth, width, n_b, n_0, n_f, n_w, "-src" if source else "",
                                                 "-var" if fields else "", {"ungained": "", "gain0": "-gain0x%g" % GAIN0,
                                                                            "gain": "-gainx%g" % GAIN}[cls])
    return {"id": cid, "kind": kind, "layers": list(layers), "n_b": n_b, "n_0": n_0, "n_f": n_f, "n_w": n_w, "seed": seed,
            "coeffs": [float(v) for v in coeffs], "source": source, "fields": fields, "cls": cls, "mask": mask, "plan": plan,
            "gain0": GAIN0 if cls == "gain0" else None, "gain": GAIN if cls == "gain" else None, "paths": paths}


def _draw_coeffs(rs, nu_positive=False):
    """every coefficient 0 with probability 1/3, else +-U(0.01, 5); nu from {0, 1e-4, U(0.01, 1), -0.05}"""
    c = [0.0 if rs.randint(3) == 0 else float(rs.choice([-1.0, 1.0]) * rs.uniform(0.01, 5.0)) for _ in range(6)]
    pick = rs.randint(4)
    u = float(rs.uniform(0.01, 1.0))
    c[2] = u if nu_positive else [0.0, 1e-4, u, -0.05][pick]
    return c


@functools.lru_cache(maxsize=None)
def specs(n_cu=HOST_N_CU):
    """every case before admission, deterministic from one RandomState; base seeds 100 apart, so the searches do not meet"""
    rs = np.random.RandomState(20261020)
    out = []
    seed = lambda: 11000 + 100 * len(out)      # noqa: E731
    some = [0.3, -0.8, 0.02, 0.6, -0.4, 1.5]
    # fewer than 64 points in all; the Robin point as the 64th lane / alone in a second tile; N_f = 0
    for i, (n_b, n_0, n_f, n_w) in enumerate([(0, 0, 1, 0), (1, 1, 1, 1), (3, 5, 17, 9), (0, 0, 63, 1), (0, 0, 64, 1),
                                              (2, 30, 0, 5)]):
        out.append(_spec("edge", "adr", layers_of((8, 4, 6)[i % 3]), n_b, n_0, n_f, n_w, seed(), some,
                         source=i in (2, 4), fields=i in (2, 3)))
    # the launch-plan boundary: n_all = 2 n_b + n_0 + N_f fills n_cu tiles less 30 lanes; Robin points alone decide the plan
    n_b, n_0 = 3, 50
    front = 2 * n_b + n_0
    for full in (False, True):
        for i, (short, n_w, tag) in enumerate([(30, 20, "plan-last-tile-partly-robin"), (30, 40, "plan-robin-spills"),
                                               (30, 30, "plan-no-padding"), (0, 1, "plan-one-live-lane")]):
            n_f = 64 * n_cu - short - front
            depth = ((8, 4, 6, 8), (4, 6, 8, 4))[full][i]
            c = _spec(tag, "adr", layers_of(depth), n_b, n_0, n_f, n_w, seed(), _draw_coeffs(rs), source=full, fields=full,
                      plan=True)
            assert n_tiles(c) == n_cu + (n_w in (40, 1)) and n_points(c) <= MAX_POINTS + 64 * max(0, n_cu - HOST_N_CU)
            out.append(c)
    # one third gained, gain0 and gain in turn
    cls_of = lambda k: CLASSES[0] if k % 3 else CLASSES[1 + (k // 3) % 2]      # noqa: E731
    counts = lambda: (int(rs.randint(0, 41)), int(rs.randint(0, 121)), int(rs.randint(1, 1501)), int(rs.randint(0, 91)))      # noqa: E731
    # kernel path 7 (and 0): depth 4, 6, 8 at width 20
    for k in range(12):
        n_b, n_0, n_f, n_w = counts()
        feat = int(rs.randint(4))
        out.append(_spec("rnd", "adr", layers_of((4, 6, 8)[k % 3]), n_b, n_0, n_f, n_w, seed(), _draw_coeffs(rs),
                         source=bool(feat & 1), fields=bool(feat & 2), cls=cls_of(k)))
    # off-shape nets: path 0 only
    for k in range(6):
        n_b, n_0, n_f, n_w = counts()
        feat = int(rs.randint(4))
        out.append(_spec("rnd", "adr", layers_of(int(rs.randint(1, 6)), (1, 7, 33)[k % 3]), n_b, n_0, n_f, n_w, seed(),
                         _draw_coeffs(rs), source=bool(feat & 1), fields=bool(feat & 2), cls=cls_of(k + 1)))
    # adr_ide: a random mask, nu > 0 (the kind stores log nu); no Robin points, source or fields (the kind has no variant)
    for k in range(4):
        n_b, n_0, n_f, _ = counts()
        out.append(_spec("rnd", "adr_ide", layers_of((8, 4, 6, 8)[k]), n_b, max(n_0, 1), n_f, 0, seed(),
                         _draw_coeffs(rs, nu_positive=True), mask=int(rs.randint(1, 64)), cls=cls_of(k + 2)))
    # fixed point weights lambda in U(0.2, 3): float64, path 7
    for k in range(3):
        n_b, n_0, n_f, _ = counts()
        out.append(_spec("rnd", "adr_pw", layers_of((4, 6, 8)[k]), n_b, n_0, n_f, 0, seed(), _draw_coeffs(rs)))
    assert len({c["id"] for c in out}) == len(out)
    return tuple(out)


def fields_of(X, coeffs):
    """every column within +-30 % of its constant: a zero constant gives a zero column, a negative nu stays negative"""
    X = np.asarray(X, dtype=np.float64)
    x, t = X[:, 0], X[:, 1]
    return np.column_stack([float(coeffs[j]) * (1.0 + 0.3 * np.sin((j + 2) * x + j) * np.exp(-t / (j + 1))) for j in range(6)])


def make_inputs(case, seed=None):
    """weights 0.9 / sqrt(max(W, 2)) N(0, 1), biases included (tests/test_gpu_fuzz.py), with grad_entries.make_case's gains;
    uniform points, targets x^2 cos(pi x) e^-t, wall pairs at common times, Robin rows as adr_var_cells.robin_points draws them"""
    rs = np.random.RandomState(case["seed"] if seed is None else seed)
    L = case["layers"]
    W = L[1]
    P = sum(a * b + b for a, b in zip(L[:-1], L[1:]))
    w = 0.9 / np.sqrt(max(W, 2)) * rs.standard_normal(P)
    if case["gain"]:
        w *= case["gain"]
    if case["gain0"]:
        w[:3 * W] *= case["gain0"]
    pts = lambda n: np.column_stack([rs.uniform(LB[0], UB[0], n), rs.uniform(LB[1], UB[1], n)])      # noqa: E731
    X_f, X_u = pts(case["n_f"]), pts(case["n_0"])
    u = (X_u[:, 0:1] ** 2) * np.cos(np.pi * X_u[:, 0:1]) * np.exp(-X_u[:, 1:2])      # the family's data, carried on in t
    tb = rs.uniform(LB[1], UB[1], case["n_b"])
    X_lo, X_hi = np.column_stack([np.full(case["n_b"], LB[0]), tb]), np.column_stack([np.full(case["n_b"], UB[0]), tb])
    robin = None
    if case["n_w"]:
        m = case["n_w"]
        j = np.arange(m)
        X_w = np.column_stack([np.where(j % 2, 1.0, -1.0), rs.uniform(0, 1, m)])
        alpha, beta, g = rs.uniform(-1.5, 1.5, m), rs.uniform(-1.5, 1.5, m), rs.uniform(-1, 1, m)
        alpha[j % 5 == 4] = 0.0
        beta[(j % 7 == 6) & (alpha != 0.0)] = 0.0
        robin = (X_w, alpha, beta, g)
    out = {"w": w, "X_f": X_f, "X_u": X_u, "u": u, "X_lo": X_lo, "X_hi": X_hi, "robin": robin,
           "s": cells.source_of(X_f) if case["source"] else None, "K": fields_of(X_f, case["coeffs"]) if case["fields"] else None,
           "lam": None}
    if case["kind"] == "adr_ide":
        out["w"] = adr_ide_ref.pack(w, case["coeffs"])
    if case["kind"] == "adr_pw":
        out["lam"] = tuple(rs.uniform(0.2, 3.0, n) for n in (case["n_0"], case["n_f"], case["n_b"]))
    for a in list(out.values()) + list(robin or ()) + list(out["lam"] or ()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


# ---- yardsticks -------------------------------------------------------------------------------------------------------------
def has_wide(case, dtype_name, n=None):
    """float32 is judged against float64; float64 against longdouble up to grad_entries.LONGDOUBLE_POINTS points (n: the point
    count of explicit inputs, where they are not the case's own)"""
    if case["kind"] == "adr_pw":
        return False                                                  # adr_pw_ref is float64 only
    n = n_points(case) if n is None else n
    return dtype_name == "f32" or (n <= ge.LONGDOUBLE_POINTS and ge.longdouble_is_wider())


def n_points_of(inp):
    """n_points of explicit inputs (make_inputs' dict, or a block of it)"""
    return 2 * len(inp["X_lo"]) + len(inp["X_u"]) + len(inp["X_f"]) + (len(inp["robin"][0]) if inp["robin"] else 0)


def _scaled(got, ref, scale):
    """worst |got - ref| / scale, the difference taken in the reference's type; an element without a scale must be exact"""
    if np.size(ref) == 0:
        return 0.0
    ref = np.asarray(ref)
    diff = np.asarray(np.abs(np.asarray(got, dtype=ref.dtype).reshape(ref.shape) - ref), dtype=np.float64)
    diff[~np.isfinite(np.asarray(got, dtype=np.float64).reshape(ref.shape))] = np.inf
    scale = np.asarray(scale, dtype=np.float64).reshape(ref.shape)
    dev = np.where(scale > 0, diff / np.where(scale > 0, scale, 1.0), np.where(diff > 0, np.inf, 0.0))
    return float(np.max(dev))


def deviations(got, ref):
    """got, ref: dicts with loss, terms, grad, f, r (ref also A, A_f, A_r) -> {quantity: deviation on its own scale}; the loss
    and its three terms share the quantity "loss" (the worst of the four, each as a share of the loss)"""
    lo = np.asarray(ref["loss"])
    share = lambda a, b: float(abs(np.asarray(a, dtype=lo.dtype) - b) / lo)      # noqa: E731
    return {"grad": _scaled(got["grad"], ref["grad"], ref["A"]), "f": _scaled(got["f"], ref["f"], ref["A_f"]),
            "r": _scaled(got["r"], ref["r"], ref["A_r"]),
            "loss": max([share(got["loss"], ref["loss"])] + [share(a, b) for a, b in zip(got["terms"], ref["terms"])])}


@functools.lru_cache(maxsize=None)
def _restated(cid, type_name):
    return restate(CASE_BY_ID[cid], {"f32": np.float32, "f64": np.float64, "ld": np.longdouble}[type_name])


_TYPES = {"f32": np.float32, "f64": np.float64, "ld": np.longdouble}


def _wider_name(case, dtype_name, n=None):
    return ("f64" if dtype_name == "f32" else "ld") if has_wide(case, dtype_name, n) else "f64"


def reference(cid, dtype_name, inp=None, totals=None):
    """the restatement a device result in `dtype_name` is compared with: the wider type, or float64 itself for a float64 set
    that is too large for an 80-bit run (cached: shared by every config, never written to).
    inp, totals: explicit inputs and denominators (a rank's block, adr_shards.shard_inputs) -- `cid` is then the case itself or
    its id, the rule for the wider type goes by the point count of `inp`, and nothing is cached here"""
    if inp is None:
        return _restated(cid, _wider_name(CASE_BY_ID[cid], dtype_name))
    case = cid if isinstance(cid, dict) else CASE_BY_ID[cid]
    return restate(case, _TYPES[_wider_name(case, dtype_name, n_points_of(inp))], inp, **(totals or {}))


def yardsticks(cid, dtype_name, inp=None, totals=None, ref=None):
    """-> {quantity: max(plain error, 32 u)}; a float64 set without an 80-bit run: grad_entries.ASSUMED_F64_ULPS u.
    inp, totals: as reference() takes them; ref: reference(cid, dtype_name, inp, totals) where the caller holds it already"""
    if inp is None:
        return _yardsticks(cid, dtype_name)
    case = cid if isinstance(cid, dict) else CASE_BY_ID[cid]
    u = ge.unit_roundoff(ge.DTYPES[dtype_name])
    if not has_wide(case, dtype_name, n_points_of(inp)):
        return {q: max(ge.ASSUMED_F64_ULPS, ge.FLOOR_ULPS) * u for q in QUANTITIES}
    ref = reference(case, dtype_name, inp, totals) if ref is None else ref
    plain = deviations(restate(case, _TYPES[dtype_name], inp, **(totals or {})), ref)
    return {q: max(plain[q], ge.FLOOR_ULPS * u) for q in QUANTITIES}


@functools.lru_cache(maxsize=None)
def _yardsticks(cid, dtype_name):
    case = CASE_BY_ID[cid]
    u = ge.unit_roundoff(ge.DTYPES[dtype_name])
    if not has_wide(case, dtype_name):
        return {q: max(ge.ASSUMED_F64_ULPS, ge.FLOOR_ULPS) * u for q in QUANTITIES}
    plain = deviations(_restated(cid, dtype_name), reference(cid, dtype_name))
    return {q: max(plain[q], ge.FLOOR_ULPS * u) for q in QUANTITIES}


def dtypes_judged(case):
    return [d for d in ("f32", "f64") if d in case["paths"] and (d == "f32" or ge.longdouble_is_wider())]


# ---- admission, as grad_entries does it ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def preactivation_stats(cid, dtype_name):
    """-> (max |z|, share of |z| > 3) over every hidden pre-activation at every point of the case, forward pass in `dtype_name`"""
    case = CASE_BY_ID[cid]
    x = inputs(cid)
    dt = ge.DTYPES[dtype_name]
    nn = adr_ide_ref.n_net(case["layers"])
    params = ge._unpack(np.asarray(x["w"][:nn], dtype=np.float64), case["layers"], dt)
    s = (2 / (UB - LB)).astype(dt)
    zs = []
    for X in (x["X_f"], x["X_u"], x["X_lo"], x["X_hi"], x["robin"][0] if x["robin"] else np.zeros((0, 2))):
        if len(X):
            h = s * (np.asarray(X).astype(dt) - LB.astype(dt)) - dt(1)
            for W, b in params[:-1]:
                z = h @ W + b
                zs.append(np.abs(z).ravel())
                h = np.tanh(z)
    z = np.concatenate(zs).astype(np.float64)
    return float(z.max()), float(np.mean(z > ge.SAT_TAIL_Z))


def refusal(cid):
    """-> None if the case meets the admission conditions in every dtype it runs in, else the first one it misses, in words:
    a gained case reaches the tail of tanh (SAT_MAX_Z, SAT_TAIL_SHARE); every yardstick of the case is at most
    SAT_YARDSTICK_ULPS u -- a draw whose plain arithmetic is worse conditioned than that is no yardstick for a kernel; every
    mutant stands SAT_MUTANT_MARGIN x above the gradient's bound -- a draw on which a lost point drowns in one loss term's
    rounding checks nothing"""
    case = CASE_BY_ID[cid]
    if case["kind"] == "adr_pw":
        return None                              # float64 against the float64 restatement only: no yardstick to admit
    if case["cls"] != "ungained":
        for d in dtypes_judged(case):
            zmax, share = preactivation_stats(cid, d)
            if zmax < ge.SAT_MAX_Z or share < ge.SAT_TAIL_SHARE:
                return "%s: max |z| %.2f, %.2f %% beyond 3" % (d, zmax, 100 * share)
    for d in dtypes_judged(case):
        u = ge.unit_roundoff(ge.DTYPES[d])
        for q, y in sorted(yardsticks(cid, d).items()):
            if not y <= ge.SAT_YARDSTICK_ULPS * u:
                return "%s: yardstick of %s %.0f u" % (d, q, y / u)
    for d in dtypes_judged(case):
        for name, ratio in sorted(mutant_margins(cid, d).items()):
            if not ratio >= ge.SAT_MUTANT_MARGIN:
                return "%s: mutant %s is %.1f x the bound" % (d, name, ratio)
    return None


@functools.lru_cache(maxsize=None)
def first_admitted_seed(base_id, n_cu=HOST_N_CU):
    """-> (seed, ((refused seed, why), ...)): the first seed from the spec's base seed that refusal() lets through"""
    spec = next(c for c in specs(n_cu) if c["id"] == base_id)
    refused = []
    for seed in range(spec["seed"], spec["seed"] + ge.SAT_SEARCH_SPAN):
        c = dict(spec, seed=seed, id="%s-s%d" % (base_id, seed), base_id=base_id)
        listed = c["id"] in CASE_BY_ID
        CASE_BY_ID.setdefault(c["id"], c)
        why = refusal(c["id"])
        if not listed:
            del CASE_BY_ID[c["id"]]
        if why is None:
            return seed, tuple(refused)
        refused.append((seed, why))
    raise RuntimeError("%s: no admissible draw in %d seeds: %s" % (base_id, ge.SAT_SEARCH_SPAN, refused))


# What first_admitted_seed() returns for every spec with n_cu = HOST_N_CU (a record, not a choice: tests/test_adr_fuzz_host.py
# runs the search and fails if a seed here is not the one it finds).  A spec that is not listed keeps its base seed.
SEEDS = {
    "edge-adr-8x20-b0-u0-f63-w1-var": 11301,                          # 11300: float32 gradient yardstick 666 u
    "plan-no-padding-adr-8x20-b3-u50-f16298-w30-src-var": 12201,      # 12200: float32 mutant robin 1.4 x
    "rnd-adr-8x20-b8-u62-f1089-w85-src": 12601,                       # 12600: float32 mutant robin 3.8 x
    "rnd-adr-4x20-b36-u44-f1219-w63-gainx3": 12703,                   # float32 gradient yardsticks 442, 697, 339 u
    "rnd-adr-4x20-b10-u54-f553-w22-gainx3": 13302,                    # float32 mutant robin 1.6 x; yardstick 511 u
    "rnd-adr-3x1-b30-u37-f1269-w37": 13601,                           # 13600: float32 mutant pair 0.1 x
    "rnd-adr-3x33-b19-u44-f94-w59-src-gainx3": 13802,                 # float32 mutant pair 3.6 x, 6.5 x
}

CASE_BY_ID = {}


@functools.lru_cache(maxsize=None)
def cases(n_cu=HOST_N_CU):
    """the admitted cases.  The plan-boundary cases depend on n_cu; their seeds are searched for n_cu = HOST_N_CU only, so on
    another device they keep their base seeds (ungained nets: the rule refuses one such draw in twenty)"""
    out = []
    for c in specs(n_cu):
        seed = SEEDS.get(c["id"], c["seed"])
        out.append(dict(c, seed=seed, id="%s-s%d" % (c["id"], seed), base_id=c["id"]))
    CASE_BY_ID.update((c["id"], c) for c in out)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def inputs(cid):
    return make_inputs(CASE_BY_ID[cid])


# ---- mutants ------------------------------------------------------------------------------------------------------------------
def lost_unit(case):
    """how many elements a mutant loses: one; a set of more than grad_entries.LONGDOUBLE_POINTS points a tile of 64, as the
    tile-loop cases of grad_entries do (one of 16 000 points moves an entry by less than plain float32 rounding)"""
    return 64 if n_points(case) > ge.LONGDOUBLE_POINTS else 1


def mutants(case):
    """-> {name: restatement of a wrong computation}, each on the case's own inputs with one element (lost_unit) wrong, in
    float64: a mutant has to stand 10 x above a bound of a few hundred u, so its own rounding (1e-16) does not matter
      colloc   the last collocation point dropped (the denominator of the full set kept, as a kernel that loses a lane does)
      robin    the last Robin point dropped
      pair     the last pair dropped
      row      one table row replaced by the constants (the row that differs most from them)
      shift    the table shifted by one row
      source   one source value zeroed (the largest)
      swap     alpha and beta exchanged at one Robin point (where they differ most)
      tail     1 % on one trained tail entry (adr_ide)"""
    x = inputs(case["id"])
    out = {}
    run = lambda inp, **tot: restate(case, np.float64, inp, **tot)      # noqa: E731
    if case["kind"] == "adr_pw":
        return out
    n_f, n_b, n_w, m = case["n_f"], case["n_b"], case["n_w"], lost_unit(case)
    if n_f > m:
        y = dict(x, X_f=x["X_f"][:-m], s=None if x["s"] is None else x["s"][:-m], K=None if x["K"] is None else x["K"][:-m])
        out["colloc"] = run(y, n_f_total=n_f)
    if case["kind"] == "adr_ide":
        ref = dict(_restated(case["id"], "f64"))
        k = max((k for k in range(6) if (case["mask"] >> k) & 1), key=lambda k: ref["A"][-6 + k])
        g = np.array(ref["grad"])
        g[-6 + k] *= 1.01
        out["tail"] = dict(ref, grad=g)
        return out
    if n_w >= 2:
        out["robin"] = run(dict(x, robin=tuple(a[:-1] for a in x["robin"])), n_w_total=n_w)
    if n_w >= 1:
        X_w, al, be, g = x["robin"]
        j = int(np.argmax(np.abs(np.abs(al) - np.abs(be))))
        al2, be2 = np.array(al), np.array(be)
        al2[j], be2[j] = be[j], al[j]
        out["swap"] = run(dict(x, robin=(X_w, al2, be2, g)))
    if n_b >= 2:
        out["pair"] = run(dict(x, X_lo=x["X_lo"][:-1], X_hi=x["X_hi"][:-1]), n_b_total=n_b)
    if x["K"] is not None and n_f > m:
        K = np.array(x["K"])
        far = np.argsort(-np.max(np.abs(K - np.asarray(case["coeffs"])), axis=1), kind="stable")[:m]
        K[far] = case["coeffs"]
        out["row"] = run(dict(x, K=K))
        out["shift"] = run(dict(x, K=np.roll(x["K"], 1, axis=0)))
    if x["s"] is not None:
        s = np.array(x["s"])
        s[np.argsort(-np.abs(s), kind="stable")[:m]] = 0.0
        out["source"] = run(dict(x, s=s))
    return out


def bound(cid, dtype_name, quantity="grad"):
    """the largest allowance of the case's paths x the yardstick: what a mutant has to exceed"""
    case = CASE_BY_ID[cid]
    return max(allowance(case, p, dtype_name) for p in case["paths"][dtype_name]) * yardsticks(cid, dtype_name)[quantity]


@functools.lru_cache(maxsize=None)
def mutant_margins(cid, dtype_name):
    """-> {mutant: worst gradient entry of the mutant against the float64 restatement, on A, over bound(cid, dtype)}"""
    ref = _restated(cid, "f64")
    return {k: _scaled(m["grad"], ref["grad"], ref["A"]) / bound(cid, dtype_name) for k, m in mutants(CASE_BY_ID[cid]).items()}


def worst(dev, yard):
    """-> (largest ratio deviation / yardstick, its quantity)"""
    q = max(QUANTITIES, key=lambda k: dev[k] / yard[k])
    return dev[q] / yard[q], q


def allowance(case, path, dtype_name):
    return ge.K[(ge.family_of(path, case["layers"], dtype_name), dtype_name)]


cases()


# ---- reused contexts ------------------------------------------------------------------------------------------------------------
def config_groups(case_list):
    """-> {(engine kind, layers, dtype, path): cases}: the cases one context can be walked through (point weights are a
    feature of the adr kind's context; adr_ide is a kind of its own)"""
    out = {}
    for c in case_list:
        kind = "adr_ide" if c["kind"] == "adr_ide" else "adr"
        for d, paths in c["paths"].items():
            for p in paths:
                out.setdefault((kind, tuple(c["layers"]), d, p), []).append(c)
    return out


def bare(case):
    """the case without Robin points, source and fields: the same draws otherwise (make_inputs draws the Robin rows last)"""
    c = dict(case, n_w=0, source=False, fields=False, id=case["id"] + "-bare", plan=None)
    CASE_BY_ID.setdefault(c["id"], c)
    return CASE_BY_ID[c["id"]]


def walk(group):
    """the order one context visits a group's cases in: smallest, largest, second smallest, second largest, ... by point
    count -- every step shrinks or grows the set, and a group with plan-boundary cases crosses the n_cu-tile boundary in both
    directions -- then the first case once more (a group of one case is visited twice), then the case with the most features
    with them, without them (bare) and with them again: every feature the group has goes on, off and on"""
    by = sorted(group, key=lambda c: (n_points(c), c["id"]))
    order = []
    while by:
        order.append(by.pop(0))
        if by:
            order.append(by.pop(-1))
    order.append(order[0])
    n_feat = lambda c: (c["n_w"] > 0) + c["source"] + c["fields"]      # noqa: E731
    full = max(group, key=lambda c: (n_feat(c), -n_points(c), c["id"]))
    if n_feat(full):
        order += [full, bare(full), full]
    return order


def on_off_on(order, feature):
    """`feature` (a function of a case -> bool) is present, absent and present again somewhere along the walk"""
    seen = "".join("1" if feature(c) else "0" for c in order)
    return "1" in seen and "0" in seen[seen.index("1"):] and "1" in seen[seen.index("1"):][seen[seen.index("1"):].index("0"):]


def toggles(order, feature):
    """how often `feature` (a function of a case -> bool) changes along the walk"""
    seen = [bool(feature(c)) for c in order]
    return sum(a != b for a, b in zip(seen[:-1], seen[1:]))


FEATURES = {"robin": lambda c: c["n_w"] > 0, "source": lambda c: c["source"], "fields": lambda c: c["fields"],
            "pairs": lambda c: c["n_b"] > 0, "data": lambda c: c["n_0"] > 0, "weights": lambda c: c["kind"] == "adr_pw"}


# ---- ensembles --------------------------------------------------------------------------------------------------------------------
ENSEMBLE_SHAPES = ((0, 0, 1), (1, 5, 63), (9, 61, 65), (0, 30, 700))          # (n_b, n_0, N_f), equal counts in every member
ENSEMBLE_K = 3


@functools.lru_cache(maxsize=None)
def ensemble_members(i):
    """-> the K member cases of ensemble case i: one depth (4, 6, 8, 8), own sets, weights and coefficients from the generator,
    member 1 with gain0 = 12.  (No admission: a member is judged on max(its plain error, 32 u) whatever that is.)"""
    n_b, n_0, n_f = ENSEMBLE_SHAPES[i]
    rs = np.random.RandomState(30000 + i)
    out = []
    for k in range(ENSEMBLE_K):
        c = _spec("ens%d-m%d" % (i, k), "adr", layers_of((4, 6, 8, 8)[i]), n_b, n_0, n_f, 0, 31000 + 10 * i + k, _draw_coeffs(rs),
                  cls="gain0" if k == 1 else "ungained")
        CASE_BY_ID[c["id"]] = c
        out.append(c)
    return tuple(out)
