"""Shapes, restatements and bounds for the sweep of the optimiser kernels (csrc/kernels_optim.h: reduce_column,
k_reduce_rows, k_reduce_adam, k_adam, k_cast_weights, k_zero_list, k_lbfgs_step, k_lbfgs_post, k_lbc_dots<1|2>,
k_lbc_coef_apply) over parameter counts n placed at their block edges.  tests/test_optim_tail_host.py pins this file on
the CPU, tests/test_gpu_optim_tail.py uses it on the device.

The shape table.  The only size these kernels see is n = n_theta (and R = n + 4), so a case is a net chosen for its
parameter count:
    continuous nets     n = 3 W + (H - 1) W (W + 1) + n_out (W + 1) + tail       tail: burgers_ide 2, adr_ide 6, else 0
    discrete inference  n = 2 W + (H - 1) W (W + 1) + n_out (W + 1)              n_out free (q = 4: a narrow table)
n_cont / n_disc state the formulas, find(n) enumerates every admissible net with a given count (4097 has none: see
test_optim_tail_host.py), TABLE lists the chosen nets with the seam each one sits on.  Point sets are the smallest that
keep every point class alive; weights are 0.9 / sqrt(W) x normal as in tests/test_gpu_fuzz.py.

Adam.  adam_wide() evaluates the five statements of adam_entry in np.longdouble:
    mi = m + (1 - b1) (g - m);  vi = v + (1 - b2) (g g - v);  m = mi;  v = vi;  theta = theta - alpha mi / (sqrt(vi) + eps)
with alpha the float64 number the host hands the kernel (adam_alpha: lr sqrt(1 - b2^t) / (1 - b1^t) in float64, as
adam_issue and oracle.optim.Adam form it -- its own rounding is an input here, not an error).  The comparison starts
every step from the device's weights and gradient; m and v are carried in longdouble over the steps.

K_A, derived (u = 2^-53, every float64 operation is off by at most u of its result; the longdouble side's 2^-64 is
neglected; 1 - b1 and 1 - b2 are exact for b1 = 0.9, b2 = 0.999 by Sterbenz's lemma):
    m   per step: the subtraction, the product, the sum: 3 u of m (the two addends have one sign while the gradient
        entry keeps its sign, so nothing is amplified; the error carried in is scaled by b1 < 1).  m_0 = 0 is exact.
        Six steps: 18 u.
    v   per step: g g, the subtraction, the product, the sum: 4 u of v; six steps: 24 u.  sqrt halves it and rounds
        once: 13 u; + eps (exact, same sign) rounds once more: 14 u of the denominator.
    step = alpha mi / denominator: one product, one quotient: 18 + 14 + 2 = 34 u of |step|.
    theta - step rounds once: u of the new weight, at most u (|theta| + |step|).
    |error| <= 35 u |step| + u |theta|  <=  K_A u (|theta| + |step|)  with  K_A = 36 (35, and the second-order terms).
The assumption is the sign of the entry over the six steps; a gradient entry that changes sign lets m cancel, and the
bound then holds for it only through the slack between this worst case and what six roundings add up to.  The host test
holds oracle.optim.Adam (plain float64 numpy) on the same gradients to the same allowance.

L-BFGS.  Lbfgs restates oracle.optim.lbfgs (utils/custom_lbfgs.py:39-236) statement by statement as an object that is
fed one evaluation at a time, with a dtype argument: begin(f, g), step() -> (t, d) or None, evaluated(f, g).  In
float64, form "vector", closed over the oracle's loss it IS oracle.optim.lbfgs bit for bit (run_closed; pinned by the host
test).  Form "compact" restates what k_lbc_coef_apply computes, in its own algebra: the Gram entries s_a.y_b, y_a.y_b,
s_a.g, y_a.g, g.g, the two-loop recursion on scalars, d = cg g + sum_j (cy_j y_j + cs_j s_j).  On the device test the
object is fed the device's own gradients (from a twin context), its own d and t form the history, and the device's next
iterate is compared with x_k(device) + t d(longdouble).

The yardstick of that comparison is measured on the restatement, never on the device: the error of the same restatement
in float64 numpy against longdouble, max-norm over the step t d, floored at 32 u of the largest step entry, plus u / 2 of
the largest |x| (the rounding of x + t d itself): yardstick().
"""
import collections
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

U = 2.0 ** -53
K_A = 36.0
EPS = float(np.finfo(float).eps)
TOL_X = 1e-19
YS_MIN = 1e-10
MARGIN = 0.01                                    # the rule of tests/test_lbfgs_cases.py
NU = 0.01 / np.pi
LB, UB = np.array([-1.0, 0.0]), np.array([1.0, 0.99])
DLB, DUB = [-1.0], [1.0]
N_F, N_U, N_B, N_STAGE, DISC_Q = 96, 24, 8, 16, 4
ADAM = dict(lr=1e-3, b1=0.9, b2=0.999, steps=6, eps=(1e-7, 1e-3))
LBFGS = dict(lr=0.8, iters=8, max_iter=20, n_corr=(3, 50))
# adr_ide: two trained, four frozen coefficients.  The six are the last entries of theta, so with n = 1027 and 4099 the
# elements behind the stride (1024 ...) and in k_lbc_dots<1>'s tail loop (4096 ...) are r1, r2, r3: the first and the last of
# them are the trained ones, so that a tail element that is dropped or misplaced moves the iterate
ADR_TRAINED = ("r1", "r3")
ADR_COEFFS = [0.3, -0.8, 0.02, 0.6, -0.4, 1.5]

TAIL = {"burgers": 0, "schrodinger": 0, "adr": 0, "burgers_ide": 2, "adr_ide": 6}
N_OUT = {"burgers": 1, "schrodinger": 2, "adr": 1, "burgers_ide": 1, "adr_ide": 1}
MAX_H = 15                                       # 16 dense layers, the output layer included (kernels_generic.h)
MAX_W, MAX_W_DISC = 128, 64                      # float64 admits 64 for the discrete-time kernels


def n_cont(pde, W, H):
    return 3 * W + (H - 1) * W * (W + 1) + N_OUT[pde] * (W + 1) + TAIL[pde]


def n_disc(W, H, n_out):
    return 2 * W + (H - 1) * W * (W + 1) + n_out * (W + 1)


def find(n):
    """every net the engine admits (both dtypes) with exactly n parameters -> [(pde, W, H, n_out)]"""
    out = []
    for W in range(1, MAX_W + 1):
        for H in range(1, MAX_H + 1):
            for pde in sorted(TAIL):
                if n_cont(pde, W, H) == n:
                    out.append((pde, W, H, N_OUT[pde]))
            if W <= MAX_W_DISC:
                rest = n - 2 * W - (H - 1) * W * (W + 1)
                if rest >= W + 1 and rest % (W + 1) == 0 and rest // (W + 1) <= 65536:
                    out.append(("burgers_disc", W, H, rest // (W + 1)))
    return out


Case = collections.namedtuple("Case", "n pde W H n_out edge also_path0")


def _c(n, pde, W, H, edge, n_out=None, also_path0=False):
    return Case(n, pde, W, H, N_OUT[pde] if n_out is None else n_out, edge, also_path0)


TABLE = [
    _c(5, "burgers", 1, 1, "n < 64: idle waves in block_sum"),
    _c(12, "schrodinger", 2, 1, "tiny, even"),
    _c(60, "schrodinger", 2, 9, "R = 64 exactly"),
    _c(61, "burgers", 15, 1, "the last reduction block holds the pad slot only"),
    _c(62, "schrodinger", 12, 1, "loss slots 62, 63 | 64 in two blocks"),
    _c(63, "burgers_ide", 15, 1, "loss slots 63 | 64, 65 in two blocks"),
    _c(65, "burgers", 16, 1, "one weight in the second block"),
    _c(127, "burgers", 9, 2, "below 128"),
    _c(129, "burgers", 32, 1, "above 128"),
    _c(192, "schrodinger", 38, 1, "n mod 64 = 0: loss slots in a block of their own"),
    _c(1536, "schrodinger", 26, 3, "n mod 64 = 0"),
    _c(255, "burgers_ide", 63, 1, "k_adam block edge, below"),
    _c(257, "burgers", 64, 1, "k_adam block edge, above"),
    _c(1021, "burgers", 15, 5, "below one stride of 1024", also_path0=True),
    _c(1023, "burgers_ide", 15, 5, "one below the stride", also_path0=True),
    _c(1027, "adr_ide", 15, 5, "three beyond the stride", also_path0=True),
    _c(2047, "burgers_disc", 2, 1, "second half of k_lbc_dots<2> empty, odd", n_out=681),
    _c(2048, "burgers_disc", 1, 1, "second half of k_lbc_dots<2> empty, full", n_out=1023),
    _c(2049, "burgers_disc", 6, 1, "one element in the second half", n_out=291),
    _c(2051, "burgers", 25, 4, "three elements in the second half"),
    _c(4093, "burgers", 31, 5, "last <2> sizes, odd"),
    _c(4095, "burgers_ide", 31, 5, "last <2> sizes, odd, the last pair half filled"),
    _c(4096, "burgers_disc", 1, 1, "last <2> size", n_out=2047),
    _c(4098, "burgers_disc", 1, 1, "first <1> sizes: tail loop of 2", n_out=2048),
    _c(4099, "adr_ide", 31, 5, "first <1> sizes: tail loop of 3"),
    _c(5117, "schrodinger", 31, 6, "tail loop below one stride"),
    _c(5121, "burgers", 20, 13, "tail loop crosses a stride by one"),
    _c(5122, "schrodinger", 40, 4, "tail loop crosses a stride by two"),
    _c(5695, "burgers", 73, 2, "float64 path 8: TileScratch slots, n mod 64 = 63", also_path0=True),
    _c(5697, "burgers_ide", 73, 2, "float64 path 8: TileScratch slots, n mod 64 = 1", also_path0=True),
    _c(6077, "schrodinger", 75, 2, "float64 path 8: TileScratch slots, n mod 64 = 61", also_path0=True),
]
IDENTITY_N = (62, 63, 255, 257, 4095, 4099)
# the seed of a case's points and weights; moved where a stop rule or the y.s test came within MARGIN of its threshold
SEEDS = {}


def case_id(c):
    return "n%d-%s-%dx%d%s" % (c.n, c.pde, c.W, c.H, "-o%d" % c.n_out if c.pde == "burgers_disc" else "")


def by_n(n):
    for c in TABLE:
        if c.n == n:
            return c
    raise KeyError(n)


def layers_of(c):
    return [1 if c.pde == "burgers_disc" else 2] + [c.W] * c.H + [c.n_out]


def count(c):
    return n_disc(c.W, c.H, c.n_out) if c.pde == "burgers_disc" else n_cont(c.pde, c.W, c.H)


_built = {}


def build(c):
    """-> dict(case, layers, w0, the point sets, loss_grad): loss_grad(w) -> (loss, gradient), the CPU oracle's"""
    if c.n in _built:
        return _built[c.n]
    from oracle import disc, pde
    import adr_ide_ref
    import disc_cases
    seed = SEEDS.get(c.n, 7000 + c.n)
    rs = np.random.RandomState(seed)
    layers = layers_of(c)
    b = dict(case=c, layers=layers, mask=None)
    if c.pde == "burgers_disc":
        sets, w, nu = disc_cases.build("burgers_disc", layers, DISC_Q, N_STAGE, N_STAGE, seed)
        b.update(w0=w, sets=sets, nu=nu,
                 loss_grad=lambda x: disc.disc_loss_grad(x, layers, DLB, DUB, sets, nu=nu)[:2])
    else:
        n_net = sum(p * q + q for p, q in zip(layers[:-1], layers[1:]))
        w = 0.9 / np.sqrt(max(c.W, 2)) * rs.standard_normal(n_net)
        pts = lambda k: np.column_stack([rs.uniform(LB[0], UB[0], k), rs.uniform(LB[1], UB[1], k)])
        X_f, X_u = pts(N_F), pts(N_U)
        u = rs.standard_normal((N_U, c.n_out))
        tb = rs.uniform(LB[1], UB[1], (N_B, 1))
        X_lb, X_ub = np.hstack([0 * tb + LB[0], tb]), np.hstack([0 * tb + UB[0], tb])
        b.update(X_f=X_f, X_u=X_u, u=u, X_lb=X_lb, X_ub=X_ub)
        if c.pde == "burgers":
            lg = lambda x: pde.burgers_loss_grad(x, layers, LB, UB, X_f, X_u, u, NU)[:2]
        elif c.pde == "burgers_ide":
            w = np.concatenate([w, [0.6, -4.5]])
            lg = lambda x: pde.burgers_ide_loss_grad(x, layers, LB, UB, X_u, u)[:2]
        elif c.pde == "schrodinger":
            lg = lambda x: pde.schrodinger_loss_grad(x, layers, LB, UB, X_f, X_lb, X_ub, X_u, u)[:2]
        else:
            assert c.pde == "adr_ide", c.pde
            w = adr_ide_ref.pack(w, ADR_COEFFS)
            mask = adr_ide_ref.mask_of(ADR_TRAINED)
            b["mask"] = mask
            lg = lambda x: adr_ide_ref.loss_grad(x, layers, LB, UB, X_f, X_u, u, X_lb, X_ub, mask)[:2]
        b.update(w0=w, loss_grad=lg)
    assert b["w0"].size == c.n == count(c), (b["w0"].size, c.n, count(c))
    _built[c.n] = b
    return b


def frozen_entries(b):
    """flat indices of the adr_ide coefficients that are not trained ([] for the other kinds)"""
    if b["mask"] is None:
        return []
    n = b["w0"].size
    return [n - 6 + k for k in range(6) if not (b["mask"] >> k) & 1]


def make_engine(b, dtype, path=None):
    """a context with the case's sets and start; path None: the one the engine chooses"""
    import pinn_native
    c = b["case"]
    if c.pde == "burgers_disc":
        eng = pinn_native.Engine(b["layers"], DLB, DUB, pde="burgers_disc", dtype=dtype)
        for k, (x, t, M) in enumerate(b["sets"]):
            eng.disc_set_stage(k, x, t, M)
        eng.set_pde_params(b["nu"])
    else:
        eng = pinn_native.Engine(b["layers"], LB, UB, pde=c.pde, dtype=dtype)
        if c.pde != "burgers_ide":
            eng.set_collocation(b["X_f"])
        eng.set_data(b["X_u"], b["u"])
        if c.pde in ("schrodinger", "adr_ide"):
            eng.set_boundary(b["X_lb"], b["X_ub"])
        if c.pde == "burgers":
            eng.set_pde_params(NU)
        if c.pde == "adr_ide":
            eng.set_pde_trainable(b["mask"])
    if path is not None:
        eng.set_kernel_path(path)
        assert eng.kernel_path() == path
    eng.set_weights(b["w0"])
    return eng


def configs():
    """(case, dtype, path) of the device sweep: every case in both types on the engine's path, the marked ones on path 0 too"""
    out = []
    for c in TABLE:
        for dtype in ("f64", "f32"):
            out.append((c, dtype, None))
            if c.also_path0:
                out.append((c, dtype, 0))
    return out


def config_id(cfg):
    c, dtype, path = cfg
    return "%s-%s-%s" % (case_id(c), dtype, "auto" if path is None else "p%d" % path)


# ---- Adam -----------------------------------------------------------------------------------------------------------
def adam_alpha(lr, b1, b2, t):
    """the step size of step t (1-based) as the host forms it, in float64"""
    return float(lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t))


class AdamWide(object):
    """adam_entry's statements in longdouble; m and v live here"""

    def __init__(self, n, b1, b2, eps):
        L = np.longdouble
        self.b1, self.b2, self.eps = L(b1), L(b2), L(eps)
        self.m, self.v = np.zeros(n, L), np.zeros(n, L)

    def step(self, theta, g, alpha):
        """-> (new weights, the step alpha mi / (sqrt(vi) + eps)), longdouble, from float64 weights and gradient"""
        L = np.longdouble
        theta, g = np.asarray(theta, np.float64).astype(L), np.asarray(g, np.float64).astype(L)
        mi = self.m + (L(1) - self.b1) * (g - self.m)
        vi = self.v + (L(1) - self.b2) * (g * g - self.v)
        self.m, self.v = mi, vi
        step = L(alpha) * mi / (np.sqrt(vi) + self.eps)
        return theta - step, step


def adam_allowance(theta, step):
    return K_A * U * (np.abs(np.asarray(theta, np.float64)) + np.abs(step).astype(np.float64))


def adam_excess(w_new, w_ref, allow):
    """largest deviation / allowance over the entries (0 / 0 counts as 0) -> (ratio, index)"""
    dev = np.abs(np.asarray(w_new, np.float64).astype(np.longdouble) - w_ref).astype(np.float64)
    ratio = np.where(dev == 0.0, 0.0, dev / np.where(allow > 0.0, allow, 1e-300))
    i = int(np.argmax(ratio))
    return float(ratio[i]), i


# ---- L-BFGS ---------------------------------------------------------------------------------------------------------
class Lbfgs(object):
    """utils/custom_lbfgs.py:39-236 between its evaluations (oracle/optim.py restated), all arithmetic in `dtype`.
    form "vector": the two-loop recursion on vectors, the oracle's statements.  form "compact": the recursion on the
    Gram entries, k_lbc_coef_apply's algebra.  done uses LbfgsState's codes; logs, kept (one bool per curvature pair
    tested) and trace (the records of oracle.optim.lbfgs(trace=...)) are what the run decided."""

    def __init__(self, max_iter, lr, n_corr, dtype=np.float64, form="vector", tol_fun=EPS, tol_x=TOL_X, max_eval=None):
        assert form in ("vector", "compact") and max_iter >= 1
        self.max_iter, self.lr, self.n_corr, self.form = max_iter, lr, n_corr, form
        self.dt = np.dtype(dtype).type
        self.tol_fun, self.tol_x = tol_fun, tol_x
        self.max_eval = max_eval or max_iter * 1.25                 # :50
        self.n_iter = self.n_eval = self.done = 0
        self.S, self.Y, self.Hdiag = [], [], 1.0
        self.d = self.t = self.g = self.g_old = self.f = self.f_old = self.final_loss = None
        self.logs, self.kept, self.trace = [], [], []

    def _cast(self, g):
        return np.asarray(g, np.float64).astype(self.dt)

    def begin(self, f, g):                                          # :65-76
        self.f, self.g, self.n_eval = f, self._cast(g), 1
        self.g0_abs = float(np.sum(np.abs(self.g)))
        if np.sum(np.abs(self.g)) <= self.tol_fun:
            self.done = 7
        return self.done

    def _direction_vector(self, g):
        S, Y = self.S, self.Y
        k = len(S)
        ro = [1.0 / np.sum(Y[i] * S[i]) for i in range(k)]          # :121-123
        al = [0.0] * k
        q = -g
        for i in range(k - 1, -1, -1):                              # :130-133
            al[i] = np.sum(S[i] * q) * ro[i]
            q = q - al[i] * Y[i]
        r = q * self.Hdiag                                          # :136
        for i in range(k):                                          # :137-139
            be_i = np.sum(Y[i] * r) * ro[i]
            r = r + (al[i] - be_i) * S[i]
        return r, np.sum(g * r)

    def _direction_compact(self, g):
        S, Y, dt = self.S, self.Y, self.dt
        k = len(S)
        dot = lambda a, b: np.sum(a * b)
        SY = np.array([[dot(S[a], Y[b]) for b in range(k)] for a in range(k)], dtype=dt).reshape(k, k)
        YY = np.array([[dot(Y[a], Y[b]) for b in range(k)] for a in range(k)], dtype=dt).reshape(k, k)
        sg = np.array([dot(S[a], g) for a in range(k)], dtype=dt)
        yg = np.array([dot(Y[a], g) for a in range(k)], dtype=dt)
        gg = dot(g, g)
        ro = np.array([dt(1) / SY[a, a] for a in range(k)], dtype=dt)
        H = dt(self.Hdiag)
        b, yq0, al = ro * -sg, -yg, np.zeros(k, dt)
        for j in range(k - 1, -1, -1):                              # al_j = ro_j s_j.(-g - sum_{i > j} al_i y_i)
            al[j] = b[j]
            b[:j] = b[:j] - al[j] * (ro[:j] * SY[:j, j])
            yq0 = yq0 - al[j] * YY[:, j]                            # y_p.q_0, q_0 = -g - sum_j al_j y_j
        e, cs = al - ro * (H * yq0), np.zeros(k, dt)
        for j in range(k):                                          # cs_j = al_j - ro_j y_j.(H q_0 + sum_{i < j} cs_i s_i)
            cs[j] = e[j]
            e[j + 1:] = e[j + 1:] - cs[j] * (ro[j + 1:] * SY[j, j + 1:])
        cy, cg = -H * al, -H
        d = cg * g
        for j in range(k):
            d = d + (cy[j] * Y[j] + cs[j] * S[j])
        return d, cg * gg + np.sum(cy * yg + cs * sg)

    def step(self):
        """custom_lbfgs.py:81-174 up to the update: -> (t, d), x + t d is the caller's; None: stopped (done 2)"""
        assert not self.done and self.n_iter < self.max_iter
        g = self.g
        self.n_iter += 1
        rec = dict(n_iter=self.n_iter, ys=None, kept=None, gtd=None, g_abs=None, s_abs=None, df=None)
        self.trace.append(rec)
        if self.n_iter == 1:                                        # :90-95
            d = -g
            self.S, self.Y, self.Hdiag = [], [], 1.0
            gtd = np.sum(g * d)
        else:
            y = g - self.g_old                                      # :98-100
            s = self.d * self.t
            ys = np.sum(y * s)
            rec.update(ys=float(ys), kept=bool(ys > YS_MIN))
            self.kept.append(bool(ys > YS_MIN))
            if ys > YS_MIN:                                         # :102-114
                if len(self.S) == self.n_corr:
                    del self.S[0]
                    del self.Y[0]
                self.S.append(s)
                self.Y.append(y)
                self.Hdiag = ys / np.sum(y * y)
            d, gtd = self._direction_vector(g) if self.form == "vector" else self._direction_compact(g)
        self.d, self.g_old, self.f_old = d, g, self.f
        rec["gtd"] = float(gtd)
        if gtd > -self.tol_x:                                       # :154-156
            self.done = 2
            return None
        self.t = min(1.0, 1.0 / np.sum(np.abs(g))) if self.n_iter == 1 else self.lr      # :159-163
        if self.n_iter == self.max_iter:                            # :176, :192: no evaluation follows
            self.done = 1
        return self.t, d

    def evaluated(self, f, g):
        """custom_lbfgs.py:176-224 behind the evaluation at x + t d"""
        assert not self.done
        rec = self.trace[-1]
        self.f, self.g = f, self._cast(g)
        self.n_eval += 1
        if self.n_eval >= self.max_eval:                            # :195
            self.done = 3
            return self.done
        rec["g_abs"] = float(np.sum(np.abs(self.g)))
        if np.sum(np.abs(self.g)) <= self.tol_fun:                  # :200-203
            self.done = 4
            return self.done
        rec["s_abs"] = float(np.sum(np.abs(self.d * self.t)))
        if np.sum(np.abs(self.d * self.t)) <= self.tol_x:           # :206-209
            self.done = 5
            return self.done
        rec["df"] = float(abs(f - self.f_old))
        if abs(f - self.f_old) < self.tol_x:                        # :212-215
            self.done = 6
            return self.done
        self.logs.append((self.n_iter, f))                          # :217-218
        if self.n_iter == self.max_iter - 1:                        # :223-224
            self.final_loss = f
        return 0


def run_closed(opfunc, x0, max_iter, lr, n_corr, dtype=np.float64, form="vector", **kw):
    """the restatement closed over a loss: what oracle.optim.lbfgs returns (and the object, for its trace)"""
    L = Lbfgs(max_iter, lr, n_corr, dtype, form, **kw)
    x = np.array(x0, dtype=np.float64).astype(L.dt)
    f, g = opfunc(x.astype(np.float64))
    x_model, f_hist = x.copy(), [f]
    L.begin(f, g)
    while not L.done:
        td = L.step()
        if td is None:
            break
        x = x + td[0] * td[1]                                       # :174
        if L.done:                                                  # the last iteration is not evaluated
            break
        f, g = opfunc(x.astype(np.float64))
        x_model = x.copy()
        f_hist.append(f)
        L.evaluated(f, g)
    return dict(x=x, x_model=x_model, f_hist=f_hist, n_eval=L.n_eval, logs=L.logs, final_loss=L.final_loss), L


def yardstick(x_k, td_wide, td_f64):
    """-> (yardstick, the longdouble reference of the next iterate) for one step from the float64 iterate x_k"""
    L = np.longdouble
    step_w = L(td_wide[0]) * td_wide[1].astype(L)
    step_d = (td_f64[0] * td_f64[1]).astype(L)
    x_ref = np.asarray(x_k, np.float64).astype(L) + step_w
    plain = float(np.max(np.abs(step_w - step_d)))
    big = float(np.max(np.abs(step_w)))
    return max(plain, 32.0 * U * big) + 0.5 * U * float(np.max(np.abs(x_ref))), x_ref


def decisions(trace, g0_abs, tol_fun=EPS, tol_x=TOL_X):
    """every floating-point comparison of a run, as tests/helpers/lbfgs_cases.py lists them: (what, iteration, margin)"""
    rel = lambda a, b: abs(a - b) / max(abs(a), abs(b), 1e-300)
    out = [("sum|g0| vs tolFun", 0, rel(g0_abs, tol_fun))]
    for r in trace:
        for key, what, thr in (("ys", "y.s vs 1e-10", YS_MIN), ("gtd", "gtd vs -tolX", -tol_x),
                               ("g_abs", "sum|g| vs tolFun", tol_fun), ("s_abs", "sum|d t| vs tolX", tol_x),
                               ("df", "|f - f_old| vs tolX", tol_x)):
            if r[key] is not None:
                out.append((what, r["n_iter"], rel(r[key], thr)))
    return out
