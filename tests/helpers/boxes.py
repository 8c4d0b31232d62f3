"""Domains other than x in [-1, 1], t from 0 (test infrastructure, numpy only).

Every kernel takes the domain as lbx, lbt, sx = 2 / (ub_x - lb_x), st = 2 / (ub_t - lb_t) and writes out its own copy of
the first layer and of the derivative seeds h_x = sx, h_t = st.  On [-1, 1] x [0, 1] the x-map is the identity and lb_t is
0: a kernel that drops lb_t, hard-wires lb_x = -1, applies sx once in u_xx or leaves it out of a Robin point's u_x computes
the same numbers there (tests/test_boxes_host.py asserts exactly that).  The boxes below have sx != 1, lb_t != 0 and lb_x not
in {-1, 0}; B and C also have sx != st.

  BOXES        A ... D, (lb, ub) in (x, t)
  OLD          [-1, 1] x [0, 1], where the four errors above are invisible
  NARROW       [-1e-3, 1e-3] x [1000, 1000.01]: float64 only (below)
  BOXES_1D     the discrete-time models' x ranges
  points, walls, points_1d

float32.  A context stores coordinates as float32, not coordinates relative to lb, so s (x - lb) carries the rounding of x
itself: half an ulp of |x| over a box of width ub - lb.  A, B and C keep the plain float32 sweep at the floor of 32 u of an
entry's scale; D (x near 100, width 1) loses 7 bits and sits near 100 u; NARROW (t near 1000, width 0.01) is at several
thousand u.  D is therefore judged in float32 against its own yardstick only (grad_entries.judge measures it), NARROW in
float64 only.  tests/test_boxes_host.py measures and prints the figures.
"""
import numpy as np

BOXES = {
    "A": (np.array([0.25, 0.5]), np.array([1.75, 2.0])),
    "B": (np.array([-3.0, -2.0]), np.array([-2.4, -0.7])),
    "C": (np.array([3.0, 10.0]), np.array([3.5, 12.0])),
    "D": (np.array([100.0, -50.0]), np.array([101.0, -49.0])),
}
OLD = (np.array([-1.0, 0.0]), np.array([1.0, 1.0]))
NARROW = (np.array([-1e-3, 1000.0]), np.array([1e-3, 1000.01]))
BOXES_1D = {"p": (np.array([0.3]), np.array([2.1])), "n": (np.array([-4.0]), np.array([-3.5]))}
for _lb, _ub in list(BOXES.values()) + [OLD, NARROW] + list(BOXES_1D.values()):
    _lb.setflags(write=False)
    _ub.setflags(write=False)

# A and D are as wide in x as in t, so sx == st there (4/3 and 2): exchanged scales are the right gradient on them, and it is
# B and C (0.6 x 1.3, 0.5 x 2) that see that error.  Every box has sx != 1, lb_t != 0 and lb_x not in {-1, 0}.
EQUAL_SCALES = ("A", "D")
FLOAT32_BOXES = ("A", "B", "C")          # at the 32 u floor in float32; D: own yardstick only


def scales(lb, ub):
    """(sx, st) as the engine forms them"""
    return 2.0 / (np.asarray(ub, dtype=np.float64) - np.asarray(lb, dtype=np.float64))


def points(rs, n, lb, ub):
    """n uniform points of the box, [n, 2]"""
    return np.column_stack([rs.uniform(lb[0], ub[0], n), rs.uniform(lb[1], ub[1], n)])


def walls(rs, n, lb, ub):
    """n pairs at common times on the walls x = lb_x and x = ub_x of the box -> (X_lo, X_hi), each [n, 2]"""
    tb = rs.uniform(lb[1], ub[1], n)
    return np.column_stack([np.full(n, lb[0]), tb]), np.column_stack([np.full(n, ub[0]), tb])


def wall_points(rs, n, lb, ub):
    """n points alternating between the two walls (Robin points) -> [n, 2]"""
    j = np.arange(n)
    return np.column_stack([np.where(j % 2, ub[0], lb[0]), rs.uniform(lb[1], ub[1], n)])


def points_1d(rs, n, lb, ub):
    """n uniform points of a 1-D box, [n, 1]"""
    return rs.uniform(lb[0], ub[0], (n, 1))


def unit(X, lb, ub):
    """the points in [-1, 1] x [0, 1]: where the adr family's data, source and coefficient fields are stated
    (tests/helpers/adr_fuzz.py), so that a box at t = -50 does not put e^-t into a table"""
    X = np.asarray(X, dtype=np.float64)
    return np.column_stack([2.0 * (X[:, 0] - lb[0]) / (ub[0] - lb[0]) - 1.0, (X[:, 1] - lb[1]) / (ub[1] - lb[1])])


ADR_COEFFS = (0.3, -0.8, 0.02, 0.6, -0.4, 1.5)


def adr_inputs(rs, layers, lb, ub, n_b, n_0, n_f, n_w=0, source=False, fields=False, coeffs=ADR_COEFFS):
    """adr_fuzz.make_inputs on a box: weights 0.9 / sqrt(W) N(0, 1), uniform points, wall pairs and Robin points on the box's
    own walls; data, source and fields are adr_fuzz's functions of the unit coordinates"""
    import adr_fuzz as af
    W = layers[1]
    w = 0.9 / np.sqrt(max(W, 2)) * rs.standard_normal(sum(a * b + b for a, b in zip(layers[:-1], layers[1:])))
    X_f, X_u = points(rs, n_f, lb, ub), points(rs, n_0, lb, ub)
    xu = unit(X_u, lb, ub)
    u = (xu[:, 0:1] ** 2) * np.cos(np.pi * xu[:, 0:1]) * np.exp(-xu[:, 1:2])
    X_lo, X_hi = walls(rs, n_b, lb, ub)
    robin = None
    if n_w:
        j = np.arange(n_w)
        X_w = wall_points(rs, n_w, lb, ub)
        alpha, beta, g = rs.uniform(-1.5, 1.5, n_w), rs.uniform(-1.5, 1.5, n_w), rs.uniform(-1, 1, n_w)
        alpha[j % 5 == 4] = 0.0
        beta[(j % 7 == 6) & (alpha != 0.0)] = 0.0
        robin = (X_w, alpha, beta, g)
    xf = unit(X_f, lb, ub)
    return {"w": w, "X_f": X_f, "X_u": X_u, "u": u, "X_lo": X_lo, "X_hi": X_hi, "robin": robin,
            "s": af.cells.source_of(xf) if source else None, "K": af.fields_of(xf, coeffs) if fields else None}


# ---- what a kernel with a wrong map computes, stated as another box -------------------------------------------------------
# A restatement forms lbd = lb and s = 2 / (ub - lb).  Three of the wrong maps are the right map of another box:
def lbt_as_zero(lb, ub):
    """(a) lb_t taken as 0, st kept"""
    return np.array([lb[0], 0.0]), np.array([ub[0], 0.0 + (ub[1] - lb[1])])


def lbx_as_minus_one(lb, ub):
    """(b) lb_x taken as -1, sx kept"""
    return np.array([-1.0, lb[1]]), np.array([-1.0 + (ub[0] - lb[0]), ub[1]])


def scales_swapped(lb, ub):
    """(d) sx and st exchanged, lb kept"""
    return np.array(lb, dtype=np.float64), np.array([lb[0] + (ub[1] - lb[1]), lb[1] + (ub[0] - lb[0])])
