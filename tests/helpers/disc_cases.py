"""Shapes and inputs of the discrete-time (IRK) shape sweep of tests/test_gpu_disc.py (and of the finite-difference
check of its reference in tests/test_oracle_vs_golden.py).

A case is (model, dtype, layers, q, n0, n1, seed):
  burgers_disc      inference: set 0 carries M [n_out, q], set 1 none.  M = dt * [A; b; extra rows] cut to n_out rows
                    (n_out = q + 1 gives the reference's [A; b]; n_out = q gives A alone; n_out > q + 1 appends random
                    rows after the IRK part: a table narrower than the outputs)
  burgers_disc_ide  identification: n_out = q, both sets carry a table (dt * A and -dt * (b - A)), the weights end with
                    [lambda_1, lambda_2]
Every input is built with the oracle's own helpers (oracle/disc.py).
"""
import numpy as np

MODELS = ("burgers_disc", "burgers_disc_ide")
MAX_WIDTH = {"f64": 64, "f32": 128}          # what the LDS-resident kernels admit (engine.hip, pinn_create)
MAX_DENSE = 16                               # dense layers incl. the output layer (kernels_generic.h)
MAX_SET = 1 << 24                            # points per stage set (pinn_disc_set_stage)


def accepted(model, dtype, layers, q, n0, n1):
    """The engine's own admission rules for a discrete-time model, plus the sweep's model conventions."""
    W, H, n_out = layers[1], len(layers) - 2, layers[-1]
    return (model in MODELS and dtype in MAX_WIDTH and layers[0] == 1 and H >= 1 and H + 1 <= MAX_DENSE
            and all(v == W for v in layers[1:-1]) and 1 <= W <= MAX_WIDTH[dtype]
            and 1 <= q <= n_out and (model == "burgers_disc" or n_out == q)
            and 0 <= n0 <= MAX_SET and 0 <= n1 <= MAX_SET and n0 + n1 >= 1)


def _inf(dtype, W, H, q, n0, n1, seed, n_out=None):
    return ("burgers_disc", dtype, [1] + [W] * H + [q + 1 if n_out is None else n_out], q, n0, n1, seed)


def _ide(dtype, W, H, q, n0, n1, seed):
    return ("burgers_disc_ide", dtype, [1] + [W] * H + [q], q, n0, n1, seed)


def _both(make, *a):
    return [make("f64", *a), make("f32", *a)]


def fixed_cases():
    """The edge cases the issue names.  Comments: the path of kernels_disc.h each one reaches."""
    c = []
    # H == 1: k_disc_fwd loads the output-layer chunk at once, k_disc_bwd_hidden skips its H > 1 prefetch / stash
    c += _both(_inf, 20, 1, 8, 15, 33, 11)             # 1 chunk
    c += _both(_inf, 64, 1, 64, 16, 16, 12)            # n_out 65: 2 chunks, the last one column wide
    c += _both(_inf, 17, 1, 1, 1, 0, 13, 1)            # n_out 1, table [1, 1], one point, set 1 empty
    c += [_inf("f32", 128, 1, 32, 0, 17, 14)]          # NT = 8, H = 1, set 0 empty (removed with its table)
    c += _both(_ide, 20, 1, 9, 16, 16, 15)             # identification, H = 1
    # output chunks: ldo = 64 ceil(n_out / 64); k_disc_bwd_hidden sums 1, 2, 2, 3, 4, 5 chunk partials
    for i, n_out in enumerate((64, 65, 128, 129, 193, 257)):
        c += _both(_inf, 32, 2, n_out - 1, 37, 20, 20 + i)
    c += _both(_ide, 24, 2, 129, 40, 23, 30)          # lamp over 3 chunks
    c += _both(_ide, 32, 3, 257, 33, 15, 31)          # lamp over 5 chunks
    # a table narrower than the outputs: q = 10 of 65 outputs, rows 11..64 of the table random
    c += _both(_inf, 32, 2, 10, 33, 16, 40, 65)
    # hidden widths at the 16-wide MFMA tile edges (NT = 4), then NT = 8 in float32
    for i, (W, H) in enumerate(((1, 2), (15, 3), (16, 2), (17, 3), (63, 2), (64, 3))):
        c += _both(_inf, W, H, 12, 15 + i, 33, 50 + i)
    for i, W in enumerate((65, 127, 128)):
        c += [_inf("f32", W, 2 + i % 2, 20, 16, 16, 60 + i)]
    # point counts: more groups than the MI355X has CUs; a single point; groups that are not full
    c += _both(_inf, 48, 2, 30, 4100, 777, 70)
    c += _both(_ide, 40, 2, 30, 4100, 777, 71)
    c += _both(_ide, 16, 3, 12, 1, 40, 72)             # identification with a 1-point set
    c += _both(_ide, 16, 2, 12, 0, 17, 73)             # identification with set 0 empty (removed with its table)
    # depth 6
    c += _both(_ide, 24, 6, 30, 40, 33, 80)
    c += _both(_inf, 50, 6, 40, 15, 1, 81)
    return c


def random_cases(n=12, seed=20261016):
    rs = np.random.RandomState(seed)
    out = []
    for i in range(n):
        model = MODELS[rs.randint(2)]
        dtype = ("f64", "f32")[rs.randint(2)]
        W = int(rs.randint(1, MAX_WIDTH[dtype] + 1))
        H = int(rs.randint(1, 7))
        q = int(rs.randint(1, 301))
        n0, n1 = int(rs.randint(0, 3001)), int(rs.randint(0, 3001))
        if n0 + n1 == 0:
            n0 = 1
        n_out = q + 1 if model == "burgers_disc" else q
        out.append((model, dtype, [1] + [W] * H + [n_out], q, n0, n1, 1000 + i))
        assert accepted(*out[-1][:6]), out[-1]
    return out


def build(model, layers, q, n0, n1, seed, lb=-1.0, ub=1.0):
    """-> (sets, w, nu): stage sets as disc_set_stage takes them (x [n,1], target [n,1], M or None), the flat weights
    (with [lambda_1, lambda_2] appended for identification) and the viscosity (None for identification).  lb, ub: the x
    range the points are drawn from (tests/helpers/boxes.py)."""
    from oracle import disc
    rs = np.random.RandomState(seed)
    W, n_out = layers[1], layers[-1]
    A, b, _ = disc.gauss_legendre_butcher(q)
    dt = rs.uniform(0.1, 0.8)
    x0, x1 = rs.uniform(lb, ub, (n0, 1)), rs.uniform(lb, ub, (n1, 1))
    u0 = -np.sin(np.pi * x0) + 0.1 * rs.standard_normal((n0, 1))
    u1 = -np.sin(np.pi * x1) + 0.1 * rs.standard_normal((n1, 1))
    n_net = sum(a * c + c for a, c in zip(layers[:-1], layers[1:]))
    w = 0.9 / np.sqrt(W) * rs.standard_normal(n_net)
    if model == "burgers_disc":
        T = np.vstack([A, b[None, :]])
        if n_out > q + 1:
            T = np.vstack([T, rs.standard_normal((n_out - q - 1, q)) / q])
        sets = disc.inference_sets(x0, u0, x1, dt, T[:n_out])
        return sets, w, rs.uniform(0.001, 0.1)
    sets = disc.identification_sets(x0, u0, x1, u1, dt, A, b[None, :])
    return sets, np.concatenate([w, [rs.uniform(0.5, 1.5), rs.uniform(-7.0, -4.0)]]), None


def case_id(c):
    model, dtype, layers, q, n0, n1, _ = c
    return "%s-%s-%s-q%d-%d+%d" % ("ide" if model.endswith("ide") else "inf", dtype,
                                   "x".join(str(v) for v in layers[1:]), q, n0, n1)
