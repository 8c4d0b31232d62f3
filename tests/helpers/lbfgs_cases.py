"""Shared table of L-BFGS cases that drive every stop rule and the curvature branch of custom_lbfgs.py:39-236.

Each case is a small problem (net, start, data) plus the optimiser's settings.  The tolerances were chosen by running
the traced oracle (oracle.optim.lbfgs(trace=...)) on the CPU so that the case ends with its stop code and so that every
floating-point comparison the oracle makes on the way -- y.s against 1e-10, gtd against -tolX, sum|g| against tolFun,
sum|d t| and |f - f_old| against tolX, in every iteration, the ones that do not fire included -- is decided with a
relative margin of at least MARGIN.  A device that rounds differently from numpy cannot flip such a decision, so the GPU
tests (tests/test_gpu_lbfgs_branches.py) may compare stop codes and iteration lists exactly.  tests/test_lbfgs_cases.py
checks the table on the CPU.

tests/ is no package: the test files put this directory on sys.path and `import lbfgs_cases`.  Every run of the oracle
here is float64 numpy on the CPU; a case takes well under a second.
"""
import collections

import numpy as np

NU = 0.01 / np.pi
LB, UB = np.array([-1.0, 0.0]), np.array([1.0, 0.99])
MARGIN = 0.01
YS_MIN = 1e-10                         # custom_lbfgs.py:102
DEFAULT_TOL_FUN = float(np.finfo(float).eps)
DEFAULT_TOL_X = 1e-19

# A problem: pde, layers, collocation / data / boundary point counts, the seed of the points and the start, the start's
# scale (times glorot) and the targets' scale.  Small scales make the loss surface flat enough that y.s falls below 1e-10
# (rejected pairs) and that the tolerance tests fire early.
Problem = collections.namedtuple("Problem", "pde layers n_f n_u n_b seed w_scale u_scale")

PROBLEMS = {
    "b501": Problem("burgers", [2, 20, 20, 1], 200, 32, 0, 11, 1.0, 1.0),
    "b501_big": Problem("burgers", [2, 20, 20, 1], 200, 32, 0, 11, 1.0, 30.0),
    "b501_c1": Problem("burgers", [2, 20, 20, 1], 200, 32, 0, 12, 0.1, 1e-3),
    "b501_c3": Problem("burgers", [2, 20, 20, 1], 200, 32, 0, 12, 0.1, 1e-2),
    "b3021": Problem("burgers", [2] + [20] * 8 + [1], 256, 48, 0, 14, 1.0, 1.0),
    "ide3023": Problem("burgers_ide", [2] + [20] * 8 + [1], 0, 200, 0, 16, 1.0, 1.0),
    "b5301": Problem("burgers", [2, 50, 50, 50, 1], 128, 32, 0, 17, 1.0, 1.0),
    "s30802": Problem("schrodinger", [2, 100, 100, 100, 100, 2], 64, 32, 16, 18, 1.0, 1.0),
}


def n_params(layers, pde):
    return sum(a * b + b for a, b in zip(layers[:-1], layers[1:])) + (2 if pde == "burgers_ide" else 0)


_built = {}


def problem(name):
    """-> dict(pde, layers, w0, X_f, X_u, u, X_lb, X_ub, loss_grad): loss_grad(w) -> (loss, flat grad), the oracle's"""
    if name in _built:
        return _built[name]
    from oracle import init, pde
    p = PROBLEMS[name]
    rs = np.random.RandomState(p.seed)
    pts = lambda n: np.column_stack([rs.uniform(LB[0], UB[0], n), rs.uniform(LB[1], UB[1], n)])
    X_f, X_u = pts(p.n_f), pts(p.n_u)
    n_out = p.layers[-1]
    u = p.u_scale * np.column_stack([-np.sin(np.pi * X_u[:, 0]) * np.exp(-X_u[:, 1]),
                                     np.cos(np.pi * X_u[:, 0]) * (1.0 - X_u[:, 1])][:n_out])
    w0 = p.w_scale * init.glorot_flat(p.layers, seed=p.seed)
    X_lb = X_ub = None
    if p.pde == "burgers":
        lg = lambda w: pde.burgers_loss_grad(w, p.layers, LB, UB, X_f, X_u, u, NU)[:2]
    elif p.pde == "burgers_ide":
        w0 = np.concatenate([w0, [0.6, -4.5]])
        lg = lambda w: pde.burgers_ide_loss_grad(w, p.layers, LB, UB, X_u, u)[:2]
    else:
        tb = rs.uniform(LB[1], UB[1], (p.n_b, 1))
        X_lb, X_ub = np.hstack([0 * tb + LB[0], tb]), np.hstack([0 * tb + UB[0], tb])
        lg = lambda w: pde.schrodinger_loss_grad(w, p.layers, LB, UB, X_f, X_lb, X_ub, X_u, u)[:2]
    assert w0.size == n_params(p.layers, p.pde)
    _built[name] = dict(name=name, pde=p.pde, layers=list(p.layers), w0=w0, X_f=X_f, X_u=X_u, u=u, X_lb=X_lb,
                        X_ub=X_ub, loss_grad=lg)
    return _built[name]


# A case: the problem, the optimiser's settings, the stop code it must end with, and whether it must keep AND reject
# curvature pairs.  `f32` marks the cases whose outcome does not depend on rounding (codes 7, 2 on iteration 1, 3, 1),
# which the float32 kernels must reproduce exactly.
Case = collections.namedtuple("Case", "name problem max_iter lr n_corr tol_fun tol_x max_eval code mixed f32")


def _case(name, problem, max_iter, code, lr=0.8, n_corr=50, tol_fun=DEFAULT_TOL_FUN, tol_x=DEFAULT_TOL_X,
          max_eval=0.0, mixed=False, f32=False):
    return Case(name, problem, max_iter, lr, n_corr, tol_fun, tol_x, max_eval, code, mixed, f32)


CASES = [
    # code 7: sum|g0| = 25.3 <= tolFun
    _case("c7_initial", "b501", 20, 7, tol_fun=50.0, f32=True),
    # code 2 on iteration 1: gtd = -|g0|^2 = -3.25 > -tolX
    _case("c2_first", "b501", 20, 2, tol_x=10.0, f32=True),
    # code 2 later: gtd on iteration 5 = -3.8e-4 (every earlier tolX test >= 6.7e-3)
    _case("c2_late", "b501", 20, 2, tol_x=5.144e-3),
    # code 3: max_eval below 1.25 max_iter = 25, integer (stops on iteration 11) and not (n_eval 10, iteration 9)
    _case("c3_int", "b501", 20, 3, max_eval=12.0, f32=True),
    _case("c3_frac", "b501", 20, 3, max_eval=9.5, f32=True),
    # code 4 on iteration 6 (3021 parameters)
    _case("c4_b3021", "b3021", 20, 4, tol_fun=7.704),
    # code 5 on iteration 4: large targets and a short step make sum|d t| the smallest tolX quantity
    _case("c5_big", "b501_big", 20, 5, lr=0.1, tol_x=0.6359),
    # tolFun and step < tolX both hold behind iteration 1: code 4, because tolFun is tested first (:200-209)
    _case("c4_before_5", "b501", 20, 4, tol_fun=20.99, tol_x=1.803),
    # code 6 on iteration 5
    _case("c6_b501", "b501", 20, 6, tol_x=1.138e-3),
    # code 1 on very short runs: max_iter = 1 (no evaluation at all after the initial one) and 2 (one logged iteration)
    _case("c1_max1", "b501", 1, 1, f32=True),
    _case("c1_max2", "b501", 2, 1, f32=True),
    # max_iter = 0: the reference returns None, the engine reports done and changes nothing
    _case("c0_max0", "b501", 0, 1, f32=True),
    # curvature: pairs kept and rejected; the ring of 1 and of 3 wraps between rejections (3: K..KrKKr..r)
    _case("cv_n1", "b501_c1", 30, 1, n_corr=1, mixed=True),
    _case("cv_n3", "b501_c3", 35, 1, n_corr=3, mixed=True),
    _case("cv_n61", "b501_c3", 30, 1, n_corr=61, mixed=True),    # the largest ring compact mode takes (62 slots)
    _case("cv_n62", "b501_c3", 30, 1, n_corr=62, mixed=True),    # compact mode falls back to mode 0
    # kernel shape limits: k_lbc_dots<2> (n <= 4096) with the identification lambdas, k_lbc_dots<1> above 4096, and the
    # Schrodinger net
    _case("c6_b3021", "b3021", 20, 6, tol_x=2.289e-3),
    _case("c2_ide3023", "ide3023", 20, 2, tol_x=1.751e-2),
    _case("c4_b5301", "b5301", 20, 4, tol_fun=4.327),
    _case("c6_b5301", "b5301", 20, 6, tol_x=5.688e-4),
    _case("c2_s30802", "s30802", 20, 2, tol_x=7.636e-4),
    _case("c4_s30802", "s30802", 20, 4, tol_fun=11.52),
]


def by_name(name):
    for c in CASES:
        if c.name == name:
            return c
    raise KeyError(name)


def run_oracle(case):
    """-> (oracle result dict or None for max_iter == 0, trace dict)"""
    from oracle import optim
    p = problem(case.problem)
    trace = {}
    res = optim.lbfgs(lambda w: p["loss_grad"](w), p["w0"].copy(), case.max_iter, case.lr, case.n_corr,
                      tol_fun=case.tol_fun, tol_x=case.tol_x, max_eval=case.max_eval or None, trace=trace)
    return res, trace


def _rel(a, b):
    return abs(a - b) / max(abs(a), abs(b), 1e-300)


def decisions(case, trace):
    """every floating-point comparison the oracle made: list of (what, iteration, relative margin)"""
    out = []
    if trace["g0_abs"] is not None:
        out.append(("sum|g0| vs tolFun", 0, _rel(trace["g0_abs"], case.tol_fun)))
    for r in trace["iters"]:
        k = r["n_iter"]
        if r["ys"] is not None:
            out.append(("y.s vs 1e-10", k, _rel(r["ys"], YS_MIN)))
        if r["gtd"] is not None:
            out.append(("gtd vs -tolX", k, _rel(r["gtd"], -case.tol_x)))
        if r["g_abs"] is not None:
            out.append(("sum|g| vs tolFun", k, _rel(r["g_abs"], case.tol_fun)))
        if r["s_abs"] is not None:
            out.append(("sum|d t| vs tolX", k, _rel(r["s_abs"], case.tol_x)))
        if r["df"] is not None:
            out.append(("|f - f_old| vs tolX", k, _rel(r["df"], case.tol_x)))
    return out


def stop_iteration(trace):
    """the iteration on which the run stopped (0: before the first, i.e. code 7 or max_iter == 0)"""
    return trace["iters"][-1]["n_iter"] if trace["iters"] else 0


def engine_done(case, trace):
    """the engine's `done` for the case: the oracle's reason, and 1 for max_iter == 0 (the reference returns None, the
    engine reports that it is done)"""
    return 1 if case.max_iter == 0 else trace["reason"]


# An ensemble of four 3021-parameter members, each with its own points, data and start, that stop with four different
# codes on four different iterations inside one lbfgs_run chunk.  tolFun, tolX, max_eval and n_corr are shared; max_iter
# and lr are per member.  Member: (problem, max_iter, lr, done, stop iteration).
PROBLEMS.update({
    "b3021_tiny": Problem("burgers", [2] + [20] * 8 + [1], 256, 48, 0, 15, 0.05, 1e-3),
    "b3021_big": Problem("burgers", [2] + [20] * 8 + [1], 256, 48, 0, 19, 1.0, 3.0),
})
ENSEMBLE = dict(n_corr=50, tol_fun=7.704, tol_x=DEFAULT_TOL_X, max_eval=12.0, members=[
    ("b3021", 20, 0.8, 4, 6),
    ("b3021", 3, 0.8, 1, 3),
    ("b3021_tiny", 20, 0.8, 7, 0),
    ("b3021_big", 20, 0.5, 3, 11),
])


def ensemble_cases():
    """the ensemble's members as Cases (max_eval and the tolerances shared)"""
    e = ENSEMBLE
    return [Case("ens%d" % k, pr, mi, lr, e["n_corr"], e["tol_fun"], e["tol_x"], e["max_eval"], code, False, False)
            for k, (pr, mi, lr, code, _) in enumerate(e["members"])]
