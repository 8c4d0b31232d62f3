"""GPU: per-point loss weights of the adr kind (pinn_pw_*, k_fused20d<PDE_ADR, H, ., SAW>, float64, kernel path 7) against
the numpy restatement tests/helpers/adr_pw_ref.py (pinned on the CPU by tests/test_adr_pw_host.py).

    L = (1/N_f) sum lam_f^2 f^2 + (1/N_u) sum lam_u^2 (u - u*)^2 + (1/N_b) sum lam_b^2 [du^2 + du_x^2]   (one lam per pair)

Shapes: depths 4, 6, 8; N_f = 40 (padded lanes), 2048 (one tile per workgroup), 40 000 (tile loop); 0, 1, 7, 8 pairs (8 fill one
16-point wave, 7 share it with data points); N_u such that the data / collocation border falls inside a wave; one empty data
set.  Float64 criteria of the project: loss and parts 1e-12, gradient 1e-11 of its largest entry, trajectories 1e-8."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import adr_pw_ref  # noqa: E402
import adr_ref  # noqa: E402
import rad_ref  # noqa: E402

pytestmark = pytest.mark.gpu

LB, UB = adr_pw_ref.LB, adr_pw_ref.UB
# (depth, N_f, pairs, N_u): every depth at every launch plan, every pair count, 2 n_b + N_u never a multiple of 16
CASES = [(4, 40, 0, 21), (4, 2048, 7, 21), (4, 40000, 8, 37), (6, 40, 1, 0), (6, 2048, 8, 21), (6, 40000, 7, 21),
         (8, 40, 7, 21), (8, 2048, 1, 37), (8, 40000, 0, 21), (8, 40000, 7, 0)]
IDS = ["d%d-Nf%d-nb%d-nu%d" % c for c in CASES]


def rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300)


def case_of(depth, n_f, n_b, n_u, seed=5):
    return adr_pw_ref.trajectory_case(depth, seed=seed, n_f=n_f, n_u=n_u, n_b=n_b)


def make(c, coeffs, weighted=True):
    from pinn_native import Engine
    eng = Engine(c["layers"], LB, UB, pde="adr", dtype="f64")
    eng.set_pde_params(*coeffs)
    eng.set_collocation(c["X_f"])
    if len(c["X_u"]):
        eng.set_data(c["X_u"], c["u"])
    if len(c["X_lo"]):
        eng.set_boundary(c["X_lo"], c["X_hi"])
    assert eng.kernel_path() == 7
    eng.set_weights(c["w0"])
    if weighted:
        eng.pw_set(c["lam_u"], c["lam_f"], c["lam_b"])
    return eng


def ref_args(c):
    return (c["layers"], LB, UB, c["X_f"], c["X_u"], c["u"], c["X_lo"], c["X_hi"])


def lams_equal(got, want):
    return all(np.array_equal(a, b) for a, b in zip(got, want))


def lbfgs_all(eng, n, chunk=7):
    eng.lbfgs_begin(n, 0.8, 50, np.finfo(float).eps)
    out, done = [], 0
    while not done:
        _, lo, done = eng.lbfgs_run(chunk)
        out.extend(lo.tolist())
    return np.array(out)


# ---- 1. unit weights, rates 0: the plain kernel's bits --------------------------------------------------------------------
@pytest.mark.parametrize("depth,n_f,n_b,n_u", CASES, ids=IDS)
def test_unit_weights_give_the_plain_kernels_bits(depth, n_f, n_b, n_u):
    c = case_of(depth, n_f, n_b, n_u)
    co = adr_ref.ALLEN_CAHN
    plain, pw = make(c, co, weighted=False), make(c, co, weighted=False)
    pw.pw_set()                                             # NULL arrays: all ones
    pw.pw_adam_init(0.0, 0.0, 0.0)
    a, b = plain.loss_grad(), pw.loss_grad()
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    for e in (plain, pw):
        e.adam_init(1e-3, 0.9, 0.999, 1e-7)
    la, lb_ = plain.adam_run(20), pw.adam_run(20)
    assert np.array_equal(la, lb_) and np.array_equal(plain.get_weights(), pw.get_weights())
    la, lb_ = lbfgs_all(plain, 10), lbfgs_all(pw, 10)
    assert len(la) and np.array_equal(la, lb_) and np.array_equal(plain.get_weights(), pw.get_weights())
    got = pw.pw_get()
    assert [g.shape for g in got] == [(n_u,), (n_f,), (n_b,)] and all(np.all(g == 1.0) for g in got)
    plain.close()
    pw.close()


# ---- 2. random weights against the restatement ------------------------------------------------------------------------
@pytest.mark.parametrize("depth,n_f,n_b,n_u", CASES, ids=IDS)
def test_random_weights_against_the_restatement(record, depth, n_f, n_b, n_u):
    c = case_of(depth, n_f, n_b, n_u)
    co = adr_ref.ALL_NONZERO if depth == 6 else adr_ref.ALLEN_CAHN
    eng = make(c, co)
    loss, grad, terms = eng.loss_grad()
    again = eng.loss_grad()
    got = eng.pw_get()
    eng.close()
    lo, go, (mf, mu, mb), _ = adr_pw_ref.loss_grad(c["w0"], *ref_args(c), co, c["lam_u"], c["lam_f"], c["lam_b"])
    dev = dict(loss=abs(loss - lo) / lo, grad=rel(grad, go), t_f=abs(terms[0] - mf) / lo, t_u=abs(terms[1] - mu) / lo,
               t_b=abs(terms[2] - mb) / lo)
    print("adr_pw %s: %s" % (IDS[CASES.index((depth, n_f, n_b, n_u))], " ".join("%s %.2e" % kv for kv in sorted(dev.items()))))
    record(depth=depth, n_f=n_f, n_b=n_b, n_u=n_u, **dev)
    assert lams_equal(got, (c["lam_u"], c["lam_f"], c["lam_b"]))
    assert again[0] == loss and np.array_equal(again[1], grad) and np.array_equal(again[2], terms)
    assert dev["loss"] < 1e-12 and max(dev["t_f"], dev["t_u"], dev["t_b"]) < 1e-12
    assert dev["grad"] < 1e-11
    assert (terms[2] > 0) == (n_b > 0) and (terms[1] > 0) == (n_u > 0)


# ---- 3. the Adam trajectory: theta down, the three lambda classes up --------------------------------------------------------
@pytest.mark.parametrize("depth", [4, 8])
@pytest.mark.parametrize("name", ["allen_cahn", "all_nonzero"])
def test_adam_trajectory_follows_the_restatement(record, name, depth):
    """the inputs of tests/test_adr_pw_host.py's conditioning check (there: 1e-10 under a change of summation order)"""
    c = adr_pw_ref.trajectory_case(depth)
    co = adr_ref.COEFF_SETS[name]
    eng = make(c, co)
    eng.adam_init(adr_pw_ref.TRAJ_LR, 0.9, 0.999, 1e-7)
    eng.pw_adam_init(*adr_pw_ref.TRAJ_RATES)
    losses = eng.adam_run(adr_pw_ref.TRAJ_STEPS)
    w_dev, lam_dev = eng.get_weights(), eng.pw_get()
    w, lam, ref = adr_pw_ref.run_trajectory(c, co)
    dev = dict(loss=float(np.max(np.abs(losses - ref) / ref)), w=float(np.max(np.abs(w_dev - w))),
               lam_u=float(np.max(np.abs(lam_dev[0] - lam[0]))), lam_f=float(np.max(np.abs(lam_dev[1] - lam[1]))),
               lam_b=float(np.max(np.abs(lam_dev[2] - lam[2]))))
    moved = [float(np.max(np.abs(a - c[k]))) for a, k in zip(lam_dev, ("lam_u", "lam_f", "lam_b"))]
    print("adr_pw trajectory H=%d %s: %s moved %s" % (depth, name, " ".join("%s %.2e" % kv for kv in sorted(dev.items())), moved))
    record(depth=depth, name=name, **dev)
    assert max(dev.values()) < 1e-8
    assert min(moved) > 1e-4
    # a class with rate 0 is not touched: only the collocation weights move from here
    eng.pw_adam_init(0.0, 0.02, 0.0)
    eng.adam_run(5)
    after = eng.pw_get()
    assert np.array_equal(after[0], lam_dev[0]) and np.array_equal(after[2], lam_dev[2])
    assert np.max(np.abs(after[1] - lam_dev[1])) > 1e-4
    # all rates 0: nothing moves
    eng.pw_adam_init(0.0, 0.0, 0.0)
    eng.adam_run(3)
    assert lams_equal(eng.pw_get(), after)
    eng.close()


# ---- 4. only Adam moves the weights ----------------------------------------------------------------------------------------
def test_only_adam_moves_the_weights_and_lbfgs_minimises_the_weighted_loss(record):
    from oracle import optim
    c = case_of(8, 2048, 7, 37, seed=9)
    co = adr_ref.ALLEN_CAHN
    lam = (c["lam_u"], c["lam_f"], c["lam_b"])
    eng = make(c, co)
    eng.adam_init(1e-3)
    eng.pw_adam_init(0.05, 0.02, 0.01)            # rates on: still nothing but an Adam step may move a weight
    eng.loss_grad()
    lbfgs_all(eng, 5)
    rs = np.random.RandomState(1)
    X = LB + (UB - LB) * rs.uniform(size=(3000, 2))
    eng.predict(X)
    eng.error_l2(X, np.sin(3 * X[:, 0:1]))
    f_set, f_at = eng.residual(), eng.residual_at(X)
    w = eng.get_weights()
    assert lams_equal(eng.pw_get(), lam)
    # the residual calls see the unweighted f
    assert rel(f_set, adr_ref.residual(w, c["layers"], LB, UB, c["X_f"], co)) < 1e-10
    assert rel(f_at, adr_ref.residual(w, c["layers"], LB, UB, X, co)) < 1e-10

    # 25 L-BFGS iterations with the weights frozen against the numpy optimiser on the weighted restatement (1e-8, the
    # trajectory criterion tests/test_gpu_adr.py holds its L-BFGS case to)
    def fg(wv):
        l, g, _, _ = adr_pw_ref.loss_grad(wv, *ref_args(c), co, *lam)
        return l, g

    eng.set_weights(c["w0"])
    lo_all = lbfgs_all(eng, 25)
    w_model = eng.get_weights()
    res = optim.lbfgs(fg, c["w0"], 25, 0.8, 50)
    ref_l = np.array([l for _, l in res["logs"]])
    n = min(len(lo_all), len(ref_l))
    dl, dm = float(np.max(np.abs(lo_all[:n] - ref_l[:n]) / ref_l[:n])), rel(w_model, res["x_model"])
    print("adr_pw lbfgs: loss %.2e w_model %.2e (%d logged)" % (dl, dm, n))
    record(lbfgs_loss=dl, lbfgs_w_model=dm)
    assert n >= 20 and len(lo_all) == len(ref_l)
    assert dl < 1e-8 and dm < 1e-8
    assert lams_equal(eng.pw_get(), lam)

    # pinn_pw_disable: the plain kernel's bits
    plain = make(c, co, weighted=False)
    eng.set_weights(c["w0"])
    eng.pw_disable()
    a, b = plain.loss_grad(), eng.loss_grad()
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    plain.adam_init(1e-3)
    assert np.array_equal(plain.adam_run(5), eng.adam_run(5)) and np.array_equal(plain.get_weights(), eng.get_weights())
    plain.close()
    eng.close()

    # the adaptive draw on another context: the density is that of the unweighted residual, the draw resets the collocation
    # class (a set replacement) and leaves the other two alone
    eng = make(c, co)
    eng.adam_init(1e-3)
    eng.pw_adam_init(0.05, 0.02, 0.01)
    n_pool, seed = 20000, 0x5EED0011
    P = rad_ref.pool_points(n_pool, seed, LB, UB, "f64")
    eng.rad_collocation(3000, seed, n_pool, k=1, c=1.0)
    want, idx = rad_ref.rad_draw(P, eng.residual_at(P), seed, 0, 3000, 1, 1.0)
    assert np.array_equal(eng.get_collocation(), want) and len(np.unique(idx)) > 1
    got = eng.pw_get()
    assert np.array_equal(got[0], lam[0]) and np.array_equal(got[2], lam[2]) and np.all(got[1] == 1.0) and got[1].shape == (3000,)
    eng.close()


def test_new_adam_constants_rewrite_the_header_and_keep_weights_and_moments():
    """Two contexts alike (4 x 20, 3 pairs, N_u = 5, N_f = 70: two 64-point tiles, the second ragged, one tile per workgroup),
    all three rates on.  After 3 steps both get pinn_adam_init with the constants they had; the second gets other (beta1, beta2,
    eps) first, reads its weights (which brings the array's header up to date) and then the old constants again, so its header
    is rewritten twice before the next step.  Network weights and all lambdas stay equal bit for bit after every step: lambda,
    m and v of every point and pair survived the rewrites.  One tile per workgroup only: nothing here forces another launch
    plan.  Last, one step with the second context under the other constants: its lambdas must then differ, so the header it
    wrote is the one the kernel reads."""
    k, consts = 3, (1e-3, 0.9, 0.999, 1e-7)
    c = case_of(4, 70, 3, 5)
    a, b = make(c, adr_ref.ALLEN_CAHN), make(c, adr_ref.ALLEN_CAHN)
    for e in (a, b):
        e.adam_init(*consts)
        e.pw_adam_init(0.05, 0.02, 0.01)

    def step_and_compare():
        for _ in range(k):
            assert np.array_equal(a.adam_run(1), b.adam_run(1))
            assert np.array_equal(a.get_weights(), b.get_weights())
            assert lams_equal(a.pw_get(), b.pw_get())

    step_and_compare()
    assert not np.array_equal(a.pw_get()[1], c["lam_f"])            # the ascent is on
    a.adam_init(*consts)
    b.adam_init(1e-3, 0.8, 0.99, 1e-5)
    assert lams_equal(a.pw_get(), b.pw_get())
    b.adam_init(*consts)
    step_and_compare()
    a.adam_init(*consts)
    b.adam_init(1e-3, 0.8, 0.99, 1e-5)
    a.adam_run(1), b.adam_run(1)
    assert not any(np.array_equal(x, y) for x, y in zip(a.pw_get(), b.pw_get()))
    a.close(); b.close()


# ---- 5. set replacement resets exactly its class; refusals -----------------------------------------------------------------
def test_set_replacement_resets_exactly_its_class():
    c = case_of(8, 2048, 7, 37, seed=13)
    co = adr_ref.ALLEN_CAHN
    lam_u, lam_f, lam_b = c["lam_u"], c["lam_f"], c["lam_b"]
    eng = make(c, co)
    eng.loss_grad()

    def check_loss(X_f, X_u, u, X_lo, X_hi, lu, lf, lb_, n_f_total=None):
        lo = adr_pw_ref.loss_grad(eng.get_weights(), c["layers"], LB, UB, X_f, X_u, u, X_lo, X_hi, co, lu, lf, lb_)[0]
        assert abs(eng.loss_grad()[0] - lo) <= 1e-12 * lo

    # a data set of another size: data weights back to 1, the others kept (the collocation rows are re-placed behind it)
    X_u2, u2 = c["X_u"][:20], c["u"][:20]
    eng.set_data(X_u2, u2)
    got = eng.pw_get()
    assert np.all(got[0] == 1.0) and got[0].shape == (20,) and np.array_equal(got[1], lam_f) and np.array_equal(got[2], lam_b)
    check_loss(c["X_f"], X_u2, u2, c["X_lo"], c["X_hi"], np.ones(20), lam_f, lam_b)
    # other pairs (another count: every row behind them moves): the pairs' weights back to 1
    eng.pw_set(np.full(20, 2.0), lam_f, lam_b)
    X_lo2, X_hi2 = c["X_lo"][:4], c["X_hi"][:4]
    eng.set_boundary(X_lo2, X_hi2)
    got = eng.pw_get()
    assert np.all(got[0] == 2.0) and np.array_equal(got[1], lam_f) and np.all(got[2] == 1.0) and got[2].shape == (4,)
    check_loss(c["X_f"], X_u2, u2, X_lo2, X_hi2, np.full(20, 2.0), lam_f, np.ones(4))
    # a new collocation set from the host, by LHS (in place) and by RAD: collocation weights back to 1, the others kept
    lam_b2 = np.array([0.5, 1.5, 2.0, 0.75])
    eng.pw_set(np.full(20, 2.0), lam_f, lam_b2)
    eng.set_collocation(c["X_f"][:1000])
    got = eng.pw_get()
    assert np.all(got[0] == 2.0) and np.all(got[1] == 1.0) and got[1].shape == (1000,) and np.array_equal(got[2], lam_b2)
    check_loss(c["X_f"][:1000], X_u2, u2, X_lo2, X_hi2, np.full(20, 2.0), np.ones(1000), lam_b2)
    eng.pw_set(np.full(20, 2.0), np.full(1000, 3.0), lam_b2)
    eng.lhs_collocation(1000, 11)
    eng.loss_grad()
    eng.lhs_collocation(1000, 12)                   # same count: an in-place redraw
    got = eng.pw_get()
    assert np.all(got[0] == 2.0) and np.all(got[1] == 1.0) and np.array_equal(got[2], lam_b2)
    check_loss(eng.get_collocation(), X_u2, u2, X_lo2, X_hi2, np.full(20, 2.0), np.ones(1000), lam_b2)
    eng.pw_set(np.full(20, 2.0), np.full(1000, 3.0), lam_b2)
    eng.rad_collocation(1000, 12, 8000)
    got = eng.pw_get()
    assert np.all(got[0] == 2.0) and np.all(got[1] == 1.0) and np.array_equal(got[2], lam_b2)
    # pinn_pw_set zeroes the moments: after Adam steps, setting the same weights again restarts the ascent from rest
    eng.set_collocation(c["X_f"])
    eng.set_weights(c["w0"])
    eng.adam_init(1e-3)
    eng.pw_adam_init(0.05, 0.02, 0.01)
    eng.pw_set(np.full(20, 2.0), lam_f, lam_b2)
    eng.adam_run(1)
    first = eng.pw_get()
    eng.set_weights(c["w0"])
    eng.adam_init(1e-3)
    eng.pw_set(np.full(20, 2.0), lam_f, lam_b2)
    eng.adam_run(1)
    assert lams_equal(eng.pw_get(), first)
    eng.close()


def test_refusals_leave_the_context_unchanged():
    import pinn_native
    c = case_of(8, 2048, 7, 37, seed=13)
    co = adr_ref.ALLEN_CAHN
    lam = (c["lam_u"], c["lam_f"], c["lam_b"])
    eng = make(c, co)
    eng.pw_adam_init(0.05, 0.02, 0.01)
    before = eng.loss_grad()

    def same():
        after = eng.loss_grad()
        assert after[0] == before[0] and np.array_equal(after[1], before[1]) and np.array_equal(after[2], before[2])
        assert eng.kernel_path() == 7 and lams_equal(eng.pw_get(), lam)

    # counts that differ from the set sizes, non-finite weights, bad rates
    for bad in ((lam[0][:-1], lam[1], lam[2]), (lam[0], np.ones(len(lam[1]) + 1), lam[2]), (lam[0], lam[1], np.ones(14)),
                (lam[0], lam[1], np.ones(0))):
        with pytest.raises(pinn_native.PinnNativeError, match="weights for"):
            eng.pw_set(*bad)
        same()
    for k in range(3):
        for v in (np.nan, np.inf):
            bad = [x.copy() for x in lam]
            bad[k][-1] = v
            with pytest.raises(pinn_native.PinnNativeError, match="not finite"):
                eng.pw_set(*bad)
            same()
    for bad in ((-0.1, 0.0, 0.0), (0.0, np.nan, 0.0), (0.0, 0.0, np.inf)):
        with pytest.raises(pinn_native.PinnNativeError, match="rate"):
            eng.pw_adam_init(*bad)
        same()
    # while the weights are on: other kernel paths and communicators
    with pytest.raises(pinn_native.PinnNativeError, match="point weights run on kernel path 7 only"):
        eng.set_kernel_path(0)
    same()
    with pytest.raises(pinn_native.PinnNativeError, match="point weights are single-device"):
        eng.comm_init(b"\0" * 128, 1, 0)
    same()
    with pytest.raises(pinn_native.PinnNativeError, match="point weights are single-device"):
        eng.comm_xgmi_export(1, 0)
    same()
    # the Burgers form stays refused for this kind
    with pytest.raises(pinn_native.PinnNativeError, match="self-adaptive weights are for Burgers"):
        eng.sa_set_weights(lam[0], lam[1])
    same()
    # on path 0 the weights are refused; back on path 7 they are accepted
    eng.pw_disable()
    eng.set_kernel_path(0)
    with pytest.raises(pinn_native.PinnNativeError, match="point weights need kernel path 7"):
        eng.pw_set(*lam)
    with pytest.raises(pinn_native.PinnNativeError, match="point weights need kernel path 7"):
        eng.pw_adam_init(0.0, 0.01, 0.0)
    with pytest.raises(pinn_native.PinnNativeError, match="point weights are off"):
        eng.pw_get()
    assert eng.kernel_path() == 0
    eng.set_kernel_path(7)
    eng.pw_set(*lam)
    same()
    eng.close()
    # other kinds, float32: refused on a context with its sets and weights in place, which evaluates as before
    ide_tail = np.array(co, dtype=np.float64)
    ide_tail[2] = np.log(ide_tail[2])                       # the adr_ide kind carries log nu
    for kw, match in (({"pde": "burgers", "dtype": "f64"}, "adr kind"), ({"pde": "adr_ide", "dtype": "f64"}, "adr kind"),
                      ({"pde": "adr", "dtype": "f32"}, "float64")):
        e = pinn_native.Engine(c["layers"], LB, UB, **kw)
        if kw["pde"] == "burgers":
            e.set_pde_params(0.01 / np.pi)
        elif kw["pde"] == "adr":
            e.set_pde_params(*co)
        e.set_collocation(c["X_f"])
        e.set_data(c["X_u"], c["u"])
        if kw["pde"] != "burgers":
            e.set_boundary(c["X_lo"], c["X_hi"])
        e.set_weights(np.concatenate([c["w0"], ide_tail]) if kw["pde"] == "adr_ide" else c["w0"])
        path, was = e.kernel_path(), e.loss_grad()
        assert np.isfinite(was[0]) and was[0] > 0
        for call in (lambda: e.pw_set(), lambda: e.pw_set(*lam), lambda: e.pw_adam_init(0.0, 0.0, 0.0),
                     lambda: e.pw_adam_init(0.05, 0.02, 0.01)):
            with pytest.raises(pinn_native.PinnNativeError, match=match):
                call()
            now = e.loss_grad()
            assert now[0] == was[0] and np.array_equal(now[1], was[1]) and np.array_equal(now[2], was[2])
            assert e.kernel_path() == path
            with pytest.raises(pinn_native.PinnNativeError, match="point weights are off"):
                e.pw_get()
        e.close()


@pytest.mark.parametrize("how", ["comm_init", "comm_xgmi_export"])
def test_a_context_with_a_communicator_refuses_the_weights(how):
    """PINN_EUNSUPPORTED for an attached communicator: one rank (the only size one device allows), by RCCL or with the
    exported mailbox; pinn_pw_set and pinn_pw_adam_init are refused, and loss, gradient, terms and path stay what they were"""
    import pinn_native
    c = case_of(8, 2048, 7, 37, seed=13)
    co = adr_ref.ALLEN_CAHN
    lam = (c["lam_u"], c["lam_f"], c["lam_b"])
    eng = make(c, co, weighted=False)
    if how == "comm_init":
        eng.comm_init(pinn_native.Engine.comm_unique_id(), 1, 0)
    else:
        eng.comm_xgmi_export(1, 0)
    before = eng.loss_grad()
    assert np.isfinite(before[0]) and before[0] > 0
    for call in (lambda: eng.pw_set(), lambda: eng.pw_set(*lam), lambda: eng.pw_adam_init(0.0, 0.0, 0.0),
                 lambda: eng.pw_adam_init(0.05, 0.02, 0.01)):
        with pytest.raises(pinn_native.PinnNativeError, match="single-device; this context has a communicator"):
            call()
        after = eng.loss_grad()
        assert after[0] == before[0] and np.array_equal(after[1], before[1]) and np.array_equal(after[2], before[2])
        assert eng.kernel_path() == 7
        with pytest.raises(pinn_native.PinnNativeError, match="point weights are off"):
            eng.pw_get()
    eng.close()


# ---- 6. the script ---------------------------------------------------------------------------------------------------------
_SCRIPT = r"""
import json, os, sys
import numpy as np
sys.argv = [sys.argv[0], sys.argv[1]]
out = sys.argv[1] + ".npz"
sys.path.insert(0, os.path.join(%(pkg)r, "1d-allen-cahn"))
import runpy
g = runpy.run_path(os.path.join(%(pkg)r, "1d-allen-cahn", "inf_cont_allen_cahn.py"), run_name="pw_test")
hp = json.load(open(sys.argv[1]))
pinn = g["run"](hp)
lu, lf, lb = pinn.get_point_weights()
np.savez(out, w=pinn.get_weights(), lu=lu, lf=lf, lb=lb)
"""


def test_allen_cahn_script_with_point_weights_is_reproducible(tmp_path):
    hp = {"N_0": 64, "N_b": 8, "N_f": 2000, "layers": [2, 20, 20, 20, 20, 20, 20, 20, 20, 1],
          "tf_epochs": 40, "tf_lr": 0.001, "tf_b1": 0.9, "tf_eps": None,
          "nt_epochs": 20, "nt_lr": 0.8, "nt_ncorr": 50, "log_frequency": 10,
          "point_weights": True, "pw_init": [10, 1, 1], "pw_lr": [0, 0.01, 0]}
    runs = []
    for k in range(2):
        p = tmp_path / ("hp%d.json" % k)
        p.write_text(json.dumps(hp))
        env = dict(os.environ, PINN_NO_PLOT="1")
        r = subprocess.run([sys.executable, "-c", _SCRIPT % {"pkg": PKG}, str(p)], cwd=PKG, env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        runs.append((r.stdout, np.load(str(p) + ".npz")))
    (o0, a), (o1, b) = runs
    assert all(np.array_equal(a[k], b[k]) for k in ("w", "lu", "lf", "lb"))
    assert o0.count("Point weights:") == 1 and o1.count("Point weights:") == 1
    assert a["lu"].shape == (64,) and np.all(a["lu"] == 10.0)
    assert a["lb"].shape == (8,) and np.all(a["lb"] == 1.0)
    assert a["lf"].shape == (2000,) and np.all(np.isfinite(a["lf"])) and not np.all(a["lf"] == 1.0)
    end = [t for t in o0.splitlines() if t.startswith("Training finished")]
    assert end and np.isfinite(float(end[-1].split("error = ")[1].split()[0]))
