"""GPU: the discrete-time adr kind with trainable coefficients (pde "adr_disc_ide": the DISC_ADR_IDE instantiations of
csrc/kernels_disc.h) against tests/helpers/adr_disc_ide_oracle.py, itself pinned by tests/test_adr_disc_ide_host.py.

Tolerances are those tests/test_gpu_disc.py and tests/test_gpu_adr_disc.py hold the family to: loss and terms f64 1e-12 / f32
2e-5 of the total loss, gradient f64 1e-11 / f32 2e-4 of its largest entry, stage predictions f64 1e-10 / f32 1e-3.  Each of
the six tail entries is also judged on its own scale A_k = sum |dN dN/dp_k| with the yardstick of
tests/helpers/grad_entries.py, as tests/test_gpu_adr_ide.py does: |entry - wider-type entry| / A_k < K * max(plain error of
the compute type, 32 u), K that of the "w20" family (8 in float64, 9 in float32: the tightest the suite has).  Every loss_grad
is taken twice and must return the same bits."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG, golden

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import adr_disc_oracle as ado  # noqa: E402
import adr_disc_ide_oracle as adi  # noqa: E402
import grad_entries as ge  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = {"f64": (1e-12, 1e-11), "f32": (2e-5, 2e-4)}
TOL_VALUE = {"f64": 1e-12, "f32": 5e-6}
TOL_STAGE = {"f64": 1e-10, "f32": 1e-3}
TOL_ADAM = {"f64": 1e-10, "f32": 1e-4}
LB, UB = [-1.0], [1.0]
LAYERS, Q = [1, 23, 23, 7], 5
PDE = "adr_disc_ide"
_COEFS = ado.coefficient_vectors()


def rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300)


def make_engine(layers, dtype, sets=(None, None), theta=None, mask=None, pairs=None, order=1, pde=PDE):
    import pinn_native
    eng = pinn_native.Engine(layers, LB, UB, pde=pde, dtype=dtype)
    for s, st in enumerate(sets):
        if st is not None:
            eng.disc_set_stage(s, *st)
    if pairs is not None:
        eng.disc_set_periodic(pairs[0], pairs[1], order)
    if theta is not None:
        assert eng.n_params == theta.size
        eng.set_weights(theta)
    if mask is not None:
        eng.set_pde_trainable(mask)
    return eng


def tail_ratio(grad, theta, layers, sets, dtype, mask=63):
    """the six tail entries against the wider type on their own scales -> worst |dev| / A_k over max(plain, 32 u); a masked
    entry, and one without any term (A_k = 0), must be exactly 0.0"""
    dt = ge.DTYPES[dtype]
    u = ge.unit_roundoff(dt)
    g, A = adi.tail(theta, layers, LB, UB, sets, dtype=dt)
    if dtype == "f64" and not ge.longdouble_is_wider():
        gw, plain = g.astype(np.longdouble), ge.ASSUMED_F64_ULPS * u
    else:
        gw, _ = adi.tail(theta, layers, LB, UB, sets, dtype=ge.wider(dt))
        gw = gw.astype(np.longdouble)
        on = A > 0
        plain = float(np.max(np.abs(g.astype(np.longdouble) - gw)[on] / A[on])) if np.any(on) else 0.0
    yard = max(plain, ge.FLOOR_ULPS * u)
    worst = 0.0
    for k in range(6):
        if not (mask >> k) & 1 or A[k] == 0.0:
            assert grad[-6 + k] == 0.0, (k, grad[-6 + k])
        else:
            worst = max(worst, float(abs(np.longdouble(grad[-6 + k]) - gw[k]) / A[k]) / yard)
    return worst


def check(eng, dtype, theta, layers, sets, per, mask=63, tag=""):
    """loss, terms, gradient and tail against the oracle; a second evaluation returns the same bits -> (loss, grad, terms)"""
    loss, grad, terms = eng.loss_grad()
    lo, go, ex = adi.loss_grad(theta, layers, LB, UB, sets, per, mask)
    tl, tg = TOL[dtype]
    d_loss, d_grad = abs(loss - lo) / abs(lo), rel(grad, go)
    d_terms = max(abs(terms[k] - ex["terms"][k]) for k in range(3)) / abs(lo)
    ratio = tail_ratio(grad, theta, layers, sets, dtype, mask)
    print("MEASURED %s %s: loss %.3e terms %.3e grad %.3e tail ratio %.3f of %d" % (tag, dtype, d_loss, d_terms, d_grad, ratio,
                                                                               ge.K[("w20", dtype)]))
    assert d_loss <= tl and d_terms <= tl and d_grad <= tg, (tag, d_loss, d_terms, d_grad)
    assert ratio < ge.K[("w20", dtype)], (tag, ratio)
    loss2, grad2, terms2 = eng.loss_grad()
    assert loss2 == loss and np.array_equal(grad2, grad) and np.array_equal(terms2, terms), tag
    return loss, grad, terms


# ---- one coefficient at a time ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("k", range(7))
def test_operator_one_coefficient_at_a_time(k, dtype):
    sets, pairs, theta = adi.case(LAYERS, Q, 17, 3, 3, seed=10 + k, coef=_COEFS[k])
    eng = make_engine(LAYERS, dtype, sets, theta, 63, pairs, 1)
    try:
        _, grad, _ = check(eng, dtype, theta, LAYERS, sets, pairs + (1,), 63, "coef%d" % k)
        assert np.all(grad[-6:] != 0.0)
    finally:
        eng.close()


# ---- group edges -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("n_pairs", [1, 8, 9])
def test_group_edges(n_pairs, order, dtype):
    """1, 17 and 33 points in set 0 (a ragged last group, padded rows) beside 1 pair, one full group of 8 and a second group
    holding one; both sets with tables.  Padded rows and the pairs add nothing to the tail: it is the oracle's"""
    for n0 in (1, 17, 33):
        sets, pairs, theta = adi.case(LAYERS, Q, n0, 3, n_pairs, seed=40 + n0 + n_pairs, coef=_COEFS[6])
        eng = make_engine(LAYERS, dtype, sets, theta, 63, pairs, order)
        try:
            _, _, terms = check(eng, dtype, theta, LAYERS, sets, pairs + (order,), 63, "pairs%d-o%d-n%d" % (n_pairs, order, n0))
            assert terms[2] > 0.0
        finally:
            eng.close()


# ---- column edges -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("layers,q", [([1, 50, 50, 101], 100), ([1, 50, 50, 71], 70), ([1, 30, 8], 5), ([1, 50, 50, 130], 130)],
                         ids=["two-chunks", "table-ends-inside-a-chunk", "n_out-beyond-q+1-H1", "three-chunks-n_out-is-q"])
def test_column_edges(layers, q, dtype):
    """the tail sums cross chunks"""
    sets, pairs, theta = adi.case(layers, q, 37, 20, 3, seed=60 + q, coef=_COEFS[6], wscale=0.9 / np.sqrt(layers[1]))
    eng = make_engine(layers, dtype, sets, theta, 63, pairs, 1)
    try:
        check(eng, dtype, theta, layers, sets, pairs + (1,), 63, "cols%d" % layers[-1])
    finally:
        eng.close()


def test_wide_hidden_layers_f32():
    """hidden width 100: the NT = 8 instantiations, float32 only"""
    layers, q = [1, 100, 100, 13], 12
    sets, pairs, theta = adi.case(layers, q, 40, 2, 1, seed=70, coef=_COEFS[6], wscale=0.3)
    eng = make_engine(layers, "f32", sets, theta, 63, pairs, 1)
    try:
        check(eng, "f32", theta, layers, sets, pairs + (1,), 63, "wide")
    finally:
        eng.close()


# ---- slot subsets ---------------------------------------------------------------------------------------------------------------
def test_slot_subsets_and_removal():
    sets, pairs, theta = adi.case(LAYERS, Q, 17, 3, 3, seed=5, coef=_COEFS[6])
    # the pairs alone (f64 only: a difference of two near-equal wall values has no relative bound in f32): no tail gradient
    eng = make_engine(LAYERS, "f64", (None, None), theta, 63, pairs, 1)
    try:
        _, grad, terms = check(eng, "f64", theta, LAYERS, [None, None], pairs + (1,), 63, "pairs-alone")
        assert terms[0] == 0.0 and terms[1] == 0.0 and terms[2] > 0.0
        assert np.all(grad[-6:] == 0.0) and np.any(grad[:-6] != 0.0)
    finally:
        eng.close()
    for dtype in ("f64", "f32"):
        for s in (0, 1):                      # one stage set alone
            only = [sets[0] if s == 0 else None, sets[1] if s == 1 else None]
            eng = make_engine(LAYERS, dtype, only, theta, 63, None, 1)
            try:
                _, grad, terms = check(eng, dtype, theta, LAYERS, only, None, 63, "set%d-alone" % s)
                assert terms[1 - s] == 0.0 and terms[2] == 0.0 and np.all(grad[-6:] != 0.0)
            finally:
                eng.close()
        # both stage sets, then all three slots, then the pairs removed again: the stage-only value bit for bit
        eng = make_engine(LAYERS, dtype, sets, theta, 63, None, 1)
        try:
            loss0, grad0, terms0 = check(eng, dtype, theta, LAYERS, sets, None, 63, "stages-alone")
            assert terms0[2] == 0.0
            eng.disc_set_periodic(pairs[0], pairs[1], 1)
            check(eng, dtype, theta, LAYERS, sets, pairs + (1,), 63, "all-three")
            eng.disc_set_periodic([], [], 1)
            loss1, grad1, terms1 = eng.loss_grad()
            assert loss1 == loss0 and np.array_equal(grad1, grad0) and np.array_equal(terms1, terms0)
            # a set without a table adds nothing to the tail: the tail is set 0's
            eng.disc_set_stage(1, sets[1][0], sets[1][1], None)
            bare = [sets[0], (sets[1][0], sets[1][1], None)]
            check(eng, dtype, theta, LAYERS, bare, None, 63, "set1-without-table")
        finally:
            eng.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_mask_zeroes_exactly_the_unset_entries(dtype):
    sets, pairs, theta = adi.case(LAYERS, Q, 17, 3, 3, seed=6, coef=_COEFS[6])
    eng = make_engine(LAYERS, dtype, sets, theta, 63, pairs, 1)
    try:
        _, g_all, _ = eng.loss_grad()
        assert np.all(g_all[-6:] != 0.0)
        for mask in [0, 13] + [1 << k for k in range(6)] + [adi.mask_of(["nu", "r1", "r3"])]:
            eng.set_pde_trainable(mask)
            _, g, _ = eng.loss_grad()
            for k in range(6):
                assert g[-6 + k] == (g_all[-6 + k] if (mask >> k) & 1 else 0.0) and not (g[-6 + k] == 0.0 and np.signbit(g[-6 + k]))
            assert np.array_equal(g[:-6], g_all[:-6])
        eng.set_pde_trainable(["nu", "r1", "r3"])
        assert np.array_equal(eng.loss_grad()[1], g)
    finally:
        eng.close()


# ---- kind 4 embedded -----------------------------------------------------------------------------------------------------------
def _embed(w_ide):
    return np.concatenate([w_ide[:-2], [0.0, w_ide[-2], w_ide[-1], 0.0, 0.0, 0.0]])


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("tag", ["_small", ""])
def test_burgers_identification_embedded(tag, dtype):
    """tail [0, lambda_1, lambda_2, 0, 0, 0] with mask {a1, nu} is the reference's model: the reference-made fixture's loss
    and gradient, and a burgers_disc_ide engine on the same sets (no bit equality: the operator is evaluated in another
    order)"""
    from oracle import disc
    g = np.load(golden("burgers_disc_ide_eval%s.npz" % tag))
    q, layers = int(g["q"]), [int(v) for v in g["layers"]]
    W, _ = disc.irk_tables_like_reference(q)
    sets = disc.identification_sets(g["x_0"], g["u_0"], g["x_1"], g["u_1"], g["dt"], W[:-1], W[-1:])
    sets = [tuple(s) for s in sets]
    theta, mask = _embed(g["w0"]), adi.mask_of(["a1", "nu"])
    tl, tg = TOL[dtype]
    eng = make_engine(layers, dtype, sets, theta, mask, None, 1)
    ref = make_engine(layers, dtype, sets, g["w0"], None, None, 1, pde="burgers_disc_ide")
    try:
        loss, grad, terms = check(eng, dtype, theta, layers, sets, None, mask, "kind4%s" % tag)
        gf = g["grad"]
        d_loss, d_net = abs(loss - float(g["loss"])) / abs(float(g["loss"])), rel(grad[:-6], gf[:-2])
        d_lam = np.max(np.abs(grad[[-5, -4]] - gf[-2:])) / np.max(np.abs(gf))
        lr, gr, tr = ref.loss_grad()
        e_loss, e_net = abs(loss - lr) / abs(lr), rel(grad[:-6], gr[:-2])
        e_lam = np.max(np.abs(grad[[-5, -4]] - gr[-2:])) / np.max(np.abs(gr))
        print("MEASURED kind4%s %s: fixture loss %.3e net %.3e lambdas %.3e | engine loss %.3e net %.3e lambdas %.3e" % (
            tag, dtype, d_loss, d_net, d_lam, e_loss, e_net, e_lam))
        assert d_loss <= tl and d_net <= tg and d_lam <= tg
        assert e_loss <= tl and e_net <= tg and e_lam <= tg
        assert max(abs(terms[k] - tr[k]) for k in range(3)) <= tl * abs(lr)
        assert grad[-6] == 0.0 and np.all(grad[-3:] == 0.0)
    finally:
        eng.close()
        ref.close()


# ---- kind 7 embedded -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_mask_0_agrees_with_adr_disc(dtype):
    sets, pairs, theta = adi.case(LAYERS, Q, 33, 16, 3, seed=80, coef=ado.REACTION_HEAVY)
    a = make_engine(LAYERS, dtype, sets, theta, 0, pairs, 1)
    b = make_engine(LAYERS, dtype, sets, theta[:-6], None, pairs, 1, pde="adr_disc")
    try:
        b.set_pde_params(*a.get_pde_params())
        la, ga, ta = a.loss_grad()
        lb_, gb, tb = b.loss_grad()
        tl, tg = TOL[dtype]
        print("MEASURED kind7 %s: loss %.3e grad %.3e" % (dtype, abs(la - lb_) / abs(lb_), rel(ga[:-6], gb)))
        assert abs(la - lb_) <= tl * abs(lb_) and rel(ga[:-6], gb) <= tg
        assert max(abs(ta[k] - tb[k]) for k in range(3)) <= tl * abs(lb_)
        assert np.all(ga[-6:] == 0.0)
        assert a.loss_grad()[0] == la and np.array_equal(a.loss_grad()[1], ga)
    finally:
        a.close()
        b.close()


# ---- trajectories -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frozen", ["zero", "nonzero"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_adam_and_lbfgs_against_the_numpy_optimisers(dtype, frozen):
    """ten Adam steps at tests/test_gpu_adr_disc.py's trajectory tolerance (1e-10 / 1e-4, the golden run's hp), then five
    L-BFGS iterations: finite and non-increasing in both types as that file asks, and in float64 the logged losses and the
    last evaluated weights against oracle.optim.lbfgs at the 1e-8 every L-BFGS trajectory of the suite is held to
    (tests/test_gpu_adr.py).  Mask {nu, r1, r3}: the frozen a0, a1, r2 come back bit-identical from both optimisers"""
    from oracle import optim
    hp = json.loads(str(np.load(golden("burgers_disc_eval_small.npz"))["hp"]))
    coef = (0.0, 0.0, 0.05, -5.0, 0.0, 5.0) if frozen == "zero" else ado.REACTION_HEAVY
    mask = adi.mask_of(["nu", "r1", "r3"])
    sets, pairs, theta = adi.case(LAYERS, Q, 17, 3, 3, seed=95, coef=coef)
    per = pairs + (1,)
    ref, th_ref = adi.adam_losses(theta, LAYERS, LB, UB, sets, per, mask, 10, hp["tf_lr"], hp["tf_b1"], 0.999, hp["tf_eps"])
    eng = make_engine(LAYERS, dtype, sets, theta, mask, pairs, 1)
    try:
        eng.adam_init(hp["tf_lr"], hp["tf_b1"], 0.999, hp["tf_eps"])
        losses = eng.adam_run(10)
        w = eng.get_weights()
        d, dw = np.max(np.abs(losses - ref) / ref), rel(w, th_ref)
        print("MEASURED adam %s frozen %s: loss %.3e weights %.3e" % (dtype, frozen, d, dw))
        assert d <= TOL_ADAM[dtype] and dw <= TOL_ADAM[dtype]
        for k in (0, 1, 4):
            assert w[-6 + k].tobytes() == theta[-6 + k].tobytes()
        for k in (2, 3, 5):
            assert w[-6 + k] != theta[-6 + k]
        eng.set_weights(theta)
        eng.lbfgs_begin(5, 0.8, 50, np.finfo(float).eps)
        it, ll, done = eng.lbfgs_run(5)
        wm = eng.get_weights()
        assert len(ll) >= 2 and np.all(np.isfinite(ll)) and np.all(np.diff(ll) <= 0.0) and eng.status()[1] == 0
        for k in (0, 1, 4):
            assert wm[-6 + k].tobytes() == theta[-6 + k].tobytes()
        assert any(wm[-6 + k] != theta[-6 + k] for k in (2, 3, 5))
        if dtype == "f64":
            res = optim.lbfgs(lambda x: adi.loss_grad(x, LAYERS, LB, UB, sets, per, mask)[:2], theta, 5, 0.8, 50)
            ref_l = np.array([l for _, l in res["logs"]])
            dl, dm = float(np.max(np.abs(ll - ref_l) / ref_l)) if len(ll) == len(ref_l) else np.inf, rel(wm, res["x_model"])
            print("MEASURED lbfgs f64 frozen %s: loss %.3e w_model %.3e (%d logged)" % (frozen, dl, dm, len(ll)))
            assert len(ll) == len(ref_l) and dl < 1e-8 and dm < 1e-8
    finally:
        eng.close()


def test_heat_mode_nu_ends_nearer_the_truth_than_it_began():
    """u = exp(-nu pi^2 t) sin(pi x), nu = 0.1, snapshots at t = 0.1 and 0.9 through dt A and -dt (b - A), n_out = q = 16, nu
    alone trained from 2 x the truth: after 1000 Adam steps it is nearer (no accuracy is asked: DESIGN.md 4.16 records what a
    full schedule recovers), and the five frozen coefficients are the zeros they were"""
    from oracle import disc, init
    nu, t_0, t_1, q, layers = 0.1, 0.1, 0.9, 16, [1, 32, 32, 16]
    rs = np.random.RandomState(4321)
    u = lambda x, t: np.exp(-nu * np.pi ** 2 * t) * np.sin(np.pi * x)
    x_0, x_1 = rs.uniform(-1, 1, 100), rs.uniform(-1, 1, 100)
    A, b, _ = disc.gauss_legendre_butcher(q)
    dt = t_1 - t_0
    sets = [(x_0, u(x_0, t_0), dt * A), (x_1, u(x_1, t_1), -dt * (b[None, :] - A))]
    theta = adi.pack(init.glorot_flat(layers), (0.0, 0.0, 2.0 * nu, 0.0, 0.0, 0.0))
    eng = make_engine(layers, "f64", sets, theta, adi.mask_of(["nu"]), ([-1.0], [1.0]), 1)
    try:
        eng.adam_init(1e-3, 0.9, 0.999, 1e-8)
        losses = eng.adam_run(1000)
        found = eng.get_pde_params()
        print("MEASURED heat: nu %.5f after 1000 Adam steps (from %.2f, truth %.2f), loss %.3e -> %.3e" % (
            found[2], 2.0 * nu, nu, losses[0], losses[-1]))
        assert abs(found[2] - nu) < abs(2.0 * nu - nu)
        assert np.array_equal(eng.get_weights()[-6:][[0, 1, 3, 4, 5]], np.zeros(5))
    finally:
        eng.close()


# ---- set_pde_params / get_pde_params -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_params_round_trip_and_predictions_follow_the_tail(dtype):
    from oracle import mlp
    sets, pairs, theta = adi.case(LAYERS, Q, 17, 3, 3, seed=90, coef=_COEFS[6])
    eng = make_engine(LAYERS, dtype, sets, None, None, pairs, 1)
    try:
        assert np.array_equal(eng.get_pde_params()[[0, 1, 3, 4, 5]], np.array(ado.BURGERS)[[0, 1, 3, 4, 5]])
        assert abs(eng.get_pde_params()[2] - ado.BURGERS[2]) <= 1e-15 * ado.BURGERS[2]
        eng.set_weights(theta)
        params = mlp.unpack(theta[:-6], LAYERS)
        xs = np.sort(np.random.RandomState(91).uniform(-1, 1, 37))
        ref_U = mlp.forward_value(params, xs[:, None], np.array(LB), np.array(UB))

        def follows(coef, tag):
            got = eng.get_pde_params()
            assert np.array_equal(got[[0, 1, 3, 4, 5]], np.array(coef)[[0, 1, 3, 4, 5]]) and abs(got[2] - coef[2]) <= 1e-15 * coef[2]
            U = eng.predict(xs[:, None])
            assert np.max(np.abs(U - ref_U)) / max(1.0, np.max(np.abs(ref_U))) <= TOL_VALUE[dtype]
            worst = 0.0
            for s in (0, 1):
                P = eng.disc_predict(s, xs)
                pred = ado.stage_prediction(params, xs, LB, UB, sets[s][2], coef)
                worst = max(worst, np.max(np.abs(P - pred)) / max(1.0, np.max(np.abs(pred))))
            print("MEASURED stage %s %s: %.3e" % (tag, dtype, worst))
            assert worst <= TOL_STAGE[dtype]
            return eng.disc_predict(0, xs)

        P0 = follows(_COEFS[6], "set_weights")
        eng.set_pde_params(*ado.REACTION_HEAVY)
        P1 = follows(ado.REACTION_HEAVY, "set_pde_params")
        assert np.max(np.abs(P1 - P0)) > 1e-2
        assert np.array_equal(eng.get_weights()[:-6], theta[:-6])
        eng.set_weights(adi.pack(theta[:-6], _COEFS[3]))
        follows(_COEFS[3], "set_weights-again")
    finally:
        eng.close()


# ---- errors ---------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_evaluation_unchanged():
    import pinn_native
    sets, pairs, theta = adi.case(LAYERS, Q, 17, 3, 3, seed=97, coef=_COEFS[6])
    eng = make_engine(LAYERS, "f64", sets, theta, 13, pairs, 1)
    try:
        before = eng.loss_grad()

        def unchanged():
            after = eng.loss_grad()
            assert after[0] == before[0] and np.array_equal(after[1], before[1]) and np.array_equal(after[2], before[2])

        for bad in (64, -1):
            with pytest.raises(pinn_native.PinnNativeError, match="outside 0..63"):
                eng._check(eng._lib.pinn_set_pde_trainable(eng._h, bad))
            unchanged()
        for bad_nu in (0.0, -1e-3):
            with pytest.raises(pinn_native.PinnNativeError, match="nu must be positive"):
                eng.set_pde_params(0.0, 1.0, bad_nu, 0.0, 0.0, 0.0)
            unchanged()
        with pytest.raises(pinn_native.PinnNativeError, match="not finite"):
            eng.set_pde_params(0.0, np.inf, 0.1, 0.0, 0.0, 0.0)
        unchanged()
        with pytest.raises(pinn_native.PinnNativeError, match="6 coefficients"):
            eng.set_pde_params(0.0, 1.0, 0.1, 0.0, 0.0)
        unchanged()
        # what refuses the discrete-time kinds 3, 4 and 7 refuses this one
        for call in (lambda: eng.set_collocation(np.zeros((4, 2))), lambda: eng.set_data(np.zeros((4, 2)), np.zeros((4, LAYERS[-1]))),
                     lambda: eng.residual()):
            with pytest.raises(pinn_native.PinnNativeError, match="discrete-time"):
                call()
        unchanged()
    finally:
        eng.close()
    # set_pde_trainable on an adr_disc context
    b = make_engine(LAYERS, "f64", [sets[0], None], theta[:-6], None, pairs, 1, pde="adr_disc")
    try:
        before = b.loss_grad()
        with pytest.raises(pinn_native.PinnNativeError, match="only the adr_ide kind"):
            b.set_pde_trainable(["nu"])
        after = b.loss_grad()
        assert after[0] == before[0] and np.array_equal(after[1], before[1])
    finally:
        b.close()
    # periodic pairs on a Burgers kind still name adr_disc
    c = make_engine(LAYERS, "f64", [(sets[0][0], sets[0][1], sets[0][2]), None], None, None, None, 1, pde="burgers_disc")
    try:
        with pytest.raises(pinn_native.PinnNativeError, match="adr_disc"):
            c.disc_set_periodic(pairs[0], pairs[1], 1)
    finally:
        c.close()


# ---- the script -------------------------------------------------------------------------------------------------------------------
LINE = re.compile(r"^(tf_epoch|nt_epoch) =\s+(\d+)\s+elapsed = \d\d:\d\d \(\+\d\d\.\d\)  loss = (\S+)  .*r1 = (\S+)  r3 = (\S+)")
END = re.compile(r"^Training finished \(epoch (\d+)\): duration = \d\d:\d\d  error = (\S+)  ")


def test_ide_disc_allen_cahn_script_runs(tmp_path):
    """1d-allen-cahn/ide_disc_allen_cahn.py as a child process with a small hp file: exits 0, both optimiser phases logged with
    the coefficient columns, and the last logged loss is below the first"""
    hp = {"N_0": 50, "N_1": 50, "q": 8, "layers": [1, 32, 32, 8], "tf_epochs": 20, "tf_lr": 0.001, "tf_b1": 0.9,
          "tf_eps": 1e-08, "nt_epochs": 20, "nt_lr": 0.8, "nt_ncorr": 50, "log_frequency": 10}
    hp_file = tmp_path / "hp.json"
    hp_file.write_text(json.dumps(hp))
    env = dict(os.environ, PINN_NO_PLOT="1", MPLBACKEND="Agg")
    res = subprocess.run([sys.executable, os.path.join(PKG, "1d-allen-cahn", "ide_disc_allen_cahn.py"), str(hp_file)],
                         cwd=PKG, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    out = res.stdout
    assert "Training started" in out and "-- Starting Adam optimization --" in out and "-- Starting LBFGS optimization --" in out
    rows = [(m.group(1), int(m.group(2)), float(m.group(3)), float(m.group(4)), float(m.group(5)))
            for m in map(LINE.match, out.splitlines()) if m]
    ends = [m for m in map(END.match, out.splitlines()) if m]
    assert any(r[0] == "tf_epoch" for r in rows) and any(r[0] == "nt_epoch" for r in rows), out[-2000:]
    # (the closing line counts the Adam epochs, as 1d-burgers/ide_disc_burgers.py's does)
    assert len(ends) == 1 and int(ends[0].group(1)) == 20 and np.isfinite(float(ends[0].group(2)))
    assert np.isfinite(rows[-1][2]) and rows[-1][2] < rows[0][2], (rows[0], rows[-1])
    assert all(np.isfinite(r[3]) and np.isfinite(r[4]) for r in rows) and rows[-1][3] != -2.0
    assert "identified coefficients" in out
