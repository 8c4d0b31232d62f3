"""GPU: the discrete-time adr family with a dispersion term (pde "adrd_disc": the DISC_ADRD instantiations of
csrc/kernels_disc.h, four Taylor channels) against tests/helpers/adrd_disc_oracle.py, itself pinned by
tests/test_adrd_disc_host.py.

float64 keeps the family's tolerances (tests/test_gpu_adr_disc_ide.py): loss and terms 1e-12 of the total loss, gradient
1e-11 of its largest entry, stage predictions 1e-10.  float32: a third derivative amplifies rounding by another factor of
the input scale, so each float32 bound comes from the helper's OWN float32-arithmetic error against its float64 result on the
very case, computed here on the CPU: the family's 2e-5 / 2e-4 / 1e-3 where that error is at most a quarter of it, 4 x that
error otherwise (f32_bound).  The kernel's output never enters a bound.  Each of the seven tail entries is also judged on its
own scale A_k = sum |dN dN/dp_k| with the yardstick of tests/helpers/grad_entries.py: |entry - wider-type entry| / A_k <
K * max(plain error of the compute type, 32 u), K that of the "w20" family.  Every loss_grad is taken twice and must return
the same bits."""
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
import adrd_disc_oracle as add  # noqa: E402
import grad_entries as ge  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = {"f64": (1e-12, 1e-11), "f32": (2e-5, 2e-4)}
TOL_VALUE = {"f64": 1e-12, "f32": 5e-6}
TOL_STAGE = {"f64": 1e-10, "f32": 1e-3}
TOL_ADAM = {"f64": 1e-10, "f32": 1e-4}
LB, UB = [-1.0], [1.0]
LAYERS, Q = [1, 23, 23, 7], 5
PDE = "adrd_disc"
ALL = 127
_COEFS = add.coefficient_vectors()


def rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300)


def f32_bound(family, helper_err):
    """the family's float32 tolerance where the helper's own float32 error is at most a quarter of it, 4 x that error else"""
    return family if helper_err <= 0.25 * family else 4.0 * helper_err


def make_engine(layers, dtype, sets=(None, None), theta=None, mask=None, pairs=None, order=1, pde=PDE, coef=None):
    """coef (seven raw values) goes in first, through set_pde_params: that is what raises or lowers the nu = 0 flag"""
    import pinn_native
    eng = pinn_native.Engine(layers, LB, UB, pde=pde, dtype=dtype)
    for s, st in enumerate(sets):
        if st is not None:
            eng.disc_set_stage(s, *st)
    if pairs is not None:
        eng.disc_set_periodic(pairs[0], pairs[1], order)
    if coef is not None:
        eng.set_pde_params(*coef)
    if theta is not None:
        assert eng.n_params == theta.size
        eng.set_weights(theta)
    if mask is not None:
        eng.set_pde_trainable(mask)
    return eng


def tail_ratio(grad, theta, layers, sets, dtype, mask=ALL, nu_on=True):
    """the seven tail entries against the wider type on their own scales -> worst |dev| / A_k over max(plain, 32 u); a masked
    entry, and one without any term (A_k = 0; the nu entry with nu = 0), must be exactly 0.0"""
    dt = ge.DTYPES[dtype]
    u = ge.unit_roundoff(dt)
    g, A = add.tail(theta, layers, LB, UB, sets, dtype=dt, nu_on=nu_on)
    if dtype == "f64" and not ge.longdouble_is_wider():
        gw, plain = g.astype(np.longdouble), ge.ASSUMED_F64_ULPS * u
    else:
        gw, _ = add.tail(theta, layers, LB, UB, sets, dtype=ge.wider(dt), nu_on=nu_on)
        gw = gw.astype(np.longdouble)
        on = A > 0
        plain = float(np.max(np.abs(g.astype(np.longdouble) - gw)[on] / A[on])) if np.any(on) else 0.0
    yard = max(plain, ge.FLOOR_ULPS * u)
    worst = 0.0
    for k in range(7):
        if not (mask >> k) & 1 or A[k] == 0.0:
            assert grad[-7 + k] == 0.0 and not np.signbit(grad[-7 + k]), (k, grad[-7 + k])
        else:
            worst = max(worst, float(abs(np.longdouble(grad[-7 + k]) - gw[k]) / A[k]) / yard)
    return worst


def bounds(dtype, theta, layers, sets, per, mask, nu_on, ref):
    """(loss and terms, gradient) tolerances for this case; float32: from the helper's float32 sweep against `ref`, its
    float64 one"""
    tl, tg = TOL[dtype]
    if dtype == "f64":
        return tl, tg, 0.0, 0.0
    lo, go, ex = ref
    l32, g32, e32 = add.loss_grad(theta, layers, LB, UB, sets, per, mask, nu_on, dtype=np.float32)
    h_loss = max(abs(l32 - lo), max(abs(e32["terms"][k] - ex["terms"][k]) for k in range(3))) / abs(lo)
    h_grad = rel(g32, go)
    return f32_bound(tl, h_loss), f32_bound(tg, h_grad), h_loss, h_grad


def check(eng, dtype, theta, layers, sets, per, mask=ALL, tag="", nu_on=True):
    """loss, terms, gradient and tail against the oracle; a second evaluation returns the same bits -> (loss, grad, terms)"""
    loss, grad, terms = eng.loss_grad()
    ref = add.loss_grad(theta, layers, LB, UB, sets, per, mask, nu_on)
    lo, go, ex = ref
    tl, tg, h_loss, h_grad = bounds(dtype, theta, layers, sets, per, mask, nu_on, ref)
    d_loss, d_grad = abs(loss - lo) / abs(lo), rel(grad, go)
    d_terms = max(abs(terms[k] - ex["terms"][k]) for k in range(3)) / abs(lo)
    ratio = tail_ratio(grad, theta, layers, sets, dtype, mask, nu_on)
    print("MEASURED %s %s: loss %.3e terms %.3e (bound %.3e, helper f32 %.3e) grad %.3e (bound %.3e, helper f32 %.3e) "
          "tail ratio %.3f of %d" % (tag, dtype, d_loss, d_terms, tl, h_loss, d_grad, tg, h_grad, ratio, ge.K[("w20", dtype)]))
    assert d_loss <= tl and d_terms <= tl and d_grad <= tg, (tag, d_loss, d_terms, d_grad, tl, tg)
    assert ratio < ge.K[("w20", dtype)], (tag, ratio)
    loss2, grad2, terms2 = eng.loss_grad()
    assert loss2 == loss and np.array_equal(grad2, grad) and np.array_equal(terms2, terms), tag
    return loss, grad, terms


# ---- one coefficient at a time ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("k", range(8))
def test_operator_one_coefficient_at_a_time(k, dtype):
    sets, pairs, theta = add.case(LAYERS, Q, 17, 3, 3, seed=10 + k, coef=_COEFS[k])
    eng = make_engine(LAYERS, dtype, sets, theta, ALL, pairs, 1)
    try:
        _, grad, _ = check(eng, dtype, theta, LAYERS, sets, pairs + (1,), ALL, "coef%d" % k)
        assert np.all(grad[-7:] != 0.0)
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
        sets, pairs, theta = add.case(LAYERS, Q, n0, 3, n_pairs, seed=40 + n0 + n_pairs, coef=_COEFS[7])
        eng = make_engine(LAYERS, dtype, sets, theta, ALL, pairs, order)
        try:
            _, _, terms = check(eng, dtype, theta, LAYERS, sets, pairs + (order,), ALL, "pairs%d-o%d-n%d" % (n_pairs, order, n0))
            assert terms[2] > 0.0
        finally:
            eng.close()


# ---- column edges -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("layers,q", [([1, 50, 50, 101], 100), ([1, 50, 50, 71], 70), ([1, 30, 8], 5), ([1, 50, 50, 130], 130)],
                         ids=["two-chunks", "table-ends-inside-a-chunk", "n_out-beyond-q+1-H1", "three-chunks-n_out-is-q"])
def test_column_edges(layers, q, dtype):
    """the seven tail sums, the seventh among them, cross chunks"""
    sets, pairs, theta = add.case(layers, q, 37, 20, 3, seed=60 + q, coef=_COEFS[7], wscale=0.9 / np.sqrt(layers[1]))
    eng = make_engine(layers, dtype, sets, theta, ALL, pairs, 1)
    try:
        check(eng, dtype, theta, layers, sets, pairs + (1,), ALL, "cols%d" % layers[-1])
    finally:
        eng.close()


# ---- width edges ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("layers,q", [([1, 64, 64, 9], 8), ([1, 3, 3, 4], 3), ([1, 17, 17, 17, 17, 17, 6], 5)],
                         ids=["full-tile-W-is-WP", "one-k-step", "five-hidden-layers"])
def test_width_edges(layers, q, dtype):
    """a full NT = 4 tile, a single k-step, and a net deep enough that the d4 term of the reverse sweep acts repeatedly"""
    sets, pairs, theta = add.case(layers, q, 37, 20, 3, seed=160 + layers[1], coef=_COEFS[7], wscale=0.9 / np.sqrt(max(layers[1], 2)))
    eng = make_engine(layers, dtype, sets, theta, ALL, pairs, 1)
    try:
        check(eng, dtype, theta, layers, sets, pairs + (1,), ALL, "width%d-H%d" % (layers[1], len(layers) - 2))
    finally:
        eng.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_width_65_is_refused_at_create(dtype):
    import pinn_native
    with pytest.raises(pinn_native.PinnNativeError, match=r"exceeds 64.*\(code -5\)"):
        pinn_native.Engine([1, 65, 65, 4], LB, UB, pde=PDE, dtype=dtype)
    pinn_native.Engine([1, 64, 64, 4], LB, UB, pde=PDE, dtype=dtype).close()


# ---- saturation --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_saturated_first_layer(dtype):
    """W0 and b0 times tests/helpers/grad_entries.py's GAIN0 (12): |a| > 0.999 on part of the first layer and below 1/2 on
    another part, so that d3t and d4 are taken on both sides of their sign changes (a^2 = 1/3 and 2/3) and in the tail of
    tanh; the same tolerances"""
    sets, pairs, theta = add.case(LAYERS, Q, 33, 16, 3, seed=300, coef=_COEFS[7], wscale=0.9 / np.sqrt(LAYERS[1]))
    W = LAYERS[1]
    theta[:2 * W] *= ge.GAIN0
    x = np.concatenate([sets[0][0], sets[1][0]]).reshape(-1, 1)
    a = np.abs(np.tanh(x * theta[:W][None, :] + theta[W:2 * W][None, :]))
    share = float(np.mean(a > 0.999))
    assert 0.05 < share < 0.95 and np.mean(a * a < 1 / 3) > 0.05 and np.mean((a * a > 1 / 3) & (a * a < 2 / 3)) > 0.02, share
    eng = make_engine(LAYERS, dtype, sets, theta, ALL, pairs, 1)
    try:
        check(eng, dtype, theta, LAYERS, sets, pairs + (1,), ALL, "saturated(%.2f)" % share)
    finally:
        eng.close()


# ---- slot subsets ---------------------------------------------------------------------------------------------------------------
def test_slot_subsets_and_removal():
    sets, pairs, theta = add.case(LAYERS, Q, 17, 3, 3, seed=5, coef=_COEFS[7])
    # the pairs alone (f64 only: a difference of two near-equal wall values has no relative bound in f32): no tail gradient
    eng = make_engine(LAYERS, "f64", (None, None), theta, ALL, pairs, 1)
    try:
        _, grad, terms = check(eng, "f64", theta, LAYERS, [None, None], pairs + (1,), ALL, "pairs-alone")
        assert terms[0] == 0.0 and terms[1] == 0.0 and terms[2] > 0.0
        assert np.all(grad[-7:] == 0.0) and np.any(grad[:-7] != 0.0)
    finally:
        eng.close()
    for dtype in ("f64", "f32"):
        for s in (0, 1):                      # one stage set alone
            only = [sets[0] if s == 0 else None, sets[1] if s == 1 else None]
            eng = make_engine(LAYERS, dtype, only, theta, ALL, None, 1)
            try:
                _, grad, terms = check(eng, dtype, theta, LAYERS, only, None, ALL, "set%d-alone" % s)
                assert terms[1 - s] == 0.0 and terms[2] == 0.0 and np.all(grad[-7:] != 0.0)
            finally:
                eng.close()
        # both stage sets, then all three slots, then the pairs removed again: the stage-only value bit for bit
        eng = make_engine(LAYERS, dtype, sets, theta, ALL, None, 1)
        try:
            loss0, grad0, terms0 = check(eng, dtype, theta, LAYERS, sets, None, ALL, "stages-alone")
            assert terms0[2] == 0.0
            eng.disc_set_periodic(pairs[0], pairs[1], 1)
            check(eng, dtype, theta, LAYERS, sets, pairs + (1,), ALL, "all-three")
            eng.disc_set_periodic([], [], 1)
            loss1, grad1, terms1 = eng.loss_grad()
            assert loss1 == loss0 and np.array_equal(grad1, grad0) and np.array_equal(terms1, terms0)
            eng.disc_set_periodic(pairs[0], pairs[1], 1)      # re-added, removed once more: the same bits again
            eng.loss_grad()
            eng.disc_set_periodic([], [], 1)
            loss2, grad2, _ = eng.loss_grad()
            assert loss2 == loss0 and np.array_equal(grad2, grad0)
            # a set without a table adds nothing to the tail: the tail is set 0's
            eng.disc_set_stage(1, sets[1][0], sets[1][1], None)
            bare = [sets[0], (sets[1][0], sets[1][1], None)]
            check(eng, dtype, theta, LAYERS, bare, None, ALL, "set1-without-table")
        finally:
            eng.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_mask_zeroes_exactly_the_unset_entries(dtype):
    sets, pairs, theta = add.case(LAYERS, Q, 17, 3, 3, seed=6, coef=_COEFS[7])
    eng = make_engine(LAYERS, dtype, sets, theta, ALL, pairs, 1)
    try:
        _, g_all, _ = eng.loss_grad()
        assert np.all(g_all[-7:] != 0.0)
        for mask in [0, 64 + 13] + [1 << k for k in range(7)] + [add.mask_of(["a1", "d3"])]:
            eng.set_pde_trainable(mask)
            _, g, _ = eng.loss_grad()
            for k in range(7):
                assert g[-7 + k] == (g_all[-7 + k] if (mask >> k) & 1 else 0.0) and not (g[-7 + k] == 0.0 and np.signbit(g[-7 + k]))
            assert np.array_equal(g[:-7], g_all[:-7])
        eng.set_pde_trainable(["a1", "d3"])
        assert np.array_equal(eng.loss_grad()[1], g)
    finally:
        eng.close()


# ---- the nu = 0 flag --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_nu_zero_is_a_flag(dtype):
    """nu = 0 gives the helper's nu_on=False values and a nu entry of exactly 0.0; 10 Adam steps and 5 L-BFGS iterations leave
    the nu slot untouched; nu raised to 0.1 and set back to 0 returns the first evaluation bit for bit"""
    coef = np.array(_COEFS[7])
    coef[2] = 0.0
    sets, pairs, theta = add.case(LAYERS, Q, 17, 3, 3, seed=7, coef=tuple(coef))
    n = add.n_net(LAYERS)
    assert theta[n + 2] == 0.0
    mask = ALL & ~4
    eng = make_engine(LAYERS, dtype, sets, theta, mask, pairs, 1, coef=coef)
    try:
        assert np.array_equal(eng.get_pde_params(), coef)
        loss, grad, terms = check(eng, dtype, theta, LAYERS, sets, pairs + (1,), mask, "nu-off", nu_on=False)
        assert grad[n + 2] == 0.0 and not np.signbit(grad[n + 2])
        eng.set_pde_params(*np.where(np.arange(7) == 2, 0.1, coef))
        assert eng.get_pde_params()[2] == pytest.approx(0.1, rel=1e-15)
        th_on = eng.get_weights()
        assert np.array_equal(th_on[:n], theta[:n]) and abs(th_on[n + 2] - np.log(0.1)) < 1e-15
        check(eng, dtype, th_on, LAYERS, sets, pairs + (1,), mask, "nu-on-again")
        assert eng.loss_grad()[0] != loss
        eng.set_pde_params(*coef)
        loss1, grad1, terms1 = eng.loss_grad()
        assert loss1 == loss and np.array_equal(grad1, grad) and np.array_equal(terms1, terms)
        assert np.array_equal(eng.get_weights(), theta)
        eng.adam_init(1e-3, 0.9, 0.999, 1e-8)
        eng.adam_run(10)
        w = eng.get_weights()
        assert w[n + 2].tobytes() == np.float64(0.0).tobytes() and w[n + 6] != theta[n + 6] and eng.get_pde_params()[2] == 0.0
        eng.set_weights(theta)
        eng.lbfgs_begin(5, 0.8, 50, np.finfo(float).eps)
        _, ll, _ = eng.lbfgs_run(5)
        w = eng.get_weights()
        assert len(ll) >= 2 and np.all(np.isfinite(ll)) and eng.status()[1] == 0
        assert w[n + 2].tobytes() == np.float64(0.0).tobytes() and w[n + 6] != theta[n + 6]
    finally:
        eng.close()


def test_errors_leave_the_evaluation_unchanged():
    import pinn_native
    coef = np.array(_COEFS[7])
    sets, pairs, theta = add.case(LAYERS, Q, 17, 3, 3, seed=97, coef=tuple(coef))
    eng = make_engine(LAYERS, "f64", sets, theta, 64 + 13, pairs, 1, coef=coef)      # the nu bit (4) is in 13
    try:
        before = eng.loss_grad()
        p_before = eng.get_pde_params()

        def unchanged():
            after = eng.loss_grad()
            assert after[0] == before[0] and np.array_equal(after[1], before[1]) and np.array_equal(after[2], before[2])
            assert np.array_equal(eng.get_pde_params(), p_before)

        for bad in (128, -1):
            with pytest.raises(pinn_native.PinnNativeError, match="outside 0..127"):
                eng._check(eng._lib.pinn_set_pde_trainable(eng._h, bad))
            unchanged()
        # nu = 0 while the nu bit is trainable
        with pytest.raises(pinn_native.PinnNativeError, match="nu must be positive to be trained"):
            eng.set_pde_params(*np.where(np.arange(7) == 2, 0.0, coef))
        unchanged()
        with pytest.raises(pinn_native.PinnNativeError, match="nu must be"):
            eng.set_pde_params(*np.where(np.arange(7) == 2, -1e-3, coef))
        unchanged()
        with pytest.raises(pinn_native.PinnNativeError, match="not finite"):
            eng.set_pde_params(*np.where(np.arange(7) == 6, np.inf, coef))
        unchanged()
        for n_bad in (6, 8):
            with pytest.raises(pinn_native.PinnNativeError, match="7 coefficients"):
                eng.set_pde_params(*([0.1] * n_bad))
            unchanged()
        # what refuses the discrete-time kinds refuses this one
        for call in (lambda: eng.set_collocation(np.zeros((4, 2))), lambda: eng.set_data(np.zeros((4, 2)), np.zeros((4, LAYERS[-1]))),
                     lambda: eng.residual()):
            with pytest.raises(pinn_native.PinnNativeError, match="discrete-time"):
                call()
        unchanged()
    finally:
        eng.close()
    # the other order: nu = 0 first, then the nu bit
    coef0 = np.where(np.arange(7) == 2, 0.0, coef)
    eng = make_engine(LAYERS, "f64", sets, add.pack(theta[:-7], coef0), 64 + 9, pairs, 1, coef=coef0)
    try:
        before = eng.loss_grad()
        for bad in (4, 64 + 13, ["nu"]):
            with pytest.raises(pinn_native.PinnNativeError, match="nu must be positive to be trained"):
                eng.set_pde_trainable(bad)
            after = eng.loss_grad()
            assert after[0] == before[0] and np.array_equal(after[1], before[1])
        assert before[1][-7 + 2] == 0.0 and before[1][-7 + 0] != 0.0 and before[1][-7 + 1] == 0.0
    finally:
        eng.close()


# ---- the siblings embedded ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_d3_zero_agrees_with_adr_disc_ide(dtype):
    """d3 = 0 with mask m against an adr_disc_ide engine on the same sets: loss, net entries and the six tail entries at the
    family tolerances (no bit equality: another instantiation)"""
    m = adi.mask_of(["a1", "nu", "r1", "r3"])
    sets, pairs, th6 = adi.case(LAYERS, Q, 33, 16, 3, seed=80, coef=ado.REACTION_HEAVY)
    th7 = np.concatenate([th6, [0.0]])
    a = make_engine(LAYERS, dtype, sets, th7, m, pairs, 1, coef=ado.REACTION_HEAVY + (0.0,))
    b = make_engine(LAYERS, dtype, sets, th6, m, pairs, 1, pde="adr_disc_ide")
    try:
        la, ga, ta = a.loss_grad()
        lb_, gb, tb = b.loss_grad()
        tl, tg = TOL[dtype]
        d_tail = np.max(np.abs(ga[-7:-1] - gb[-6:])) / np.max(np.abs(gb))
        print("MEASURED kind8 %s: loss %.3e net %.3e tail %.3e" % (dtype, abs(la - lb_) / abs(lb_), rel(ga[:-7], gb[:-6]), d_tail))
        assert abs(la - lb_) <= tl * abs(lb_) and rel(ga[:-7], gb[:-6]) <= tg and d_tail <= tg
        assert max(abs(ta[k] - tb[k]) for k in range(3)) <= tl * abs(lb_)
        for k in range(6):
            assert (ga[-7 + k] == 0.0) == (not (m >> k) & 1)
        assert ga[-1] == 0.0
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_mask_0_and_d3_zero_agrees_with_adr_disc(dtype):
    sets, pairs, th6 = adi.case(LAYERS, Q, 33, 16, 3, seed=80, coef=ado.REACTION_HEAVY)
    th7 = np.concatenate([th6, [0.0]])
    a = make_engine(LAYERS, dtype, sets, th7, 0, pairs, 1, coef=ado.REACTION_HEAVY + (0.0,))
    b = make_engine(LAYERS, dtype, sets, th6[:-6], None, pairs, 1, pde="adr_disc")
    try:
        b.set_pde_params(*a.get_pde_params()[:6])
        la, ga, ta = a.loss_grad()
        lb_, gb, tb = b.loss_grad()
        tl, tg = TOL[dtype]
        print("MEASURED kind7 %s: loss %.3e grad %.3e" % (dtype, abs(la - lb_) / abs(lb_), rel(ga[:-7], gb)))
        assert abs(la - lb_) <= tl * abs(lb_) and rel(ga[:-7], gb) <= tg
        assert max(abs(ta[k] - tb[k]) for k in range(3)) <= tl * abs(lb_)
        assert np.all(ga[-7:] == 0.0)
        assert a.loss_grad()[0] == la and np.array_equal(a.loss_grad()[1], ga)
    finally:
        a.close()
        b.close()


# ---- trajectories -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_adam_and_lbfgs_against_the_numpy_optimisers(dtype):
    """ten Adam steps at the family's trajectory tolerance (1e-10 / 1e-4, the golden run's hp), then five L-BFGS iterations:
    finite and non-increasing in both types, and in float64 the logged losses and the last evaluated weights against
    oracle.optim.lbfgs at 1e-8.  Mask {a1, d3}: the frozen entries come back bit-identical from both optimisers"""
    from oracle import optim
    hp = json.loads(str(np.load(golden("burgers_disc_eval_small.npz"))["hp"]))
    coef = ado.REACTION_HEAVY + (0.02,)
    mask = add.mask_of(["a1", "d3"])
    sets, pairs, theta = add.case(LAYERS, Q, 17, 3, 3, seed=95, coef=coef)
    per = pairs + (1,)
    ref, th_ref = add.adam_losses(theta, LAYERS, LB, UB, sets, per, mask, 10, hp["tf_lr"], hp["tf_b1"], 0.999, hp["tf_eps"])
    eng = make_engine(LAYERS, dtype, sets, theta, mask, pairs, 1, coef=coef)
    try:
        eng.adam_init(hp["tf_lr"], hp["tf_b1"], 0.999, hp["tf_eps"])
        losses = eng.adam_run(10)
        w = eng.get_weights()
        d, dw = np.max(np.abs(losses - ref) / ref), rel(w, th_ref)
        print("MEASURED adam %s: loss %.3e weights %.3e" % (dtype, d, dw))
        assert d <= TOL_ADAM[dtype] and dw <= TOL_ADAM[dtype]
        for k in (0, 2, 3, 4, 5):
            assert w[-7 + k].tobytes() == theta[-7 + k].tobytes()
        for k in (1, 6):
            assert w[-7 + k] != theta[-7 + k]
        eng.set_weights(theta)
        eng.lbfgs_begin(5, 0.8, 50, np.finfo(float).eps)
        it, ll, done = eng.lbfgs_run(5)
        wm = eng.get_weights()
        assert len(ll) >= 2 and np.all(np.isfinite(ll)) and np.all(np.diff(ll) <= 0.0) and eng.status()[1] == 0
        for k in (0, 2, 3, 4, 5):
            assert wm[-7 + k].tobytes() == theta[-7 + k].tobytes()
        assert any(wm[-7 + k] != theta[-7 + k] for k in (1, 6))
        if dtype == "f64":
            res = optim.lbfgs(lambda x: add.loss_grad(x, LAYERS, LB, UB, sets, per, mask)[:2], theta, 5, 0.8, 50)
            ref_l = np.array([l for _, l in res["logs"]])
            dl, dm = float(np.max(np.abs(ll - ref_l) / ref_l)) if len(ll) == len(ref_l) else np.inf, rel(wm, res["x_model"])
            print("MEASURED lbfgs f64: loss %.3e w_model %.3e (%d logged)" % (dl, dm, len(ll)))
            assert len(ll) == len(ref_l) and dl < 1e-8 and dm < 1e-8
    finally:
        eng.close()


def test_linear_dispersive_mode_d3_ends_nearer_the_truth_than_it_began():
    """u = sin(pi x + d3 pi^3 t) solves u_t + d3 u_xxx = 0: d3 = 0.02, snapshots at t = 0.1 and 0.9 through dt A and
    -dt (b - A), [1, 32, 32, 16], n_out = q = 16, 100 + 100 points, the pair (-1, 1) at order 1, nu = 0, d3 alone trained from
    2 x the truth.  S = 1000 Adam steps at step size 1e-2, chosen by running the helper's own Adam on the CPU: it ends at
    d3 = 0.019585 (distance 4.1e-4 of the starting 2e-2, and within 8.5e-4 from step 250 to 3000).  The raw d3 is of the size
    of the step: at 1e-3 (and 1e-4, 3e-4, 3e-3) the transient of the untrained net carries d3 to 0.3 ... 0.6 within 3000 steps,
    away from the truth, so the step size -- which the case leaves open -- is what was chosen; d3, the gap and the net are as
    specified.  No accuracy is asked of the engine, only that d3 ends nearer than it began; the other six are what they were"""
    from oracle import disc, init
    d3, t_0, t_1, q, layers = 0.02, 0.1, 0.9, 16, [1, 32, 32, 16]
    rs = np.random.RandomState(4321)
    u = lambda x, t: np.sin(np.pi * x + d3 * np.pi ** 3 * t)
    x_0, x_1 = rs.uniform(-1, 1, 100), rs.uniform(-1, 1, 100)
    A, b, _ = disc.gauss_legendre_butcher(q)
    dt = t_1 - t_0
    sets = [(x_0, u(x_0, t_0), dt * A), (x_1, u(x_1, t_1), -dt * (b[None, :] - A))]
    coef = (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 2.0 * d3)
    theta = add.pack(init.glorot_flat(layers), coef)
    eng = make_engine(layers, "f64", sets, theta, add.mask_of(["d3"]), ([-1.0], [1.0]), 1, coef=coef)
    try:
        eng.adam_init(1e-2, 0.9, 0.999, 1e-8)
        losses = eng.adam_run(1000)
        found = eng.get_pde_params()
        print("MEASURED dispersive: d3 %.6f after 1000 Adam steps (from %.2f, truth %.2f), loss %.3e -> %.3e" % (
            found[6], 2.0 * d3, d3, losses[0], losses[-1]))
        assert abs(found[6] - d3) < abs(2.0 * d3 - d3)
        assert np.array_equal(eng.get_weights()[-7:-1], np.zeros(6)) and np.array_equal(found[:6], np.zeros(6))
    finally:
        eng.close()


# ---- set_pde_params / get_pde_params -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_params_round_trip_and_predictions_follow_the_tail(dtype):
    from oracle import mlp
    sets, pairs, theta = add.case(LAYERS, Q, 17, 3, 3, seed=90, coef=_COEFS[7])
    eng = make_engine(LAYERS, dtype, sets, None, None, pairs, 1)
    try:
        start = eng.get_pde_params()
        assert start.shape == (7,) and np.array_equal(start[[0, 1, 3, 4, 5, 6]], np.array(ado.BURGERS + (0.0,))[[0, 1, 3, 4, 5, 6]])
        assert abs(start[2] - ado.BURGERS[2]) <= 1e-15 * ado.BURGERS[2]
        eng.set_weights(theta)
        xs = np.sort(np.random.RandomState(91).uniform(-1, 1, 37))
        ref_U = mlp.forward_value(mlp.unpack(theta[:-7], LAYERS), xs[:, None], np.array(LB), np.array(UB))

        def follows(coef, tag):
            got = eng.get_pde_params()
            assert np.array_equal(got[[0, 1, 3, 4, 5, 6]], np.array(coef)[[0, 1, 3, 4, 5, 6]]) and abs(got[2] - coef[2]) <= 1e-15 * coef[2]
            U = eng.predict(xs[:, None])
            assert np.max(np.abs(U - ref_U)) / max(1.0, np.max(np.abs(ref_U))) <= TOL_VALUE[dtype]
            th = add.pack(theta[:-7], coef)
            worst, helper = 0.0, 0.0
            for s in (0, 1):
                P = eng.disc_predict(s, xs)
                pred = add.stage_prediction(th, LAYERS, xs, LB, UB, sets[s][2])
                scale = max(1.0, np.max(np.abs(pred)))
                worst = max(worst, np.max(np.abs(P - pred)) / scale)
                if dtype == "f32":
                    p32 = add.stage_prediction(th, LAYERS, xs, LB, UB, sets[s][2], dtype=np.float32)
                    helper = max(helper, np.max(np.abs(p32 - pred)) / scale)
            tol = TOL_STAGE[dtype] if dtype == "f64" else f32_bound(TOL_STAGE[dtype], helper)
            print("MEASURED stage %s %s: %.3e (bound %.3e, helper f32 %.3e)" % (tag, dtype, worst, tol, helper))
            assert worst <= tol
            return eng.disc_predict(0, xs)

        P0 = follows(_COEFS[7], "set_weights")
        heavy = ado.REACTION_HEAVY + (-0.03,)
        eng.set_pde_params(*heavy)
        P1 = follows(heavy, "set_pde_params")
        assert np.max(np.abs(P1 - P0)) > 1e-2
        assert np.array_equal(eng.get_weights()[:-7], theta[:-7])
        eng.set_weights(add.pack(theta[:-7], _COEFS[6]))
        follows(_COEFS[6], "set_weights-again")
    finally:
        eng.close()


# ---- the script -------------------------------------------------------------------------------------------------------------------
LINE = re.compile(r"^(tf_epoch|nt_epoch) =\s+(\d+)\s+elapsed = \d\d:\d\d \(\+\d\d\.\d\)  loss = (\S+)  .*a1 = (\S+)  d3 = (\S+)")
END = re.compile(r"^Training finished \(epoch (\d+)\): duration = \d\d:\d\d  error = (\S+)  ")


def test_ide_disc_kdv_script_runs(tmp_path):
    """1d-kdv/ide_disc_kdv.py as a child process with a small hp file: exits 0, both optimiser phases logged with the a1 and d3
    columns, the last logged loss is below the first, and the identified coefficients are printed"""
    hp = {"N_0": 50, "N_1": 50, "q": 8, "layers": [1, 32, 32, 8], "tf_epochs": 20, "tf_lr": 0.001, "tf_b1": 0.9,
          "tf_eps": 1e-08, "nt_epochs": 20, "nt_lr": 0.8, "nt_ncorr": 50, "log_frequency": 10}
    hp_file = tmp_path / "hp.json"
    hp_file.write_text(json.dumps(hp))
    env = dict(os.environ, PINN_NO_PLOT="1", MPLBACKEND="Agg")
    res = subprocess.run([sys.executable, os.path.join(PKG, "1d-kdv", "ide_disc_kdv.py"), str(hp_file)],
                         cwd=PKG, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    out = res.stdout
    assert "Training started" in out and "-- Starting Adam optimization --" in out and "-- Starting LBFGS optimization --" in out
    rows = [(m.group(1), int(m.group(2)), float(m.group(3)), float(m.group(4)), float(m.group(5)))
            for m in map(LINE.match, out.splitlines()) if m]
    ends = [m for m in map(END.match, out.splitlines()) if m]
    assert any(r[0] == "tf_epoch" for r in rows) and any(r[0] == "nt_epoch" for r in rows), out[-2000:]
    assert len(ends) == 1 and int(ends[0].group(1)) == 20 and np.isfinite(float(ends[0].group(2)))
    assert np.isfinite(rows[-1][2]) and rows[-1][2] < rows[0][2], (rows[0], rows[-1])
    assert all(np.isfinite(r[3]) and np.isfinite(r[4]) for r in rows) and rows[-1][3] != 0.5 and rows[-1][4] != 0.005
    assert "identified coefficients" in out and re.search(r"nu = +0\.0+e\+00 .*frozen", out)
