"""CPU: pins tests/helpers/optim_tail.py, on which tests/test_gpu_optim_tail.py rests.

  * the table of parameter counts: every listed n is what the formulas give for its net and what the oracle's weight
    vector holds, every seam the optimiser kernels have in n is occupied, and no admissible net has n = 4097;
  * the float64 "vector" restatement of L-BFGS is oracle.optim.lbfgs bit for bit, on every case and both ring sizes;
    the "compact" restatement (the algebra of k_lbc_coef_apply) gives the same directions in longdouble;
  * the Adam allowance K_A u (|w| + |step|) holds for oracle.optim.Adam's plain float64 arithmetic on the oracle's own
    gradients, against the longdouble statements fed the same gradients;
  * no stop rule and no y.s test comes within 1 % of its threshold inside the iterations the device test runs (the rule
    of tests/test_lbfgs_cases.py), with the CPU oracle's loss and gradient.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import optim_tail as ot  # noqa: E402

IDS = [ot.case_id(c) for c in ot.TABLE]
LB_RUNS = [(c, m) for c in ot.TABLE for m in ot.LBFGS["n_corr"]]
LB_IDS = ["%s-m%d" % (ot.case_id(c), m) for c, m in LB_RUNS]
# the restatement is closed over max_iter = iterations + 1: eight evaluated iterations and the last, unevaluated one,
# whose y.s and gtd tests are held to the margin too; the device runs the same eight under a larger max_iter
CLOSED_ITERS = ot.LBFGS["iters"] + 1

_runs = {}


def oracle_run(c, n_corr):
    """oracle.optim.lbfgs on the case -> (result, trace, [(x, f, g) of every evaluation])"""
    key = (c.n, n_corr)
    if key not in _runs:
        from oracle import optim
        b = ot.build(c)
        evals = []

        def opfunc(x):
            f, g = b["loss_grad"](x)
            evals.append((np.array(x, copy=True), f, np.array(g, copy=True)))
            return f, g
        trace = {}
        res = optim.lbfgs(opfunc, b["w0"].copy(), CLOSED_ITERS, ot.LBFGS["lr"], n_corr, trace=trace)
        _runs[key] = (res, trace, evals)
    return _runs[key]


def test_the_table_lists_the_counts_the_formulas_give():
    want = [5, 12, 60, 61, 62, 63, 65, 127, 129, 192, 1536, 255, 257, 1021, 1023, 1027, 2047, 2048, 2049, 2051, 4093, 4095,
            4096, 4098, 4099, 5117, 5121, 5122, 5695, 5697, 6077]
    assert [c.n for c in ot.TABLE] == want
    for c in ot.TABLE:
        assert ot.count(c) == c.n, c
        assert (c.pde, c.W, c.H, c.n_out) in ot.find(c.n), c
    assert set(ot.IDENTITY_N) <= set(want)
    assert ot.find(4097) == []                     # nothing to add between the last <2> and the first <1> size


def test_every_seam_in_n_is_occupied():
    ns = np.array([c.n for c in ot.TABLE])
    assert {0, 1, 60, 61, 62, 63} <= set((ns % 64).tolist())                 # reduction blocks and k_lbc_coef_apply
    assert {255, 1} <= set((ns % 256).tolist())                              # k_adam
    assert np.any(ns < 64) and {1023, 1027} <= set(ns.tolist()) and 1021 in ns          # 1024-thread stride loops
    assert np.any(ns <= 2048) and {2047, 2048, 2049, 2051} <= set(ns.tolist())           # second half of <2>
    assert {4093, 4095, 4096, 4098, 4099} <= set(ns.tolist())                # the <2> / <1> threshold, tails of 2 and 3
    assert np.any((ns > 4096) & (ns < 5120)) and np.sum(ns >= 5120) >= 2     # tail loop within / beyond a stride
    p8 = [c for c in ot.TABLE if c.W > 64 and 2 <= c.H <= 4]                  # float64 path 8 (engine.hip t16_fused)
    assert {c.n % 64 for c in p8} == {63, 1, 61} and all(c.also_path0 for c in p8)
    assert all(c.also_path0 for c in ot.TABLE if (c.W, c.H) == (15, 5))
    assert {c.pde for c in ot.TABLE} == {"burgers", "burgers_ide", "schrodinger", "adr_ide", "burgers_disc"}
    assert len(ot.configs()) == 2 * (len(ot.TABLE) + 6)


@pytest.mark.parametrize("c", ot.TABLE, ids=IDS)
def test_a_case_builds_with_its_count_and_a_finite_gradient(c):
    b = ot.build(c)
    f, g = b["loss_grad"](b["w0"])
    assert g.shape == (c.n,) and np.isfinite(f) and np.all(np.isfinite(g))
    for i in ot.frozen_entries(b):
        assert g[i] == 0.0
    if c.pde == "adr_ide":
        assert len(ot.frozen_entries(b)) == 4
        assert ot.frozen_entries(b) == [c.n - 6, c.n - 5, c.n - 4, c.n - 2]
        assert g[-3] != 0.0 and g[-1] != 0.0        # r1 and r3 are trained: the last entry of theta is live


@pytest.mark.parametrize("c,n_corr", LB_RUNS, ids=LB_IDS)
def test_float64_restatement_is_the_oracle_bit_for_bit(c, n_corr):
    res, trace, evals = oracle_run(c, n_corr)
    it = iter(evals)

    def replay(x):                                 # the restatement must ask for the very same points
        xe, f, g = next(it)
        assert np.array_equal(x, xe)
        return f, g
    mine, L = ot.run_closed(replay, ot.build(c)["w0"], CLOSED_ITERS, ot.LBFGS["lr"], n_corr)
    assert np.array_equal(mine["x"], res["x"]) and np.array_equal(mine["x_model"], res["x_model"])
    assert mine["f_hist"] == res["f_hist"] and mine["logs"] == res["logs"]
    assert mine["n_eval"] == res["n_eval"] == trace["n_eval"] and mine["final_loss"] == res["final_loss"]
    assert L.done == trace["reason"] == 1 and L.trace == trace["iters"] and L.g0_abs == trace["g0_abs"]
    assert [i for i, _ in mine["logs"]] == list(range(1, ot.LBFGS["iters"] + 1))


@pytest.mark.parametrize("c,n_corr", LB_RUNS, ids=LB_IDS)
def test_no_decision_within_one_percent_of_its_threshold(c, n_corr):
    _, trace, _ = oracle_run(c, n_corr)
    ds = ot.decisions(trace["iters"], trace["g0_abs"])
    assert len(ds) >= 1 + 2 * ot.LBFGS["iters"]
    worst = min(ds, key=lambda d: d[2])
    assert worst[2] >= ot.MARGIN, "%s: %s on iteration %d is decided by a relative margin of %.3g only" % (
        ot.case_id(c), worst[0], worst[1], worst[2])
    kept = [r["kept"] for r in trace["iters"] if r["kept"] is not None]
    if n_corr == 3:
        assert sum(kept) > 3, "the ring of 3 must wrap inside the iterations run"


@pytest.mark.parametrize("c,n_corr", LB_RUNS, ids=LB_IDS)
def test_compact_restatement_gives_the_vector_directions(c, n_corr):
    """both forms in longdouble, fed the oracle's evaluations: same decisions, directions equal to far below float64's
    rounding of either; and the float64 run of each form stays within sight of its longdouble run (a finite yardstick)"""
    _, _, evals = oracle_run(c, n_corr)
    objs = {(form, dt): ot.Lbfgs(ot.LBFGS["max_iter"], ot.LBFGS["lr"], n_corr, dt, form)
            for form in ("vector", "compact") for dt in (np.longdouble, np.float64)}
    for L in objs.values():
        L.begin(evals[0][1], evals[0][2])
    for k in range(ot.LBFGS["iters"]):
        td = {key: L.step() for key, L in objs.items()}
        assert all(v is not None for v in td.values())
        tv, dv = td[("vector", np.longdouble)]
        tc, dc = td[("compact", np.longdouble)]
        assert tv == tc
        scale = float(np.max(np.abs(dv)))
        assert float(np.max(np.abs(dv - dc))) <= 1e-12 * scale, (k, float(np.max(np.abs(dv - dc))) / scale)
        for form in ("vector", "compact"):
            yard, x_ref = ot.yardstick(evals[k][0], td[(form, np.longdouble)], td[(form, np.float64)])
            assert np.isfinite(yard) and yard <= 1e-6 * max(float(np.max(np.abs(x_ref))), 1e-300), (form, k, yard)
        for L in objs.values():
            assert L.evaluated(evals[k + 1][1], evals[k + 1][2]) == 0
    for L in objs.values():
        assert L.kept == objs[("vector", np.float64)].kept and [i for i, _ in L.logs] == list(range(1, ot.LBFGS["iters"] + 1))


@pytest.mark.parametrize("eps", ot.ADAM["eps"])
@pytest.mark.parametrize("c", ot.TABLE, ids=IDS)
def test_adam_allowance_holds_for_the_oracle_arithmetic(c, eps):
    from oracle import optim
    b = ot.build(c)
    A = ot.ADAM
    plain = optim.Adam(A["lr"], A["b1"], A["b2"], eps)
    wide = ot.AdamWide(c.n, A["b1"], A["b2"], eps)
    w = b["w0"].copy()
    worst = 0.0
    for t in range(1, A["steps"] + 1):
        _, g = b["loss_grad"](w)
        w_new = plain.step(w, g)
        alpha = ot.adam_alpha(A["lr"], A["b1"], A["b2"], t)
        assert alpha == A["lr"] * np.sqrt(1.0 - A["b2"] ** t) / (1.0 - A["b1"] ** t)
        w_ref, step = wide.step(w, g, alpha)
        ratio, i = ot.adam_excess(w_new, w_ref, ot.adam_allowance(w, step))
        assert ratio <= 1.0, "step %d entry %d is off by %.3g of its allowance" % (t, i, ratio)
        worst = max(worst, ratio)
        for i in ot.frozen_entries(b):
            assert w_new[i] == w[i] and step[i] == 0.0
        assert np.any(w_new != w)
        w = w_new
    assert worst > 0.0                             # the allowance is on the scale of the rounding it bounds


def test_adam_allowance_is_not_slack_enough_to_hide_a_wrong_entry():
    """what the device test must be able to see: a gradient entry taken from its neighbour, one step applied with the
    previous step's alpha, eps forgotten -- each is far outside the allowance"""
    c = ot.by_n(257)
    b = ot.build(c)
    A = ot.ADAM
    _, g = b["loss_grad"](b["w0"])
    w = b["w0"]
    for eps in A["eps"]:
        wide = ot.AdamWide(c.n, A["b1"], A["b2"], eps)
        w_ref, step = wide.step(w, g, ot.adam_alpha(A["lr"], A["b1"], A["b2"], 1))
        allow = ot.adam_allowance(w, step)
        g_bad = g.copy()
        g_bad[-1] = g[-2]
        for w_bad in (ot.AdamWide(c.n, A["b1"], A["b2"], eps).step(w, g_bad, ot.adam_alpha(A["lr"], A["b1"], A["b2"], 1))[0],
                      ot.AdamWide(c.n, A["b1"], A["b2"], eps).step(w, g, ot.adam_alpha(A["lr"], A["b1"], A["b2"], 2))[0],
                      ot.AdamWide(c.n, A["b1"], A["b2"], 0.0).step(w, g, ot.adam_alpha(A["lr"], A["b1"], A["b2"], 1))[0]):
            assert ot.adam_excess(w_bad.astype(np.float64), w_ref, allow)[0] > 1e3
