"""CPU: the shared L-BFGS case table (tests/helpers/lbfgs_cases.py) reaches the branch each case claims, with every
floating-point decision of the traced oracle at least MARGIN away from its threshold -- the property that lets
tests/test_gpu_lbfgs_branches.py compare the device's stop codes and iteration lists exactly."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import lbfgs_cases as L  # noqa: E402

_runs = {}


def traced(case):
    if case.name not in _runs:
        _runs[case.name] = L.run_oracle(case)
    return _runs[case.name]


@pytest.mark.parametrize("case", L.CASES, ids=[c.name for c in L.CASES])
def test_case_reaches_its_branch_with_margin(case):
    res, tr = traced(case)
    if case.max_iter == 0:
        assert res is None and tr["reason"] == 0 and tr["iters"] == []
        return
    assert tr["reason"] == case.code, (case.name, tr["reason"])
    k = L.stop_iteration(tr)
    if case.code == 7:
        assert k == 0 and tr["n_eval"] == 1
    elif case.code == 1:
        assert k == case.max_iter
    elif case.code in (3, 4, 5, 6):                   # decided behind an evaluation, in the middle of the run
        assert 1 <= k < case.max_iter
    if case.code == 2 and case.name.startswith("c2_first"):
        assert k == 1
    if case.code == 3:
        assert case.max_eval < 1.25 * case.max_iter and tr["n_eval"] == int(np.ceil(case.max_eval))
    kept = [r["kept"] for r in tr["iters"] if r["kept"] is not None]
    if case.mixed:
        assert any(kept) and not all(kept), case.name
    # n_iter / n_eval are integers (decided exactly everywhere); every floating-point comparison needs the margin
    ds = L.decisions(case, tr)
    assert ds
    worst = min(ds, key=lambda d: d[2])
    assert worst[2] >= L.MARGIN, "%s: %s on iteration %d is decided by a relative margin of %.3g only" % (
        case.name, worst[0], worst[1], worst[2])
    # the log is what the engine must reproduce: one entry per iteration that passed every test
    assert [i for i, _ in res["logs"]] == [r["n_iter"] for r in tr["iters"] if r["df"] is not None and
                                           r["n_iter"] != k]


def test_the_table_covers_every_branch_and_shape():
    codes = {c.code for c in L.CASES}
    assert codes == {1, 2, 3, 4, 5, 6, 7}
    assert {c.max_iter for c in L.CASES} >= {0, 1, 2}
    ev = [c.max_eval for c in L.CASES if c.code == 3]
    assert any(e == int(e) for e in ev) and any(e != int(e) for e in ev)
    assert {c.n_corr for c in L.CASES if c.mixed} >= {1, 3, 61, 62}
    sizes = {L.n_params(L.PROBLEMS[c.problem].layers, L.PROBLEMS[c.problem].pde) for c in L.CASES}
    assert sizes >= {501, 3021, 3023, 5301, 30802}
    assert any(c.code == 2 and traced(c)[1]["iters"] and L.stop_iteration(traced(c)[1]) == 1 for c in L.CASES)
    assert any(c.code == 2 and L.stop_iteration(traced(c)[1]) > 1 for c in L.CASES)


def test_tol_fun_and_step_tests_fire_together_once():
    """the order of the tests behind an evaluation matters only where two of them hold at once"""
    c = L.by_name("c4_before_5")
    r = traced(c)[1]["iters"][-1]
    assert r["g_abs"] <= c.tol_fun and r["s_abs"] is None
    res = L.run_oracle(c._replace(tol_fun=L.DEFAULT_TOL_FUN))[1]
    assert res["reason"] == 5 and L.stop_iteration(res) == L.stop_iteration(traced(c)[1])


def test_the_ring_wraps_between_rejections():
    """n_corr = 1 and 3: more pairs are kept than the ring holds, and for n_corr = 3 a pair is kept after a rejection
    once the ring is full"""
    for name, m in (("cv_n1", 1), ("cv_n3", 3)):
        kept = [r["kept"] for r in traced(L.by_name(name))[1]["iters"] if r["kept"] is not None]
        assert sum(kept) > m + 1
    kept = [r["kept"] for r in traced(L.by_name("cv_n3"))[1]["iters"] if r["kept"] is not None]
    first_reject = kept.index(False)
    assert sum(kept[:first_reject]) > 3 and any(kept[first_reject:])


def test_trace_leaves_the_result_unchanged():
    from oracle import optim
    c = L.by_name("cv_n3")
    p = L.problem(c.problem)
    a = optim.lbfgs(p["loss_grad"], p["w0"].copy(), 8, c.lr, c.n_corr)
    b = optim.lbfgs(p["loss_grad"], p["w0"].copy(), 8, c.lr, c.n_corr, trace={})
    assert np.array_equal(a["x"], b["x"]) and np.array_equal(a["x_model"], b["x_model"])
    assert a["logs"] == b["logs"] and a["n_eval"] == b["n_eval"] and a["final_loss"] == b["final_loss"]


def test_ensemble_members_stop_with_different_codes_on_different_iterations():
    cases = L.ensemble_cases()
    assert len(cases) >= 4
    seen = set()
    for c, m in zip(cases, L.ENSEMBLE["members"]):
        res, tr = traced(c)
        assert tr["reason"] == m[3] and L.stop_iteration(tr) == m[4], (c.name, tr["reason"], L.stop_iteration(tr))
        worst = min(L.decisions(c, tr), key=lambda d: d[2])
        assert worst[2] >= L.MARGIN, (c.name, worst)
        seen.add((m[3], m[4]))
    assert len({s[0] for s in seen}) == len(cases) and len({s[1] for s in seen}) == len(cases)
    shapes = {(L.PROBLEMS[c.problem].layers[1:-1] == [20] * 8, L.PROBLEMS[c.problem].n_f, L.PROBLEMS[c.problem].n_u)
              for c in cases}
    assert shapes == {(True, 256, 48)}             # pinn_ens_* takes one net shape and equal per-member set sizes
