"""GPU: the device L-BFGS against the traced oracle on every stop rule and on the curvature branch.

The cases (tests/helpers/lbfgs_cases.py) end with each of the engine's seven `done` codes and keep and reject curvature
pairs; every decision the oracle makes is at least 1 % away from its threshold (tests/test_lbfgs_cases.py), so stop codes
and iteration lists are compared exactly.  Each case runs in both modes (0: k_lbfgs_step + k_lbfgs_post; 1: k_lbc_dots +
k_lbc_coef_apply, whose folded post-evaluation tests give way to k_lbfgs_post at the end of a chunk) and in four
chunkings, so that every stop decided behind an evaluation lands once inside a chunk and once on a chunk's end.  After the
stop, later chunks (and the chunk that ran ahead) must log nothing, report the same code and leave the weights and the
returned x bit-identical."""
import collections
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import lbfgs_cases as L  # noqa: E402

pytestmark = pytest.mark.gpu

# float32-kernel bounds of test_gpu_parity.py (F32_LBFGS_TOL): losses of the first 5 / 10 / all iterations, weights
F32_LBFGS_TOL = dict(loss5=1e-5, loss10=5e-5, loss25=1e-3, w_model=1e-3)
AHEAD = 3                      # iterations per chunk when two chunks are in flight


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300))


@pytest.fixture(scope="module")
def oracle_runs():
    cache = {}

    def get(case):
        if case.name not in cache:
            cache[case.name] = L.run_oracle(case)
        return cache[case.name]
    return get


def make_engine(p, dtype):
    from pinn_native import Engine
    eng = Engine(p["layers"], L.LB, L.UB, pde=p["pde"], dtype=dtype)
    if p["pde"] == "burgers":
        eng.set_collocation(p["X_f"])
        eng.set_data(p["X_u"], p["u"])
        eng.set_pde_params(L.NU)
    elif p["pde"] == "burgers_ide":
        eng.set_data(p["X_u"], p["u"])
    else:
        eng.set_collocation(p["X_f"])
        eng.set_data(p["X_u"], p["u"])
        eng.set_boundary(p["X_lb"], p["X_ub"])
    return eng


CHUNKINGS = ("whole", "one", "seven", "ahead")


def chunk_size(case, chunking):
    return {"whole": max(case.max_iter, 1), "one": 1, "seven": 7, "ahead": AHEAD}[chunking]


def drive(eng, case, chunking):
    """runs the case to its stop in one chunking -> (iters, losses, done); then checks that nothing moves any more"""
    eng.set_weights(L.problem(case.problem)["w0"])
    eng.lbfgs_begin(case.max_iter, case.lr, case.n_corr, case.tol_fun, case.tol_x, case.max_eval)
    its, los, done = [], [], 0
    n = chunk_size(case, chunking)
    if chunking == "ahead":
        tickets = collections.deque([eng.lbfgs_enqueue(n), eng.lbfgs_enqueue(n)])
        for _ in range(case.max_iter + 2):
            it, lo, done = eng.lbfgs_collect(tickets.popleft())
            its += it.tolist()
            los += lo.tolist()
            if done:
                break
            tickets.append(eng.lbfgs_enqueue(n))
        assert done and len(tickets) == 1
        it, lo, d2 = eng.lbfgs_collect(tickets.popleft())          # the chunk that ran ahead of the stop
        assert len(it) == 0 and len(lo) == 0 and d2 == done, (case.name, chunking, it, d2)
    else:
        for _ in range(case.max_iter + 2):
            it, lo, done = eng.lbfgs_run(n)
            its += it.tolist()
            los += lo.tolist()
            if done:
                break
        assert done, (case.name, chunking)
        if chunking == "whole":
            assert len(its) == len(los)
    w_stop = eng.get_weights()
    x_stop = eng.lbfgs_x() if case.max_iter else None
    for n_more in (1, 3, 7):                                        # later chunks: nothing logged, nothing moves
        it, lo, d2 = eng.lbfgs_run(n_more)
        assert len(it) == 0 and d2 == done, (case.name, chunking, n_more, it, d2)
        assert np.array_equal(eng.get_weights(), w_stop), (case.name, chunking, n_more)
        if x_stop is not None:
            assert np.array_equal(eng.lbfgs_x(), x_stop), (case.name, chunking, n_more)
    return its, los, done, w_stop, x_stop


def check_against_oracle(case, res, tr, its, los, done, w, x, chunking, mode, loss_bounds, w_bound):
    w0 = L.problem(case.problem)["w0"]
    assert done == L.engine_done(case, tr), (case.name, mode, chunking, done, tr["reason"])
    if res is None:                                                 # max_iter == 0: nothing changes
        assert its == [] and np.array_equal(w, w0)
        return 0.0, 0.0
    want_it = [i for i, _ in res["logs"]]
    assert its == want_it, (case.name, mode, chunking, its, want_it)
    dl = 0.0
    if want_it:
        want_lo = np.array([f for _, f in res["logs"]])
        d = np.abs(np.array(los) - want_lo) / np.abs(want_lo)
        for upto, bound in loss_bounds:
            assert d[:upto].max() < bound, (case.name, mode, chunking, upto, d[:upto].max())
        dl = float(d.max())
    if L.stop_iteration(tr) <= 1 and case.code in (2, 7):          # stopped before the first step: w0 bit for bit
        assert np.array_equal(w, w0) and np.array_equal(x, w0), (case.name, mode, chunking)
    dw = max(rel(w, res["x_model"]), rel(x, res["x"]))
    assert rel(w, res["x_model"]) < w_bound and rel(x, res["x"]) < w_bound, (case.name, mode, chunking, dw)
    return dl, dw


_f64_done = collections.defaultdict(set)     # mode -> done codes the f64 cases produced on the device
_f64_ran = collections.defaultdict(set)      # mode -> names of the f64 cases that passed


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("case", L.CASES, ids=[c.name for c in L.CASES])
def test_f64_case_matches_oracle_in_every_chunking(case, mode, oracle_runs, record):
    res, tr = oracle_runs(case)
    eng = make_engine(L.problem(case.problem), "f64")
    eng.lbfgs_set_mode(mode)
    worst_l = worst_w = 0.0
    for chunking in CHUNKINGS:
        its, los, done, w, x = drive(eng, case, chunking)
        dl, dw = check_against_oracle(case, res, tr, its, los, done, w, x, chunking, mode, [(None, 1e-8)], 1e-7)
        worst_l, worst_w = max(worst_l, dl), max(worst_w, dw)
    _f64_done[mode].add(done)
    _f64_ran[mode].add(case.name)
    record(case=case.name, mode=mode, loss_dev=worst_l, weight_dev=worst_w)
    eng.close()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("case", [c for c in L.CASES if c.f32], ids=[c.name for c in L.CASES if c.f32])
def test_f32_rounding_free_case_matches_oracle(case, mode, oracle_runs, record):
    """float32 kernels, float64 optimiser state: the cases whose outcome does not depend on rounding"""
    res, tr = oracle_runs(case)
    eng = make_engine(L.problem(case.problem), "f32")
    eng.lbfgs_set_mode(mode)
    bounds = [(5, F32_LBFGS_TOL["loss5"]), (10, F32_LBFGS_TOL["loss10"]), (None, F32_LBFGS_TOL["loss25"])]
    for chunking in CHUNKINGS:
        its, los, done, w, x = drive(eng, case, chunking)
        dl, dw = check_against_oracle(case, res, tr, its, los, done, w, x, chunking, mode, bounds,
                                      F32_LBFGS_TOL["w_model"])
        record(case=case.name, mode=mode, chunking=chunking, loss_dev=dl, weight_dev=dw)
    eng.close()


def test_every_post_evaluation_stop_lands_inside_a_chunk_and_on_a_chunk_end(oracle_runs):
    """codes 3-6 are decided behind an evaluation: by k_lbc_coef_apply's folded tests when the chunk goes on, by
    k_lbfgs_post when it ends there (mode 1).  Each such case meets both across CHUNKINGS."""
    for case in L.CASES:
        if case.code not in (3, 4, 5, 6):
            continue
        k = L.stop_iteration(oracle_runs(case)[1])
        ends = {k % chunk_size(case, ch) == 0 for ch in CHUNKINGS}
        assert ends == {True, False}, (case.name, k)


def test_f64_cases_cover_every_code_in_both_modes(oracle_runs):
    """the f64 cases above run in both modes and between them end with every done code 1..7; where they have run in
    this session (pytest keeps file order), the device produced every code in each mode"""
    assert {L.engine_done(c, oracle_runs(c)[1]) for c in L.CASES} == {1, 2, 3, 4, 5, 6, 7}
    for mode in (0, 1):
        ran = _f64_ran[mode]
        if ran == {c.name for c in L.CASES}:
            assert _f64_done[mode] == {1, 2, 3, 4, 5, 6, 7}, (mode, sorted(_f64_done[mode]))


def test_ensemble_members_stop_like_solo_engines_and_the_oracle(oracle_runs):
    """K = 4 members with their own sets, starts, max_iter and lr stop with four codes on four iterations inside one
    lbfgs_run chunk: each equals a solo engine bit for bit and the oracle's reason, and a stopped member's weights stay
    bit-identical over every later chunk"""
    import pinn_native
    cases = L.ensemble_cases()
    e = L.ENSEMBLE
    probs = [L.problem(c.problem) for c in cases]
    layers, K = probs[0]["layers"], len(cases)
    ens = pinn_native.Ensemble(layers, L.LB, L.UB, K, pde="burgers")
    ens.set_collocation(np.stack([p["X_f"] for p in probs]))
    ens.set_data(np.stack([p["X_u"] for p in probs]), np.stack([p["u"] for p in probs]))
    ens.set_pde_params(np.full(K, L.NU))
    W0 = np.stack([p["w0"] for p in probs])
    ens.set_weights(W0)
    max_iter = np.array([c.max_iter for c in cases], dtype=np.int32)
    lr = np.array([c.lr for c in cases])
    ens.lbfgs_begin(max_iter, lr, e["n_corr"], e["tol_fun"], e["tol_x"], e["max_eval"])
    n_chunk = int(max_iter.max())
    its, los, done = ens.lbfgs_run(n_chunk)                        # every member stops inside this chunk
    W = ens.get_weights()
    for k, (c, p) in enumerate(zip(cases, probs)):
        res, tr = oracle_runs(c)
        assert done[k] == L.engine_done(c, tr), (k, done[k], tr["reason"])
        assert its[k].tolist() == [i for i, _ in res["logs"]], k
        eng = make_engine(p, "f64")
        assert eng.kernel_path() == 7
        eng.set_weights(p["w0"])
        eng.lbfgs_begin(c.max_iter, c.lr, c.n_corr, c.tol_fun, c.tol_x, c.max_eval)
        it, lo, d = eng.lbfgs_run(n_chunk)
        assert d == done[k] and np.array_equal(it, its[k]) and np.array_equal(lo, los[k]), k
        assert np.array_equal(eng.get_weights(), W[k]), k
        assert rel(W[k], res["x_model"]) < 1e-7, k
        if c.code == 7:
            assert np.array_equal(W[k], p["w0"]), k
        eng.close()
    assert len(set(done.tolist())) == K
    for n_more in (1, 5):                                          # stopped members stay frozen
        it2, lo2, d2 = ens.lbfgs_run(n_more)
        assert all(len(a) == 0 for a in it2) and np.array_equal(d2, done), n_more
        assert np.array_equal(ens.get_weights(), W), n_more
    ens.close()
