"""GPU tests (pytest -m gpu) of the optimiser driver's rules that tests/test_gpu_async_log.py leaves open: a ticket collected by the
call of the other optimiser, the ticket of an L-BFGS run with max_iter = 0, the refusal of log arrays that are too short, and
an ensemble whose members stop at different iterations (and step at different rates) against contexts of their own, bit for
bit.  The small set of test_ticket_rules (N_u = 64, N_f = 2048, the 8 x 20 net), a few steps per call.

An ensemble hands out no lbfgs_x (the C API has no call for it), so the walk compares logs, done, weights and status; the
solo contexts' lbfgs_x is held against an unchunked run instead."""
import ctypes

import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu

NU = 0.01 / np.pi
LAYERS = [2] + [20] * 8 + [1]
EPS = float(np.finfo(float).eps)


@pytest.fixture(scope="module")
def small(burgers_sets):
    r = burgers_sets(64, 2048)
    return dict(X_u=r[7], u=r[8], X_f=r[9], ub=r[10], lb=r[11], w0=np.load(golden("burgers_eval.npz"))["w0"])


def _fill(eng, s):
    eng.set_collocation(s["X_f"]); eng.set_data(s["X_u"], s["u"]); eng.set_pde_params(NU)


def _engine(s, w=None, lr=0.03):
    from pinn_native import Engine
    eng = Engine(LAYERS, s["lb"], s["ub"], pde="burgers", dtype="f64")
    _fill(eng, s)
    eng.set_weights(s["w0"] if w is None else w)
    eng.adam_init(lr, 0.9, 0.999, 1e-7)
    return eng


def _members(s, K):
    return np.stack([s["w0"] * (1.0 + 0.01 * k) for k in range(K)])


def _ensemble(s, W):
    from pinn_native import Ensemble
    ens = Ensemble(LAYERS, s["lb"], s["ub"], len(W))
    _fill(ens, s)
    ens.set_weights(W)
    return ens


def test_a_ticket_is_refused_by_the_other_kinds_collect_and_stays_collectable(small):
    from pinn_native import PinnNativeError
    eng, ref = _engine(small), _engine(small)
    eng.lbfgs_begin(12, 0.8, 50, EPS)
    ref.lbfgs_begin(12, 0.8, 50, EPS)
    ta, tl = eng.adam_enqueue(2), eng.lbfgs_enqueue(3)               # both kinds in flight, the Adam chunk the oldest
    with pytest.raises(PinnNativeError, match="ticket %d belongs to an Adam chunk" % ta):
        eng.lbfgs_collect(ta)
    losses = eng.adam_collect(ta)                                    # refused, not consumed
    with pytest.raises(PinnNativeError, match="ticket %d belongs to an L-BFGS chunk" % tl):
        eng.adam_collect(tl)
    its, ls, done = eng.lbfgs_collect(tl)
    # the refusals changed nothing: the same chunks through the synchronous calls
    assert np.array_equal(losses, ref.adam_run(2)) and len(losses) == 2 and np.all(np.isfinite(losses))
    its_r, ls_r, done_r = ref.lbfgs_run(3)
    assert np.array_equal(its, its_r) and np.array_equal(ls, ls_r) and done == done_r
    assert len(its) <= 3 and np.all(np.isfinite(ls))
    assert np.array_equal(eng.get_weights(), ref.get_weights())
    assert len(eng.adam_run(1)) == 1                                 # nothing is left in flight
    eng.close(); ref.close()


def test_max_iter_zero_is_done_at_once_with_nothing_logged(small):
    eng = _engine(small)
    eng.adam_run(2)
    w = eng.get_weights()
    n_evals = eng.status()[0]
    eng.lbfgs_begin(0, 0.8, 50, EPS)
    its, ls, done = eng.lbfgs_collect(eng.lbfgs_enqueue(3))
    assert len(its) == 0 and len(ls) == 0 and done == 1
    its, ls, done = eng.lbfgs_run(3)
    assert len(its) == 0 and len(ls) == 0 and done == 1
    assert np.array_equal(eng.get_weights(), w) and eng.status() == (n_evals, 0)      # custom_lbfgs.py:43-44: nothing ran
    eng.close()


def test_log_arrays_one_entry_short_are_refused(small):
    from pinn_native import PinnNativeError, _c_int_p, _dp
    eng, ref = _engine(small), _engine(small)
    ref.lbfgs_begin(12, 0.8, 50, EPS)
    due = len(ref.lbfgs_run(5)[0])
    assert due == 5                                                  # one entry per iteration: no break on this set
    eng.lbfgs_begin(12, 0.8, 50, EPS)
    t = eng.lbfgs_enqueue(5)
    iters, losses = np.zeros(due, dtype=np.int32), np.zeros(due, dtype=np.float64)
    n_logged, done = ctypes.c_int(0), ctypes.c_int(0)
    with pytest.raises(PinnNativeError, match="%d log entries are due, the arrays hold %d" % (due, due - 1)):
        eng._check(eng._lib.pinn_lbfgs_collect(eng._h, t, due - 1, iters.ctypes.data_as(_c_int_p), _dp(losses),
                                               ctypes.byref(n_logged), ctypes.byref(done)))
    assert n_logged.value == 0 and not iters.any() and not losses.any()          # nothing was written
    eng.close(); ref.close()


def test_ensemble_members_that_end_at_different_iterations_equal_solo_contexts(small):
    K, max_iter = 3, [0, 3, 7]
    W = _members(small, K)
    ens = _ensemble(small, W)
    solo = [_engine(small, W[k]) for k in range(K)]
    ens.lbfgs_begin(max_iter, 0.8, 50, EPS)
    for k in range(K):
        solo[k].lbfgs_begin(max_iter[k], 0.8, 50, EPS)
    logged = [0] * K
    for chunk in range(3):                                           # 4 + 4 + 4 > 7: the last chunk issues nothing
        its, ls, done = ens.lbfgs_run(4)
        for k in range(K):
            i, l, d = solo[k].lbfgs_run(4)
            assert np.array_equal(its[k], i) and np.array_equal(ls[k], l) and done[k] == d, (chunk, k)
            logged[k] += len(i)
    assert logged == [0, 2, 6] and list(done) == [1, 1, 1]           # max_iter - 1 entries each: no break on this set
    Wf = ens.get_weights()
    n_evals, bad = ens.status()
    for k in range(K):
        assert np.array_equal(solo[k].get_weights(), Wf[k]), k
        assert solo[k].status() == (n_evals[k], bad[k]), k
    assert np.array_equal(Wf[0], W[0])
    # the chunked walk of a solo context against one call: the same kernels, so the same log, weights and x
    one = _engine(small, W[2])
    one.lbfgs_begin(7, 0.8, 50, EPS)
    i, l, d = one.lbfgs_run(12)
    assert list(i) == list(range(1, 7)) and d == 1
    assert np.array_equal(one.get_weights(), Wf[2]) and np.array_equal(one.lbfgs_x(), solo[2].lbfgs_x())
    one.close(); ens.close()
    for e in solo:
        e.close()


def test_ensemble_step_sizes_equal_solo_contexts(small):
    K, lr = 3, np.array([1e-3, 0.01, 0.03])
    W = _members(small, K)
    ens = _ensemble(small, W)
    ens.adam_init(lr, 0.9, 0.999, 1e-7)
    L = np.concatenate([ens.adam_run(n) for n in (5, 16, 3)])
    Wf = ens.get_weights()
    assert L.shape == (24, K) and np.all(np.isfinite(L))
    for k in range(K):
        eng = _engine(small, W[k], lr=lr[k])
        got = np.concatenate([eng.adam_run(5), eng.adam_collect(eng.adam_enqueue(16)), eng.adam_run(3)])
        assert np.array_equal(got, L[:, k]), k
        assert np.array_equal(eng.get_weights(), Wf[k]), k
        eng.close()
    ens.close()
