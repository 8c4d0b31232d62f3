"""GPU: the reduction and optimiser tail (csrc/kernels_optim.h) swept over parameter counts n placed at its block edges --
the table of tests/helpers/optim_tail.py, pinned on the CPU by tests/test_optim_tail_host.py.  31 nets, float64 and float32,
each on the path the engine chooses; the 15x5, 73x2 and 75x2 nets on path 0 as well: 74 configurations.

Lockstep.  Each case uses two contexts with the same sets and path: E, the optimiser under test, and a twin T on which only
set_weights and loss_grad are ever called.  After every single optimiser step E's iterate is handed to T, which returns the
loss, the terms and the gradient the step kernel itself saw (evaluations are bit-reproducible across contexts).  The loss
kernel's rounding is thereby out of the comparison: what is left is the optimiser's own arithmetic on float64 inputs.

Adam, 6 steps, lr 1e-3, b1 0.9, b2 0.999, eps 1e-7 and 1e-3 (test_adam_lockstep):
 (a) the terms of adam_run_terms(1) are np.array_equal to T's terms, the loss of adam_run(1) == T's loss (the two calls
     alternate over the steps, and start the other way round in the second eps run): k_reduce_adam against k_reduce_rows;
 (b) every new weight against adam_entry's statements in longdouble fed the device's gradients, m and v carried in longdouble,
     allowance K_A u (|w| + |step|) per entry, K_A = 36 derived in the helper's docstring;
 (c) adam_run(6) on a fresh context has the bits of the six single calls, losses and weights;
 (d) the frozen adr_ide coefficients keep their bits.
L-BFGS, modes 0 and 1, n_corr 3 (the ring wraps) and 50, 8 iterations of lbfgs_run(1), lr 0.8, max_iter 20
(test_lbfgs_lockstep):
 (a) every logged loss == T's loss at that iterate;
 (b) get_weights() is np.array_equal to lbfgs_x() while an evaluation follows;
 (c) x_{k+1} against x_k(device) + t d of the longdouble restatement (mode 0: the vector recursion; mode 1: the compact
     form's own algebra), deviation <= K_L x yardstick, the yardstick measured on the restatement (optim_tail.yardstick);
 (d) iteration numbers and `done` equal the restatement's.  The state's hist_len is not readable through the C ABI; a pair
     the device kept or dropped against the restatement's decision changes d by orders of magnitude more than (c) allows,
     and the host test shows every y.s at least 1 % away from 1e-10.
Identities without a tolerance, on the 62, 63, 255, 257, 4095 and 4099 nets (test_world1_*, test_used_context_*,
test_snapshot_*): a world-1 communicator (reduce, all-reduce, k_adam) leaves Adam's losses and weights and both L-BFGS modes'
logs and weights bit-equal; a used context walked through lbfgs_begin(n_corr = 7), (3), (20), five iterations each, and
adam_init with three steps is bit-equal to fresh contexts at every step; weights_restore behind three Adam steps brings back
the bits of the first loss_grad.  The 4099 net is adr_ide, which the engine refuses a communicator by design
(single_device_only, engine.hip): that refusal is asserted, and the 5121 net stands in beyond 4096 for the communicator.

Measured on an MI355X (profiles/optim_tail_measured.jsonl, written through the `record` fixture: one line per configuration
and run, the ratios of its steps in order).  No seam failed: all 494 tests pass, every identity holds bit for bit.

L-BFGS (c), largest ratio deviation / yardstick per dtype and mode over all configurations, both ring sizes, 8 iterations:

  dtype mode  largest  where
  f64   0     1.66     n 255 (burgers_ide 63x1), n_corr 3, iteration 7;  n 63: 1.65 (n_corr 50, iteration 5)
  f64   1     1.66     the same case and iteration
  f32   0     1.75     n 5697 (burgers_ide 73x2, path 4), n_corr 3, iteration 7;  n 4095: 1.61;  on path 0: 1.57
  f32   1     1.75     the same case and iteration

  per n, the largest over dtypes, paths, modes and ring sizes:
  5: 0.72   12: 0.32   60: 0.43   61: 1.12   62: 0.60   63: 1.65   65: 1.42   127: 0.81   129: 1.25   192: 0.93   255: 1.66
  257: 1.23   1021: 0.64   1023: 1.43   1027: 0.42   1536: 1.05   2047: 0.51   2048: 0.98   2049: 0.45   2051: 1.31
  4093: 1.20   4095: 1.61   4096: 1.26   4098: 0.90   4099: 0.48   5117: 1.22   5121: 1.31   5122: 1.51   5695: 1.11
  5697: 1.75   6077: 1.18

K_L = 4: the smallest power of two that is at least twice the largest measured ratio (2 x 1.75 = 3.5).  The two modes give the
same figure to three digits almost everywhere: a step is small against the iterate, so the deviation is the rounding of
x + t d itself (at most u |x_i|, i.e. 2 of the yardstick's u / 2 max |x|), on which the error of d hardly shows; what the
bound has room for beside that rounding is an error of d of 2 u max |x| / max |t d|, about 1e-13 of d, where an element, a
pair or a ring row lost at a seam moves d by 1 / n or more.  Seven pairs are kept in the 8 iterations of every case but the
4096 and 4098 nets (six: one y.s below 1e-10 there, decided with the host test's margin), so both branches run; n_corr 3 wraps.

Adam (b), largest ratio deviation / allowance (K_A = 36) over the six steps:  eps 1e-7: 0.25 in float64 (n 4093, step 5) and
0.25 in float32 (n 5695, path 4, step 6);  eps 1e-3: 0.07 in both.  Nine roundings where the worst case allows 36.

Paths met: 4 for the continuous nets (0 for adr_ide and, where asked, for the 15x5, 73x2 and 75x2 nets), 8 for the 73x2 and
75x2 nets in float64, 1 for the 20x13 net in float32, 0 for the discrete-time nets.

What the sweep sees.  A variant library with six mutants of kernels_optim.h, each of which only skips work at one seam, was
run against this file (not kept): 222 of the 494 tests fail, each mutant at exactly the n it touches and nowhere else.
  * k_lbc_dots: the `else if (i < n)` branch leaves the last element of an odd n out of the history operands: mode 1 fails at
    every odd n <= 4095 (5, 61, 63, 65, 127, 129, 255, 257, 1021, 1023, 1027, 2047, 2049, 2051, 4093, 4095), mode 0 passes;
  * k_lbc_dots<1>: the tail loop stops one element early: mode 1 fails at 4098, 4099, 5117, 5121, 5122, 5695, 5697, 6077;
  * k_lbfgs_step: y.s and y.y lose the last element where n mod 1024 = 3: mode 0 fails at 1027, 2051, 4099 only;
  * k_lbc_coef_apply: the lone weight of the last workgroup is not updated where n mod 64 = 1: mode 1 at 65 ... 5697;
  * k_reduce_adam: a loss slot that is the first column of a block is not handed to loss3: (a) fails at the twelve nets with
    n mod 64 in {62, 63, 0}, and the communicator and used-context identities fail with it;
  * k_adam: the lone weight of the last block is skipped where n mod 256 = 1: the communicator identity fails at 257 and 5121.
  (With nu and r1 trained the 1027 and 4099 nets saw none of the first three: their last entries were frozen, s = y = 0.  The
  trained pair is r1, r3 for that reason.)

Two findings on the way, both orderings between the context's non-blocking stream and the null stream, neither a seam in n:
pinn_lbfgs_get_x copied on the null stream, so lbfgs_x() straight behind lbfgs_begin did not wait for the copy of the start
into the iterate; disc_ensure cleared the partial rows with hipMemset on the null stream, which is not ordered before the first
evaluation's kernels -- the 4098 net's first Adam step had a gradient entry of the output layer wiped (weight 2279, the same
entry in two runs, gone with the clear in stream order).  Both are stream-ordered now (engine.hip).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import optim_tail as ot  # noqa: E402

pytestmark = pytest.mark.gpu

K_L = 4.0
CONFIGS = ot.configs()
CONFIG_IDS = [ot.config_id(k) for k in CONFIGS]
A, LBF = ot.ADAM, ot.LBFGS
IDENT = [(n, d) for n in ot.IDENTITY_N for d in ("f64", "f32")]
IDENT_IDS = ["n%d-%s" % k for k in IDENT]
COMM = IDENT + [(5121, "f64"), (5121, "f32")]
COMM_IDS = ["n%d-%s" % k for k in COMM]


def sig(v):
    return float("%.4g" % v)


@pytest.mark.parametrize("run", [0, 1], ids=["eps1e-7", "eps1e-3"])
@pytest.mark.parametrize("cfg", CONFIGS, ids=CONFIG_IDS)
def test_adam_lockstep(cfg, run, record):
    c, dtype, path = cfg
    eps = A["eps"][run]
    b = ot.build(c)
    E, T, F = (ot.make_engine(b, dtype, path) for _ in range(3))
    frozen = ot.frozen_entries(b)
    wide = ot.AdamWide(c.n, A["b1"], A["b2"], eps)
    E.adam_init(A["lr"], A["b1"], A["b2"], eps)
    singles, ratios = [], []
    for t in range(1, A["steps"] + 1):
        w = E.get_weights()
        T.set_weights(w)
        loss, g, terms = T.loss_grad()
        if (t + run) % 2:                                        # (a)
            te = E.adam_run_terms(1)[0]
            assert np.array_equal(te, terms), (t, te, terms)
            singles.append(te[0] + te[1] + te[2])
        else:
            le = E.adam_run(1)[0]
            assert le == loss, (t, le, loss)
            singles.append(le)
        w_new = E.get_weights()
        w_ref, step = wide.step(w, g, ot.adam_alpha(A["lr"], A["b1"], A["b2"], t))
        ratio, i = ot.adam_excess(w_new, w_ref, ot.adam_allowance(w, step))   # (b)
        ratios.append(sig(ratio))
        assert ratio <= 1.0, "step %d: weight %d of %d is off by %.3g of its allowance" % (t, i, c.n, ratio)
        assert np.any(w_new != w)
        for i in frozen:                                         # (d)
            assert w_new[i] == b["w0"][i]
    record(n=c.n, dtype=dtype, path=E.kernel_path(), eps=eps, K_A=ot.K_A, adam_ratios=ratios)
    F.adam_init(A["lr"], A["b1"], A["b2"], eps)                  # (c)
    assert np.array_equal(F.adam_run(A["steps"]), np.array(singles))
    assert np.array_equal(F.get_weights(), E.get_weights())
    assert E.status()[1] == 0
    for e in (E, T, F):
        e.close()


@pytest.mark.parametrize("n_corr", LBF["n_corr"])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("cfg", CONFIGS, ids=CONFIG_IDS)
def test_lbfgs_lockstep(cfg, mode, n_corr, record):
    c, dtype, path = cfg
    b = ot.build(c)
    E, T = ot.make_engine(b, dtype, path), ot.make_engine(b, dtype, path)
    frozen = ot.frozen_entries(b)
    form = "compact" if mode == 1 else "vector"
    Lw = ot.Lbfgs(LBF["max_iter"], LBF["lr"], n_corr, np.longdouble, form)
    Ld = ot.Lbfgs(LBF["max_iter"], LBF["lr"], n_corr, np.float64, form)
    E.lbfgs_set_mode(mode)
    E.lbfgs_begin(LBF["max_iter"], LBF["lr"], n_corr, ot.EPS, ot.TOL_X)
    x = E.lbfgs_x()
    assert np.array_equal(x, b["w0"]) and np.array_equal(E.get_weights(), x)
    T.set_weights(x)
    f, g, _ = T.loss_grad()
    assert Lw.begin(f, g) == 0 and Ld.begin(f, g) == 0
    ratios = []
    for k in range(LBF["iters"]):
        tdw, tdd = Lw.step(), Ld.step()
        assert tdw is not None and tdd is not None
        iters, losses, done = E.lbfgs_run(1)
        x1 = E.lbfgs_x()
        assert np.array_equal(E.get_weights(), x1)               # (b)
        T.set_weights(x1)
        f, g, _ = T.loss_grad()
        assert Lw.evaluated(f, g) == 0 and Ld.evaluated(f, g) == 0
        assert done == 0 and iters.tolist() == [Lw.n_iter] == [k + 1], (k, iters, done)     # (d)
        assert losses[0] == f, (k, losses[0], f)                 # (a)
        yard, x_ref = ot.yardstick(x, tdw, tdd)                  # (c)
        dev = np.abs(x1.astype(np.longdouble) - x_ref)
        i = int(np.argmax(dev))
        ratio = float(dev[i]) / yard
        ratios.append(sig(ratio))
        assert ratio <= K_L, "iteration %d: x[%d] of %d is %.3g yardsticks (%.3e) from the restatement" % (
            k + 1, i, c.n, ratio, yard)
        for i in frozen:
            assert x1[i] == b["w0"][i]
        x = x1
    assert Lw.kept == Ld.kept and len(Lw.kept) == LBF["iters"] - 1
    record(n=c.n, dtype=dtype, path=E.kernel_path(), mode=mode, n_corr=n_corr, kept=sum(Lw.kept), lbfgs_ratios=ratios)
    assert E.status()[1] == 0
    E.close(); T.close()


def lbfgs_walk(eng, mode, n_corr, n_iters):
    """-> what n_iters single iterations show: (iteration list, loss list, done, x, weights) behind each"""
    eng.lbfgs_set_mode(mode)
    eng.lbfgs_begin(LBF["max_iter"], LBF["lr"], n_corr, ot.EPS, ot.TOL_X)
    out = []
    for _ in range(n_iters):
        it, ll, done = eng.lbfgs_run(1)
        out.append((it.tolist(), ll.tolist(), done, eng.lbfgs_x(), eng.get_weights()))
    return out


def same_walk(a, b):
    assert len(a) == len(b)
    for k, (p, q) in enumerate(zip(a, b)):
        assert p[0] == q[0] and p[1] == q[1] and p[2] == q[2], (k, p[:3], q[:3])
        assert np.array_equal(p[3], q[3]) and np.array_equal(p[4], q[4]), k


def adam_walk(eng, n_steps):
    eng.adam_init(A["lr"], A["b1"], A["b2"], A["eps"][0])
    out = []
    for _ in range(n_steps):
        out.append((eng.adam_run_terms(1)[0].tolist(), eng.get_weights()))
    return out


@pytest.mark.parametrize("n,dtype", COMM, ids=COMM_IDS)
def test_world1_communicator_changes_no_bit(n, dtype):
    import pinn_native
    b = ot.build(ot.by_n(n))
    solo, comm = ot.make_engine(b, dtype), ot.make_engine(b, dtype)
    if b["case"].pde == "adr_ide":
        with pytest.raises(pinn_native.PinnNativeError, match="single-device"):
            comm.comm_init(pinn_native.Engine.comm_unique_id(), 1, 0)
        solo.close(); comm.close()
        return
    comm.comm_init(pinn_native.Engine.comm_unique_id(), 1, 0)
    assert comm.comm_mode() == "rccl" and solo.comm_mode() == "none"
    for e in (solo, comm):
        e.adam_init(A["lr"], A["b1"], A["b2"], A["eps"][0])
    la, lb = solo.adam_run_terms(A["steps"]), comm.adam_run_terms(A["steps"])      # k_reduce_adam | k_reduce_rows + k_adam
    assert np.array_equal(la, lb) and np.array_equal(solo.get_weights(), comm.get_weights())
    assert np.any(solo.get_weights() != b["w0"])
    for mode in (0, 1):
        for e in (solo, comm):
            e.set_weights(b["w0"])
        same_walk(lbfgs_walk(solo, mode, 50, LBF["iters"]), lbfgs_walk(comm, mode, 50, LBF["iters"]))
    solo.close(); comm.close()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n,dtype", IDENT, ids=IDENT_IDS)
def test_used_context_is_a_fresh_one_at_every_step(n, dtype, mode):
    """lbfgs_begin_setup reallocates the rings only when n_corr grows, yet every layout stride depends on M1 = n_corr + 1:
    7, then 3 (smaller: the old allocation is kept), then 20 (larger: reallocated), then Adam"""
    b = ot.build(ot.by_n(n))
    used = ot.make_engine(b, dtype)
    for n_corr in (7, 3, 20):
        w = used.get_weights()
        fresh = ot.make_engine(b, dtype)
        fresh.set_weights(w)
        same_walk(lbfgs_walk(used, mode, n_corr, 5), lbfgs_walk(fresh, mode, n_corr, 5))
        fresh.close()
    w = used.get_weights()
    fresh = ot.make_engine(b, dtype)
    fresh.set_weights(w)
    for p, q in zip(adam_walk(used, 3), adam_walk(fresh, 3)):
        assert p[0] == q[0] and np.array_equal(p[1], q[1])
    assert used.status()[1] == 0
    used.close(); fresh.close()


@pytest.mark.parametrize("n,dtype", IDENT, ids=IDENT_IDS)
def test_snapshot_and_restore_round_three_adam_steps(n, dtype):
    b = ot.build(ot.by_n(n))
    eng = ot.make_engine(b, dtype)
    l0, g0, t0 = eng.loss_grad()
    eng.weights_snapshot(0)
    eng.adam_init(A["lr"], A["b1"], A["b2"], A["eps"][0])
    eng.adam_run(3)
    l3, g3, _ = eng.loss_grad()
    assert l3 != l0 and np.any(g3 != g0)
    eng.weights_restore(0)
    l1, g1, t1 = eng.loss_grad()
    assert l1 == l0 and np.array_equal(g1, g0) and np.array_equal(t1, t0)
    assert np.array_equal(eng.get_weights(), b["w0"])
    eng.close()
