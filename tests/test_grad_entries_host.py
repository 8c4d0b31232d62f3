"""Host: the entrywise yardstick of tests/helpers/grad_entries.py checked on its own -- the restatement against the oracle,
|g_i| <= A_i, the plain-arithmetic floor, and THE CONDITION THAT KEEPS THE GPU TEST FROM HIDING A FAILURE: at every case,
dtype and kernel family of tests/test_gpu_grad_entries.py, each wrong gradient of grad_entries.mutants() (a dropped point,
1 % on a small entry, a dropped boundary pair, 1 % on the lambda_2 entry) lies above the bound K x max(plain error, 32 u)
that the GPU test asserts.  A K loosened past that cap fails here, without a GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import grad_entries as ge  # noqa: E402

CASE_IDS = [c["id"] for c in ge.CASES]
CASE_DTYPES = [(c["id"], d) for c in ge.CASES for d in ("f32", "f64") if d in c["paths"]]


def need_longdouble(dtype):
    if dtype == "f64" and not ge.longdouble_is_wider():
        pytest.skip("np.longdouble is no wider than float64 on this host: plain float64 has nothing to be judged against")


def oracle_of(case):
    from oracle import pde
    w, s = ge.case_inputs(case["id"])
    if case["kind"] == "burgers":
        return pde.burgers_loss_grad(w, case["layers"], ge.LB, ge.UB, s["X_f"], s["X_u"], s["u"], s["nu"])
    if case["kind"] == "burgers_ide":
        return pde.burgers_ide_loss_grad(w, case["layers"], ge.LB, ge.UB, s["X_u"], s["u"])
    return pde.schrodinger_loss_grad(w, case["layers"], ge.LB, ge.UB, s["X_f"], s["X_lb"], s["X_ub"], s["X0"], s["uv0"])


@pytest.mark.parametrize("cid", CASE_IDS)
def test_restatement_in_float64_is_the_oracle_and_A_dominates(cid):
    case = ge.CASE_BY_ID[cid]
    w, s = ge.case_inputs(cid)
    loss, grad, A = ge.restate(case["kind"], w, case["layers"], ge.LB, ge.UB, s, np.float64)
    lo, go, _ = oracle_of(case)
    assert grad.shape == go.shape == A.shape
    assert abs(loss - lo) <= 1e-13 * abs(lo)
    assert np.max(np.abs(grad - go)) <= 1e-13 * np.max(np.abs(go))
    assert np.all(np.abs(grad) <= A * (1 + 1e-12))                       # triangle inequality, entry by entry
    layout = ge.blocks(case["layers"], case["kind"])
    assert layout[-1][1].stop == grad.size and [b[0] for b in layout[:2]] == ["W0", "b0"]
    if case["kind"] == "burgers_ide":
        assert [b[0] for b in layout[-2:]] == ["lam1", "lam2"] and A[-1] > 0 and A[-2] >= 0


def test_restatement_takes_no_wider_type_on_the_way():
    """float32 in, float32 out (restate asserts that nothing was promoted); the tanh formula of the float32 kernels agrees
    with tanh to float32 rounding"""
    cid = "burgers_ide-8x20-f0-u700-lam0.6_-4.5"
    case = ge.CASE_BY_ID[cid]
    w, s = ge.case_inputs(cid)
    l32, g32, A = ge.restate(case["kind"], w, case["layers"], ge.LB, ge.UB, s, np.float32)
    assert g32.dtype == np.float32 and np.asarray(l32).dtype == np.float32 and A.dtype == np.float64
    _, gf, _ = ge.restate(case["kind"], w, case["layers"], ge.LB, ge.UB, s, np.float32, tanh_formula=True)
    _, ref, Ar = ge.reference(cid, "f32")
    layout = ge.blocks(case["layers"], case["kind"])
    assert 0 < ge.entry_dev(gf, ref, Ar, layout)[0] < 1e-4 and not np.array_equal(gf, g32)


def test_entry_dev_names_the_entry_and_insists_on_exact_zeros():
    layers = [2, 3, 1]
    layout = ge.blocks(layers, "burgers_ide")
    assert [b[0] for b in layout] == ["W0", "b0", "W1", "b1", "lam1", "lam2"]
    n = layout[-1][1].stop
    ref, A = np.arange(1.0, n + 1), np.full(n, 10.0)
    g = ref.copy()
    g[4] += 0.5                                                          # W0[1, 1]
    assert ge.entry_dev(g, ref, A, layout) == (0.05, "W0", (1, 1))
    g = ref.copy()
    g[-1] -= 2.0
    assert ge.entry_dev(g, ref, A, layout) == (0.2, "lam2", (0, 0))
    A0 = A.copy()
    A0[7] = 0.0                                                          # b0[0, 1]: no term at all -> must be equal
    assert ge.entry_dev(ref, ref, A0, layout)[0] == 0.0
    g = ref.copy()
    g[7] = np.nextafter(g[7], np.inf)
    assert ge.entry_dev(g, ref, A0, layout) == (np.inf, "b0", (0, 1))
    g = ref.copy()
    g[2] = np.nan
    assert ge.entry_dev(g, ref, A, layout)[0] == np.inf


@pytest.mark.parametrize("cid,dtype", CASE_DTYPES)
def test_plain_floor_and_every_mutant_is_above_the_bound(cid, dtype):
    need_longdouble(dtype)
    case = ge.CASE_BY_ID[cid]
    plain = ge.plain_error(cid, dtype)
    assert plain >= 0
    if dtype == "f32":
        assert plain <= 1e-4                                             # the yardstick itself is not rotten
    bound = ge.bound(cid, dtype)
    _, ref, A = ge.reference(cid, dtype)
    layout = ge.blocks(case["layers"], case["kind"])
    found = ge.mutants(cid, dtype)
    assert set(found) == {"a", "b"} | ({"c"} if case["kind"] == "schrodinger" else set()) | (
        {"d"} if case["kind"] == "burgers_ide" else set())
    for name, g in sorted(found.items()):
        dev, block, rc = ge.entry_dev(g, ref, A, layout)
        assert dev > bound, "mutant %s (worst at %s%s: %.3e of its scale) passes the bound %.3e = K %g x %.3e" % (
            name, block, rc, dev, bound, ge.K[(case["family"], dtype)], ge.yardstick(cid, dtype))


def test_the_global_criterion_misses_a_lost_point_that_the_entrywise_one_finds():
    """8x20, 700 collocation points, float32: the gradient without the last point is within 5e-5 of the largest entry
    (2.6e-5) -- the tolerance of the float32 parity tests -- and 30 x above the entrywise bound (5.1e-4 of its scale against
    1.7e-5).  (How far a lost point moves the global figure depends on the draw: 3e-5 ... 1.7e-3 over six 4x100 nets with
    700 points; the example is the case of the shared list where it stays below the tolerance.)"""
    cid = "burgers-8x20-f700-u61"
    case = ge.CASE_BY_ID[cid]
    _, ref, A = ge.reference(cid, "f32")
    g = ge.mutants(cid, "f32")["a"]
    assert np.max(np.abs(g - ref)) / np.max(np.abs(ref)) < 5e-5
    assert ge.entry_dev(g, ref, A, ge.blocks(case["layers"], case["kind"]))[0] > ge.bound(cid, "f32")
