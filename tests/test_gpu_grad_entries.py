"""GPU: loss_grad() of every eligible kernel path against the restatement in the next wider type, ENTRY BY ENTRY: each
gradient entry on its own rounding scale A_i (tests/helpers/grad_entries.py), bound K[(family, dtype)] x max(plain error of
the same width, 32 u).  The cases are the smallest that reach each code path: one partial tile, one ragged tile per
workgroup, the tile loop's first launch (257 tiles), identification with lambda = (0.6, -4.5) and (0, -6), the Schrodinger
net with 1 and 17 boundary pairs and over two chunks, the shape-generic sweeps at widths 1, 24, 65, 97, 128 -- and, on the
same paths, nets whose hidden pre-activations reach into the tail of tanh (ge.SAT_CASES: first layer times 12, or every
weight times 2.5 ... 3; max |z| 5 ... 17, 1 ... 17 % beyond 3), each path judged by its own tanh formula.  The global
criterion max|g - ref| / max|ref| stays asserted at the tolerances of tests/test_gpu_fuzz.py, next to the loss and
run-to-run bit equality.  tests/test_grad_entries_host.py shows that the bounds used here reject a dropped point, a dropped
boundary pair and 1 % on a small entry or on the lambda_2 entry."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import grad_entries as ge  # noqa: E402

pytestmark = pytest.mark.gpu


def engine_for(case, dtype):
    import pinn_native
    w, s = ge.case_inputs(case["id"])
    eng = pinn_native.Engine(case["layers"], ge.LB, ge.UB, pde=case["kind"], dtype=dtype)
    if case["kind"] == "burgers":
        eng.set_collocation(s["X_f"]); eng.set_data(s["X_u"], s["u"]); eng.set_pde_params(s["nu"])
    elif case["kind"] == "burgers_ide":
        eng.set_data(s["X_u"], s["u"])
    else:
        eng.set_collocation(s["X_f"]); eng.set_data(s["X0"], s["uv0"]); eng.set_boundary(s["X_lb"], s["X_ub"])
    return eng, w


@pytest.mark.parametrize("cid,dtype", [(c["id"], d) for c in ge.CASES for d in ("f32", "f64") if d in c["paths"]])
def test_gradient_entries_on_every_path(cid, dtype, record):
    if dtype == "f64" and not ge.longdouble_is_wider():
        pytest.skip("np.longdouble is no wider than float64 on this host: no reference for the float64 kernels")
    case = ge.CASE_BY_ID[cid]
    ref_loss, ref, A = ge.reference(cid, dtype)
    plain = ge.plain_error(cid, dtype)
    layout = ge.blocks(case["layers"], case["kind"])
    tl, tg = (1e-11, 1e-10) if dtype == "f64" else (2e-5, 5e-5)
    eng, w = engine_for(case, dtype)
    assert eng.kernel_path() == case["paths"][dtype][0], (eng.kernel_path(), case["paths"][dtype])
    for path in case["paths"][dtype]:
        eng.set_kernel_path(path)                       # a path the case lists is eligible: a refusal is an error
        eng.set_weights(w)
        loss, grad, _ = eng.loss_grad()
        grad = np.array(grad, copy=True)
        dev, block, (row, col) = ge.entry_dev(grad, ref, A, layout)
        glob = np.max(np.abs(grad - ref)) / np.max(np.abs(ref))
        # a saturated case judges a path by its own tanh formula (ge.formula_of); the others have one yardstick
        yard, bound = ge.yardstick(cid, dtype, path), ge.bound(cid, dtype, path)
        ratio = dev / yard
        record(case=cid, dtype=dtype, path=path, entry_dev=dev, plain_error=plain, yardstick=yard, ratio=ratio, block=block,
               row=row, col=col, glob=glob)
        print("%s %s path %d: entry_dev %.3e at %s[%d,%d], plain %.3e, ratio %.2f, global %.3e"
              % (cid, dtype, path, dev, block, row, col, plain, ratio, glob))
        assert dev <= bound, "path %d: %s[%d,%d] is off by %.3e of its scale, bound %.3e (plain %s arithmetic: %.3e)" % (
            path, block, row, col, dev, bound, dtype, plain)
        assert abs(loss - ref_loss) <= tl * max(abs(ref_loss), 1e-3), (path, loss, ref_loss)
        assert glob <= tg, (path, glob)
        loss2, grad2, _ = eng.loss_grad()
        assert loss2 == loss and np.array_equal(grad, grad2), "path %d is not bit-reproducible" % path
    eng.close()
