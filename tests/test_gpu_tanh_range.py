"""GPU: the tanh of every forward kernel over its whole range, read back exactly through a one-hidden-layer net whose output
is tanh(c x) (tests/helpers/tanh_probe.py): 4097 grid points, c = m 2^e from the subnormals to the overflow of -2|z|, widths
20 (k_fwd20d: tanh_d, k_fwd20f: tanh_r5), 7 (k_forward: the library), 24 and 65 (k_t16_fwd: tanh_mm), both types.  Every
value finite and at most 1 in magnitude, +-1 exactly past saturation, odd (tanh_r5: within twice the bound), within 4 x the
worst error of the same formula in numpy on the same grid; and the residual at the same points against its closed form
a c d1 + 2 nu a d1 c^2 within the tanh bound propagated through it, which pins 1 - a^2 at a one unit below 1.  The parity
tests elsewhere keep |z| below 1.3; tests/test_tanh_probe_host.py shows that these assertions reject a seamed exponential,
a clamp in the tail and a wrong d1."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import tanh_probe as tp  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("W", tp.WIDTHS)
def test_tanh_over_its_range_through_the_forward_kernel(W, dtype, record):
    if not tp.longdouble_is_wider():
        pytest.skip("np.longdouble is no wider than float64 on this host: no reference")
    import pinn_native
    form = tp.FORM[(W, dtype)]
    bound = tp.device_bound_u(form, dtype)
    X = tp.points()
    worst = {"worst_u": 0.0, "worst_z": 0.0}
    rel_small, res_ratio, failures = 0.0, 0.0, []
    eng = pinn_native.Engine([2, W, 1], tp.LB, tp.UB, pde="burgers", dtype=dtype)
    try:
        eng.set_pde_params(tp.NU)
        residual_scales = set(tp.residual_scales(dtype))
        for m, e in tp.scales(dtype):
            eng.set_weights(tp.weights(W, tp.scale_value(m, e), seed=W))
            a = eng.predict(X)
            assert a.shape == (X.shape[0], 1)
            try:
                out = tp.check_values(a, m, e, dtype, form, bound)
                if out["worst_u"] > worst["worst_u"]:
                    worst = out
                rel_small = max(rel_small, out["rel_small"])
            except AssertionError as err:                              # every scale is looked at before the test fails
                failures.append(str(err))
                w_u, w_z = tp.abs_error_u(a, m, e, dtype)
                if w_u > worst["worst_u"]:
                    worst = {"worst_u": w_u, "worst_z": w_z}
            if (m, e) in residual_scales:
                try:
                    res_ratio = max(res_ratio, tp.check_residual(eng.residual_at(X), m, e, dtype, bound))
                except AssertionError as err:
                    failures.append(str(err))
                    res_ratio = float("inf")
    finally:
        eng.close()
    record(kernel=tp.KERNEL[(W, dtype)], W=W, dtype=dtype, form=form, worst_u=worst["worst_u"], worst_z=worst["worst_z"],
           bound_u=bound, host_worst_u=tp.host_error(form, dtype)[0], rel_small=rel_small, residual_over_bound=res_ratio)
    print("%s %s (%s): worst %.3f u at z = %r, bound %.2f u (numpy: %.3f u); relative below 2^-10: %.3e; residual / bound %.3f"
          % (tp.KERNEL[(W, dtype)], dtype, form, worst["worst_u"], worst["worst_z"], bound, tp.host_error(form, dtype)[0],
             rel_small, res_ratio))
    assert not failures, "%d of the checks failed:\n%s" % (len(failures), "\n".join(failures))
