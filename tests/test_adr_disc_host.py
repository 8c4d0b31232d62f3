"""CPU: the numpy reference of the discrete-time adr kind (tests/helpers/adr_disc_oracle.py), which the GPU tests of
tests/test_gpu_adr_disc.py hold the kernels of csrc/kernels_disc.h to.  Pinned three ways: against the existing Burgers
oracle (oracle/disc.py) where the two coincide, against central differences of its own loss with one coefficient switched
on at a time, and against the exact heat mode for the sign and table conventions."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import adr_disc_oracle as ado  # noqa: E402

LAYERS, Q, N0, N1 = [1, 23, 23, 7], 5, 17, 3
LB, UB = [-1.0], [1.0]


def test_burgers_coefficients_without_pairs_agree_with_the_existing_oracle():
    """loss and gradient equal oracle.disc.disc_loss_grad to 1e-14 relative"""
    from oracle import disc
    sets, _, w = ado.case(LAYERS, Q, N0, N1, 0, seed=3)
    lo, go, ex = disc.disc_loss_grad(w, LAYERS, LB, UB, sets, nu=ado.BURGERS[2])
    l, g, e = ado.loss_grad(w, LAYERS, LB, UB, sets, ado.BURGERS)
    d_loss, d_grad = abs(l - lo) / abs(lo), np.max(np.abs(g - go)) / np.max(np.abs(go))
    print("loss %.3e grad %.3e" % (d_loss, d_grad))
    assert d_loss <= 1e-14 and d_grad <= 1e-14
    assert abs(e["terms"][0] - ex["sse"][0]) <= 1e-14 * lo and abs(e["terms"][1] - ex["sse"][1]) <= 1e-14 * lo
    assert e["terms"][2] == 0.0
    # the stage prediction too
    xs = np.linspace(-1.0, 1.0, 9)[:, None]
    from oracle import mlp
    params = mlp.unpack(w, LAYERS)
    ref = disc.stage_prediction(params, xs, np.array(LB), np.array(UB), sets[0][2], 1.0, ado.BURGERS[2])[0]
    assert np.max(np.abs(ado.stage_prediction(params, xs, LB, UB, sets[0][2], ado.BURGERS) - ref)) <= 1e-14 * np.max(np.abs(ref))


_COEFS = ado.coefficient_vectors()


def test_coefficient_vectors_switch_on_one_term_each():
    assert len(_COEFS) == 7
    for k, c in enumerate(_COEFS[:6]):
        on = {i for i in range(6) if c[i] != 0.0}
        assert on == {k, 2} and c[k] == 1.0 and (k == 2 or c[2] == 0.1)
    assert all(-1.0 <= v <= 1.0 and v != 0.0 for v in _COEFS[6]) and _COEFS[6][2] > 0.0


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("k", range(7))
def test_gradient_against_central_differences(k, order):
    """20 randomly chosen entries, h = 1e-6, to 1e-6 of the largest gradient entry; 3 periodic pairs"""
    coef = _COEFS[k]
    sets, (x_lb, x_ub), w = ado.case(LAYERS, Q, N0, N1, 3, seed=10 + k)
    per = (x_lb, x_ub, order)
    loss, g, e = ado.loss_grad(w, LAYERS, LB, UB, sets, coef, per)
    assert all(t > 0.0 for t in e["terms"]) and abs(sum(e["terms"]) - loss) <= 1e-15 * loss
    rs = np.random.RandomState(100 + k)
    idx = rs.choice(w.size, 20, replace=False)
    h = 1e-6
    worst = 0.0
    for i in idx:
        wp, wm = w.copy(), w.copy()
        wp[i] += h
        wm[i] -= h
        fd = (ado.loss_grad(wp, LAYERS, LB, UB, sets, coef, per)[0] - ado.loss_grad(wm, LAYERS, LB, UB, sets, coef, per)[0]) / (2 * h)
        worst = max(worst, abs(fd - g[i]))
    print("coef %d order %d: worst %.3e of %.3e" % (k, order, worst, np.max(np.abs(g))))
    assert worst <= 1e-6 * np.max(np.abs(g))


def test_order_changes_the_periodic_term_only():
    sets, (x_lb, x_ub), w = ado.case(LAYERS, Q, N0, N1, 3, seed=4)
    t0 = ado.loss_grad(w, LAYERS, LB, UB, sets, _COEFS[6], (x_lb, x_ub, 0))[2]["terms"]
    t1 = ado.loss_grad(w, LAYERS, LB, UB, sets, _COEFS[6], (x_lb, x_ub, 1))[2]["terms"]
    assert t0[:2] == t1[:2] and t1[2] > t0[2] > 0.0


def _heat_defects(q, dt, nu=0.1, t0=0.1):
    """U + N(U) M^T - u(t0) for the exact heat mode u = exp(-nu pi^2 t) sin(pi x) at the Gauss stage times, M = dt [A; b]
    -> (largest stage defect, largest final-row defect)"""
    from oracle import disc
    A, b, c = disc.gauss_legendre_butcher(q)
    M = dt * np.vstack([A, b[None, :]])                           # [q + 1, q]
    x = np.linspace(-1.0, 1.0, 41)[:, None]
    times = np.concatenate([t0 + c * dt, [t0 + dt]])[None, :]     # the q stages, then t1
    amp = np.exp(-nu * np.pi ** 2 * times)
    U, U_x, U_xx = amp * np.sin(np.pi * x), np.pi * amp * np.cos(np.pi * x), -np.pi ** 2 * amp * np.sin(np.pi * x)
    N = ado.operator((0.0, 0.0, nu, 0.0, 0.0, 0.0), U[:, :q], U_x[:, :q], U_xx[:, :q])
    defect = U + N @ M.T - np.exp(-nu * np.pi ** 2 * t0) * np.sin(np.pi * x)
    return np.max(np.abs(defect[:, :q])), np.max(np.abs(defect[:, q]))


def test_sign_and_table_convention_on_the_exact_heat_mode():
    """q = 3: the stage defect is of order q + 1 = 4 in dt and the final row's of order 2 q + 1 = 7 (Gauss collocation), so
    halving dt divides them by 16 and 128; asserted with one power of two to spare.  A wrong sign of N, a transposed table
    or b in the wrong row leaves defects of order dt."""
    s1, f1 = _heat_defects(3, 0.5)
    s2, f2 = _heat_defects(3, 0.25)
    print("stage ratio %.1f final ratio %.1f final defect at dt 0.5 %.2e" % (s1 / s2, f1 / f2, f1))
    assert s1 / s2 >= 8.0 and f1 / f2 >= 64.0
    assert f1 <= 1e-8
