"""CPU: the advection-diffusion-reaction residual kind (PINN_PDE_ADR, pde="adr") without a device.

  * tests/helpers/adr_ref.py, the hand-derived numpy oracle the GPU tests use, pinned twice: against torch autograd in
    float64 (nested autograd.grad for u_x, u_t, u_xx, backward to the flat weights) and, with Burgers coefficients, against
    oracle.pde.burgers_loss_grad and the reference-made fixture tests/golden/burgers_eval.npz;
  * the Fourier split-step solver of 1d-allen-cahn/allencahnutil.py: self-convergence in dt and in the number of modes;
  * prep_data shapes, hp validation and refusals that need no device, the enum value in the header and the Engine name table.
"""
import os
import re
import sys

import numpy as np
import pytest

from conftest import PKG, ROOT, golden

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
sys.path.insert(0, os.path.join(PKG, "1d-allen-cahn"))
import adr_ref  # noqa: E402

LB, UB = np.array([-1.0, 0.0]), np.array([1.0, 1.0])
NETS = {"8x20": [2] + [20] * 8 + [1], "4x20": [2] + [20] * 4 + [1], "3x33": [2, 33, 33, 33, 1]}


def rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300)


def _weights(layers, seed):
    from oracle import init
    return init.glorot_flat(layers) + 0.05 * np.random.RandomState(seed).standard_normal(
        sum(fi * fo + fo for fi, fo in zip(layers[:-1], layers[1:])))


def _sets(seed, n_f=300, n_u=60, n_b=40):
    rs = np.random.RandomState(seed)
    X_f = LB + (UB - LB) * rs.uniform(size=(n_f, 2))
    X_u = np.column_stack([rs.uniform(-1, 1, n_u), np.zeros(n_u)])
    u = (X_u[:, 0:1] ** 2) * np.cos(np.pi * X_u[:, 0:1])
    tb = rs.uniform(0, 1, n_b)
    return X_f, X_u, u, np.column_stack([np.full(n_b, -1.0), tb]), np.column_stack([np.full(n_b, 1.0), tb])


def _torch_loss_grad(w, layers, X_f, X_u, u, X_lo, X_hi, coeffs):
    import torch
    torch.set_num_threads(4)
    a0, a1, nu, r1, r2, r3 = coeffs
    wt = torch.tensor(w, dtype=torch.float64, requires_grad=True)
    lb, ub = torch.tensor(LB), torch.tensor(UB)

    def net(x, t):
        h = torch.cat([x, t], dim=1)
        h = 2.0 * (h - lb) / (ub - lb) - 1.0
        off = 0
        n = len(layers) - 1
        for i, (fi, fo) in enumerate(zip(layers[:-1], layers[1:])):
            W = wt[off:off + fi * fo].reshape(fi, fo)
            off += fi * fo
            b = wt[off:off + fo]
            off += fo
            h = h @ W + b
            if i < n - 1:
                h = torch.tanh(h)
        return h

    def channels(X):
        x = torch.tensor(X[:, 0:1], requires_grad=True)
        t = torch.tensor(X[:, 1:2], requires_grad=True)
        uu = net(x, t)
        ones = torch.ones_like(uu)
        u_x, u_t = torch.autograd.grad(uu, [x, t], ones, create_graph=True)
        u_xx = torch.autograd.grad(u_x, x, ones, create_graph=True)[0]
        return uu, u_x, u_t, u_xx

    uu, u_x, u_t, u_xx = channels(X_f)
    f = u_t + (a0 + a1 * uu) * u_x - nu * u_xx + r1 * uu + r2 * uu ** 2 + r3 * uu ** 3
    loss = torch.mean(f ** 2)
    loss = loss + torch.mean((channels(X_u)[0] - torch.tensor(u)) ** 2)
    ul, ul_x, _, _ = channels(X_lo)
    uh, uh_x, _, _ = channels(X_hi)
    loss = loss + torch.mean((ul - uh) ** 2) + torch.mean((ul_x - uh_x) ** 2)
    loss.backward()
    return float(loss.detach()), wt.grad.numpy().copy()


@pytest.mark.parametrize("net", sorted(NETS))
@pytest.mark.parametrize("name", sorted(adr_ref.COEFF_SETS))
def test_oracle_against_torch_autograd(net, name):
    """measured when this was written: 3.5e-16 in the loss, 2.2e-15 in the gradient; asserted at 1e-14 / 1e-13"""
    layers, coeffs = NETS[net], adr_ref.COEFF_SETS[name]
    w = _weights(layers, 5)
    X_f, X_u, u, X_lo, X_hi = _sets(9)
    lo, go, ex = adr_ref.adr_loss_grad(w, layers, LB, UB, X_f, X_u, u, X_lo, X_hi, coeffs)
    lt, gt = _torch_loss_grad(w, layers, X_f, X_u, u, X_lo, X_hi, coeffs)
    print("adr_ref vs autograd %s %s: loss %.2e grad %.2e" % (net, name, abs(lo - lt) / abs(lt), rel(go, gt)))
    assert ex["mse_b"] > 0 and ex["mse_u"] > 0 and ex["mse_f"] > 0
    assert abs(lo - lt) / abs(lt) < 1e-14
    assert rel(go, gt) < 1e-13


def test_oracle_with_burgers_coefficients_against_the_burgers_oracle_and_the_golden(burgers_sets):
    from oracle import pde
    g = np.load(golden("burgers_eval.npz"))
    nu = float(g["nu"])
    r = burgers_sets(100, 10000)
    X_u, u, X_f, ub, lb = r[7], r[8], r[9], r[10], r[11]
    layers = [2] + [20] * 8 + [1]
    co = adr_ref.BURGERS(nu)
    l, gr, ex = adr_ref.adr_loss_grad(g["w0"], layers, lb, ub, X_f, X_u, u, None, None, co)
    assert abs(l - float(g["loss"])) / float(g["loss"]) < 1e-14
    assert rel(gr, g["grad"]) < 1e-13
    w1 = g["w0"] + 0.05 * np.random.RandomState(7).standard_normal(g["w0"].size)
    l, gr, ex = adr_ref.adr_loss_grad(w1, layers, lb, ub, X_f, X_u, u, None, None, co)
    lo, go, eo = pde.burgers_loss_grad(w1, layers, lb, ub, X_f, X_u, u, nu)
    assert abs(l - lo) / lo < 1e-14
    assert rel(gr, go) < 1e-13
    assert rel(ex["f"], eo["f"]) < 1e-13
    assert rel(adr_ref.residual(w1, layers, lb, ub, X_f, co), eo["f"]) < 1e-13


# ---- the split-step solver ------------------------------------------------------------------------------------------
def test_split_step_converges_second_order_in_dt():
    import allencahnutil as ac
    fields = [ac.solve_allen_cahn(512, 201, s)[2] for s in (25, 50, 100)]
    d1, d2 = np.abs(fields[0] - fields[1]).max(), np.abs(fields[1] - fields[2]).max()
    print("dt halving: %.3e -> %.3e (ratio %.3f)" % (d1, d2, d1 / d2))
    assert 3.0 < d1 / d2 < 5.0
    assert d2 < 1e-7


def test_split_step_converges_in_space_and_keeps_the_initial_condition():
    import allencahnutil as ac
    x2, t2, U2 = ac.solve_allen_cahn(2048, 201, 50)
    x4, t4, U4 = ac.solve_allen_cahn(4096, 201, 50)
    d = np.abs(U2 - U4[:, ::2]).max()
    print("2048 vs 4096 modes: %.3e" % d)
    assert d < 2e-4
    assert np.array_equal(U4[0], ac.initial_condition(x4))
    assert np.all(np.abs(U4) <= 1.0 + 1e-12)          # u = +-1 are the reaction's stable states: the field stays inside
    assert x4[0] == -1.0 and x4[-1] < 1.0 and t4[0] == 0.0 and t4[-1] == 1.0


def test_exact_field_is_cached_and_subsampled(tmp_path):
    import allencahnutil as ac
    x, t, E = ac.exact_field(str(tmp_path), n_x=64, n_t=11, n_modes=256, substeps=10)
    assert x.shape == (64, 1) and t.shape == (11, 1) and E.shape == (11, 64)
    assert os.path.exists(os.path.join(str(tmp_path), "allen_cahn_exact.npz"))
    x2, t2, E2 = ac.exact_field(str(tmp_path), n_x=64, n_t=11, n_modes=256, substeps=10)
    assert np.array_equal(E, E2) and np.array_equal(x, x2)
    assert np.array_equal(E, ac.solve_allen_cahn(256, 11, 10)[2][:, ::4])
    x3, _, E3 = ac.exact_field(str(tmp_path), n_x=32, n_t=11, n_modes=256, substeps=10)     # another key: recomputed
    assert E3.shape == (11, 32)
    with pytest.raises(ValueError):
        ac.exact_field(None, n_x=48, n_t=11, n_modes=256, substeps=10)


def test_prep_data_shapes():
    import allencahnutil as ac
    field = ac.exact_field(None, n_x=64, n_t=11, n_modes=256, substeps=10)
    np.random.seed(1234)
    (x, t, X, T, Exact_u, X_star, u_star, X_u, u, X_f, X_lb, X_ub, ub, lb) = ac.prep_data(32, 20, 500, field=field)
    assert X_star.shape == (64 * 11, 2) and u_star.shape == (64 * 11, 1)
    assert X_u.shape == (32, 2) and u.shape == (32, 1) and np.all(X_u[:, 1] == 0.0)
    assert np.allclose(u[:, 0], ac.initial_condition(X_u[:, 0]), atol=0, rtol=0)
    assert X_f.shape == (500, 2) and np.all(X_f >= lb) and np.all(X_f <= ub)
    assert X_lb.shape == X_ub.shape == (20, 2)
    assert np.all(X_lb[:, 0] == -1.0) and np.all(X_ub[:, 0] == 1.0) and np.array_equal(X_lb[:, 1], X_ub[:, 1])
    assert list(lb) == [-1.0, 0.0] and list(ub) == [1.0, 1.0]
    assert ac.ADR_COEFFS == (0.0, 0.0, 1e-4, -5.0, 0.0, 5.0)


# ---- surface without a device -----------------------------------------------------------------------------------------
def test_enum_value_in_the_header_and_the_engine_name_table():
    import pinn_native
    text = open(os.path.join(ROOT, "include", "pinn_hip.h")).read()
    assert re.search(r"PINN_PDE_ADR\s*=\s*5\b", text)
    assert pinn_native.PDE_KINDS["adr"] == 5
    assert pinn_native.PDE_KINDS == {"burgers": 0, "burgers_ide": 1, "schrodinger": 2, "burgers_disc": 3, "burgers_disc_ide": 4,
                                     "adr": 5, "adr_ide": 6}
    assert "the ABI version stays 6" in text[text.index("advection-diffusion-reaction"):text.index("PINN_PDE_ADR = 5")]


def _hp(**kw):
    hp = {"layers": [2, 20, 20, 20, 20, 1], "tf_epochs": 1, "tf_lr": 0.01, "tf_b1": 0.9, "tf_eps": None,
          "nt_epochs": 1, "nt_lr": 0.8, "nt_ncorr": 50, "log_frequency": 1}
    hp.update(kw)
    return hp


def test_hp_validation_for_the_adr_kind_needs_no_device(monkeypatch):
    import neuralnetwork as nn
    # residual-adaptive redraws are accepted for "adr" (it has a collocation set) ...
    assert nn._resample_options(_hp(resample="rad", resample_every=10), "adr")[0] == "rad"
    with pytest.raises(ValueError, match="resample_every"):
        nn._resample_options(_hp(resample="rad"), "adr")
    # ... self-adaptive weights stay Burgers-only, refused by name
    with pytest.raises(ValueError, match="sa_weights.*adr"):
        nn._sa_options(_hp(sa_weights=True), "adr")
    # a data-parallel launch is refused by name before any engine is made
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setenv("LOCAL_RANK", "0")
    with pytest.raises(ValueError, match='"adr".*data-parallel'):
        nn.NeuralNetwork(_hp(), None, UB, LB, pde="adr")


def test_unknown_pde_name_is_refused_with_the_table():
    import pinn_native
    with pytest.raises(ValueError, match="adr"):
        pinn_native.Engine([2, 20, 1], LB, UB, pde="allen-cahn")
