"""CPU: the numpy reference of the discrete-time adr kind with trainable coefficients (tests/helpers/adr_disc_ide_oracle.py),
which tests/test_gpu_adr_disc_ide.py holds the DISC_ADR_IDE kernels of csrc/kernels_disc.h to.  Pinned against torch float64
autograd, against the Burgers identification oracle (oracle/disc.py) and the reference-made fixtures where the two models
coincide, and against central differences in each raw coefficient; then the mask, the header and the binding."""
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT, golden

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import adr_disc_oracle as ado  # noqa: E402
import adr_disc_ide_oracle as adi  # noqa: E402

LB, UB = [-1.0], [1.0]
_COEFS = ado.coefficient_vectors()


def rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300)


def _torch_loss_grad(theta, layers, sets, periodic):
    """the loss spelled with nested autograd.grad, backward to theta = [net | a0, a1, log nu, r1, r2, r3]"""
    import torch
    torch.set_num_threads(4)
    th = torch.tensor(theta, dtype=torch.float64, requires_grad=True)
    n_net = adi.n_net(layers)

    def net(x):
        h = 2.0 * (x - LB[0]) / (UB[0] - LB[0]) - 1.0
        off, n = 0, len(layers) - 1
        for i, (fi, fo) in enumerate(zip(layers[:-1], layers[1:])):
            W = th[off:off + fi * fo].reshape(fi, fo)
            off += fi * fo
            b = th[off:off + fo]
            off += fo
            h = h @ W + b
            if i < n - 1:
                h = torch.tanh(h)
        return h

    def channels(x):
        """every output column and its first two x derivatives, a column at a time"""
        x = torch.tensor(np.asarray(x, dtype=np.float64).reshape(-1, 1), requires_grad=True)
        U = net(x)
        Ux, Uxx = [], []
        for j in range(U.shape[1]):
            gx = torch.autograd.grad(U[:, j].sum(), x, create_graph=True)[0]
            Ux.append(gx)
            Uxx.append(torch.autograd.grad(gx.sum(), x, create_graph=True)[0])
        return U, torch.cat(Ux, dim=1), torch.cat(Uxx, dim=1)

    a0, a1, lnu, r1, r2, r3 = (th[n_net + k] for k in range(6))
    loss = 0.0
    for x, target, M in sets:
        U, Ux, Uxx = channels(x)
        pred = U
        if M is not None:
            q = M.shape[1]
            u, ux, uxx = U[:, :q], Ux[:, :q], Uxx[:, :q]
            N = (a0 + a1 * u) * ux - torch.exp(lnu) * uxx + r1 * u + r2 * u ** 2 + r3 * u ** 3
            pred = U + N @ torch.tensor(M).T
        loss = loss + torch.sum((pred - torch.tensor(np.asarray(target).reshape(-1, 1))) ** 2)
    x_lb, x_ub, order = periodic
    Ul, Ulx, _ = channels(x_lb)
    Uu, Uux, _ = channels(x_ub)
    loss = loss + torch.sum((Ul - Uu) ** 2)
    if order:
        loss = loss + torch.sum((Ulx - Uux) ** 2)
    loss.backward()
    return float(loss.detach()), th.grad.numpy().copy()


# ---- 1. against autograd ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", [5, 6])
def test_oracle_against_torch_autograd(q):
    """[1, 9, 9, 6]: q = 5 leaves a column beyond q, q = 6 none; both sets with tables, 3 pairs at order 1.  The agreement
    tests/test_adr_ide_host.py reaches: 1e-14 in the loss, 1e-13 in the gradient (whole vector), 1e-12 on each tail entry
    against its own size"""
    layers = [1, 9, 9, 6]
    sets, (x_lb, x_ub), theta = adi.case(layers, q, 17, 5, 3, seed=21 + q, coef=_COEFS[6])
    assert sets[0][2].shape == (6, q) and sets[1][2].shape == (6, q)
    per = (x_lb, x_ub, 1)
    lo, go, ex = adi.loss_grad(theta, layers, LB, UB, sets, per)
    lt, gt = _torch_loss_grad(theta, layers, sets, per)
    tail = np.abs(go[-6:] - gt[-6:]) / np.abs(gt[-6:])
    print("q %d: loss %.2e grad %.2e tail %s" % (q, abs(lo - lt) / abs(lt), rel(go, gt), tail))
    assert all(t > 0.0 for t in ex["terms"])
    assert abs(lo - lt) / abs(lt) < 1e-14
    assert rel(go, gt) < 1e-13
    assert np.all(gt[-6:] != 0.0) and np.max(tail) < 1e-12


# ---- 2. the reference's model embedded --------------------------------------------------------------------------------------
def _embed(w_ide):
    """[net | lambda_1, lambda_2] of the Burgers identification -> [net | 0, lambda_1, lambda_2, 0, 0, 0]"""
    return np.concatenate([w_ide[:-2], [0.0, w_ide[-2], w_ide[-1], 0.0, 0.0, 0.0]])


@pytest.mark.parametrize("tag", ["_small", ""])
def test_burgers_identification_is_the_kind_with_mask_a1_nu(tag):
    """against oracle.disc.disc_loss_grad(identify=True) and the reference-made fixture, at the tolerances
    tests/test_oracle_vs_golden.py applies to it"""
    from oracle import disc
    g = np.load(golden("burgers_disc_ide_eval%s.npz" % tag))
    q, layers = int(g["q"]), [int(v) for v in g["layers"]]
    W, _ = disc.irk_tables_like_reference(q)
    sets = disc.identification_sets(g["x_0"], g["u_0"], g["x_1"], g["u_1"], g["dt"], W[:-1], W[-1:])
    lo, go, _ = disc.disc_loss_grad(g["w0"], layers, LB, UB, sets, identify=True)
    loss, grad, ex = adi.loss_grad(_embed(g["w0"]), layers, LB, UB, sets, mask=adi.mask_of(["a1", "nu"]))
    assert abs(loss - lo) <= 1e-14 * abs(lo) and rel(grad[:-6], go[:-2]) < 1e-13
    assert abs(loss - float(g["loss"])) <= 1e-13 * abs(loss)
    assert rel(grad[:-6], g["grad"][:-2]) < 1e-12
    assert np.max(np.abs(grad[[-5, -4]] - g["grad"][-2:])) <= 1e-10 * np.max(np.abs(g["grad"][-2:]))
    assert np.max(np.abs(grad[[-5, -4]] - go[-2:])) <= 1e-13 * np.max(np.abs(go[-2:]))
    assert grad[-6] == 0.0 and np.all(grad[-3:] == 0.0)
    assert ex["terms"][2] == 0.0


# ---- 3. central differences in each raw coefficient ------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(7))
def test_tail_entries_against_central_differences(k):
    """the loss is quadratic in a0, a1, r1, r2, r3 (central differences are exact up to the rounding of two loss values:
    8 u max L / h, h = 2^-10, the check of tests/test_adr_ide_host.py); in log nu it is not, so that entry takes h = 1e-5 and
    1e-8 of its own size"""
    layers, q = [1, 23, 23, 7], 5
    sets, (x_lb, x_ub), theta = adi.case(layers, q, 17, 3, 3, seed=10 + k, coef=_COEFS[k])
    per = (x_lb, x_ub, 1)
    _, g, _ = adi.loss_grad(theta, layers, LB, UB, sets, per)
    u = np.finfo(np.float64).eps / 2
    for e in range(6):
        h = 1e-5 if e == 2 else 2.0 ** -10
        tp, tm = theta.copy(), theta.copy()
        tp[-6 + e] += h
        tm[-6 + e] -= h
        Lp = adi.loss_grad(tp, layers, LB, UB, sets, per)[0]
        Lm = adi.loss_grad(tm, layers, LB, UB, sets, per)[0]
        fd = (Lp - Lm) / (2 * h)
        bound = 8 * u * max(Lp, Lm) / h + (1e-8 * abs(g[-6 + e]) if e == 2 else 0.0)
        assert abs(fd - g[-6 + e]) < bound, (adi.NAMES[e], fd, g[-6 + e], bound)
        assert g[-6 + e] != 0.0


# ---- 4. the mask ----------------------------------------------------------------------------------------------------------------
def test_masked_entries_are_exactly_zero_and_the_others_unchanged():
    layers, q = [1, 23, 23, 7], 5
    sets, (x_lb, x_ub), theta = adi.case(layers, q, 17, 3, 3, seed=3, coef=_COEFS[6])
    per = (x_lb, x_ub, 1)
    _, g_all, _ = adi.loss_grad(theta, layers, LB, UB, sets, per)
    assert np.all(g_all[-6:] != 0.0)
    for mask in [0, 63, 13] + [1 << k for k in range(6)]:
        _, g, _ = adi.loss_grad(theta, layers, LB, UB, sets, per, mask=mask)
        for k in range(6):
            assert g[-6 + k] == (g_all[-6 + k] if (mask >> k) & 1 else 0.0)
        assert np.array_equal(g[:-6], g_all[:-6])
    assert adi.mask_of(["nu", "r1", "r3"]) == 0b101100


def test_pairs_and_sets_without_a_table_add_nothing_to_the_tail():
    layers, q = [1, 23, 23, 7], 5
    sets, (x_lb, x_ub), theta = adi.case(layers, q, 17, 3, 3, seed=4, coef=_COEFS[6])
    t_both, _ = adi.tail(theta, layers, LB, UB, sets)
    t0, _ = adi.tail(theta, layers, LB, UB, [sets[0], None])
    t1, _ = adi.tail(theta, layers, LB, UB, [None, sets[1]])
    assert np.allclose(t_both, t0 + t1, rtol=1e-14, atol=0.0)
    bare = [(sets[0][0], sets[0][1], None), None]
    assert np.all(adi.tail(theta, layers, LB, UB, bare)[0] == 0.0)
    g = adi.loss_grad(theta, layers, LB, UB, [None, None], (x_lb, x_ub, 1))[1]
    assert np.all(g[-6:] == 0.0) and np.any(g[:-6] != 0.0)


# ---- 5. header and binding ---------------------------------------------------------------------------------------------------
def test_enum_binding_and_abi_version():
    import pinn_native
    text = open(os.path.join(ROOT, "include", "pinn_hip.h")).read()
    assert re.search(r"PINN_PDE_ADR_DISC_IDE\s*=\s*8\b", text)
    assert pinn_native.pde_kind("adr_disc_ide") == 8 and pinn_native.DISC_PDE_KINDS["adr_disc_ide"] == 8
    assert pinn_native.PDE_KINDS == {"burgers": 0, "burgers_ide": 1, "schrodinger": 2, "burgers_disc": 3,
                                     "burgers_disc_ide": 4, "adr": 5, "adr_ide": 6}
    assert pinn_native.load().pinn_abi_version() == 6
    src = open(os.path.join(ROOT, "pinns-tf2.0_amd", "csrc", "kernels_disc.h")).read()
    assert re.search(r"DISC_ADR_IDE = 2\b", src)


def test_hp_options_of_the_script_kind_need_no_device(monkeypatch):
    import neuralnetwork as nn
    hp = {"layers": [1, 20, 20, 8], "tf_epochs": 1, "tf_lr": 0.01, "tf_b1": 0.9, "tf_eps": None, "nt_epochs": 1,
          "nt_lr": 0.8, "nt_ncorr": 50, "log_frequency": 1, "adr_trainable": ["nu", "r4"]}
    with pytest.raises(ValueError, match="adr_trainable"):
        nn.NeuralNetwork(hp, None, np.array(UB), np.array(LB), pde="adr_disc_ide")
