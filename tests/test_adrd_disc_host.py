"""CPU: the numpy four-channel reference of the discrete-time adr family with a dispersion term
(tests/helpers/adrd_disc_oracle.py), which tests/test_gpu_adrd_disc.py holds the DISC_ADRD kernels of csrc/kernels_disc.h to.
Pinned against torch float64 autograd (three nested autograd.grad per column), against the three-channel sibling
(tests/helpers/adr_disc_ide_oracle.py) where d3 = 0, against nu -> 0, and against central differences in each raw
coefficient; then the mask, the exact soliton of 1d-kdv/kdvutil.py, the header and the binding."""
import os
import re
import sys

import numpy as np
import pytest

from conftest import PKG, ROOT

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import adr_disc_ide_oracle as adi  # noqa: E402
import adrd_disc_oracle as add  # noqa: E402

LB, UB = [-1.0], [1.0]
_COEFS = add.coefficient_vectors()


def rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300)


def _torch_loss_grad(theta, layers, sets, periodic):
    """the loss spelled with nested autograd.grad, backward to theta = [net | a0, a1, log nu, r1, r2, r3, d3]"""
    import torch
    torch.set_num_threads(4)
    th = torch.tensor(theta, dtype=torch.float64, requires_grad=True)
    n_net = add.n_net(layers)

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
        """every output column and its first three x derivatives, a column at a time"""
        x = torch.tensor(np.asarray(x, dtype=np.float64).reshape(-1, 1), requires_grad=True)
        U = net(x)
        Ux, Uxx, Uxxx = [], [], []
        for j in range(U.shape[1]):
            gx = torch.autograd.grad(U[:, j].sum(), x, create_graph=True)[0]
            gxx = torch.autograd.grad(gx.sum(), x, create_graph=True)[0]
            Ux.append(gx)
            Uxx.append(gxx)
            Uxxx.append(torch.autograd.grad(gxx.sum(), x, create_graph=True)[0])
        return U, torch.cat(Ux, dim=1), torch.cat(Uxx, dim=1), torch.cat(Uxxx, dim=1)

    a0, a1, lnu, r1, r2, r3, d3 = (th[n_net + k] for k in range(7))
    loss = 0.0
    for x, target, M in sets:
        U, Ux, Uxx, Uxxx = channels(x)
        pred = U
        if M is not None:
            q = M.shape[1]
            u, ux, uxx, uxxx = U[:, :q], Ux[:, :q], Uxx[:, :q], Uxxx[:, :q]
            N = (a0 + a1 * u) * ux - torch.exp(lnu) * uxx + d3 * uxxx + r1 * u + r2 * u ** 2 + r3 * u ** 3
            pred = U + N @ torch.tensor(M).T
        loss = loss + torch.sum((pred - torch.tensor(np.asarray(target).reshape(-1, 1))) ** 2)
    x_lb, x_ub, order = periodic
    Ul, Ulx, _, _ = channels(x_lb)
    Uu, Uux, _, _ = channels(x_ub)
    loss = loss + torch.sum((Ul - Uu) ** 2)
    if order:
        loss = loss + torch.sum((Ulx - Uux) ** 2)
    loss.backward()
    return float(loss.detach()), th.grad.numpy().copy()


# ---- 1. against autograd ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", [5, 6])
def test_oracle_against_torch_autograd(q):
    """[1, 9, 9, 6]: q = 5 leaves a column beyond q, q = 6 none; both sets with tables, 3 pairs at order 1, all seven
    coefficients non-zero.  The bounds tests/test_adr_disc_ide_host.py holds: 1e-14 in the loss, 1e-13 in the gradient (whole
    vector), 1e-12 on each tail entry against its own size"""
    layers = [1, 9, 9, 6]
    sets, (x_lb, x_ub), theta = add.case(layers, q, 17, 5, 3, seed=21 + q, coef=_COEFS[7])
    assert sets[0][2].shape == (6, q) and sets[1][2].shape == (6, q) and np.all(np.array(_COEFS[7]) != 0.0)
    per = (x_lb, x_ub, 1)
    lo, go, ex = add.loss_grad(theta, layers, LB, UB, sets, per)
    lt, gt = _torch_loss_grad(theta, layers, sets, per)
    tail = np.abs(go[-7:] - gt[-7:]) / np.abs(gt[-7:])
    print("q %d: loss %.2e grad %.2e tail %s" % (q, abs(lo - lt) / abs(lt), rel(go, gt), tail))
    assert all(t > 0.0 for t in ex["terms"])
    assert abs(lo - lt) / abs(lt) < 1e-14
    assert rel(go, gt) < 1e-13
    assert np.all(gt[-7:] != 0.0) and np.max(tail) < 1e-12


# ---- 2. the three-channel sibling embedded ------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(7))
def test_d3_zero_is_the_three_channel_sibling(k):
    """with d3 = 0 the loss, the net entries and the first six tail entries are adr_disc_ide_oracle's, to 1e-14"""
    layers, q = [1, 23, 23, 7], 5
    coef = adi.ado.coefficient_vectors()[k]
    sets, (x_lb, x_ub), th6 = adi.case(layers, q, 17, 3, 3, seed=10 + k, coef=coef)
    th7 = np.concatenate([th6, [0.0]])
    per = (x_lb, x_ub, 1)
    l6, g6, e6 = adi.loss_grad(th6, layers, LB, UB, sets, per)
    l7, g7, e7 = add.loss_grad(th7, layers, LB, UB, sets, per)
    assert abs(l7 - l6) <= 1e-14 * abs(l6)
    assert rel(g7[:-7], g6[:-6]) <= 1e-14
    assert np.all(np.abs(g7[-7:-1] - g6[-6:]) <= 1e-14 * np.abs(g6[-6:]))
    assert max(abs(e7["terms"][i] - e6["terms"][i]) for i in range(3)) <= 1e-14 * abs(l6)
    assert g7[-1] != 0.0                  # d L / d d3 is there at d3 = 0 too


# ---- 3. nu = 0 -------------------------------------------------------------------------------------------------------------------
def test_nu_off_is_the_operator_without_the_diffusion_term():
    """nu_on=False against the limit nu -> 0: at log nu = -800 exp underflows to exactly 0.0, so the two agree bit for bit
    but for the nu entry, which is exactly 0.0 with the flag and -0.0 * sum without; the slot's content is not read"""
    layers, q = [1, 23, 23, 7], 5
    sets, (x_lb, x_ub), theta = add.case(layers, q, 17, 3, 3, seed=31, coef=_COEFS[7])
    per = (x_lb, x_ub, 1)
    n = add.n_net(layers)
    lim = theta.copy()
    lim[n + 2] = -800.0
    assert np.exp(lim[n + 2]) == 0.0
    l0, g0, e0 = add.loss_grad(theta, layers, LB, UB, sets, per, nu_on=False)
    l1, g1, e1 = add.loss_grad(lim, layers, LB, UB, sets, per, nu_on=True)
    assert l0 == l1 and e0["terms"] == e1["terms"]
    keep = np.arange(theta.size) != n + 2
    assert np.array_equal(g0[keep], g1[keep])
    assert g0[n + 2] == 0.0 and not np.signbit(g0[n + 2])
    other = theta.copy()
    other[n + 2] = 3.0                    # the slot is not read
    l2, g2, _ = add.loss_grad(other, layers, LB, UB, sets, per, nu_on=False)
    assert l2 == l0 and np.array_equal(g2, g0)
    # and it differs from nu on
    assert add.loss_grad(theta, layers, LB, UB, sets, per)[0] != l0
    params = add.unpack(theta[:n], layers)
    (h, p, r, t), _ = add.forward4(params, sets[0][0], LB, UB)
    c = add.coef_of(theta, nu_on=False)
    assert c[2] == 0.0
    N = add.operator(c, h[:, :q], p[:, :q], r[:, :q], t[:, :q])
    assert np.array_equal(add.stage_prediction(theta, layers, sets[0][0], LB, UB, sets[0][2], nu_on=False), h + N @ sets[0][2].T)


# ---- 4. central differences in each raw coefficient ------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(8))
def test_tail_entries_against_central_differences(k):
    """the loss is quadratic in a0, a1, r1, r2, r3 and d3 (central differences are exact up to the rounding of two loss values:
    8 u max L / h, h = 2^-10, the check of tests/test_adr_disc_ide_host.py); in log nu it is not, so that entry takes h = 1e-5
    and 1e-8 of its own size"""
    layers, q = [1, 23, 23, 7], 5
    sets, (x_lb, x_ub), theta = add.case(layers, q, 17, 3, 3, seed=10 + k, coef=_COEFS[k])
    per = (x_lb, x_ub, 1)
    _, g, _ = add.loss_grad(theta, layers, LB, UB, sets, per)
    u = np.finfo(np.float64).eps / 2
    for e in range(7):
        h = 1e-5 if e == 2 else 2.0 ** -10
        tp, tm = theta.copy(), theta.copy()
        tp[-7 + e] += h
        tm[-7 + e] -= h
        Lp = add.loss_grad(tp, layers, LB, UB, sets, per)[0]
        Lm = add.loss_grad(tm, layers, LB, UB, sets, per)[0]
        fd = (Lp - Lm) / (2 * h)
        bound = 8 * u * max(Lp, Lm) / h + (1e-8 * abs(g[-7 + e]) if e == 2 else 0.0)
        assert abs(fd - g[-7 + e]) < bound, (add.NAMES[e], fd, g[-7 + e], bound)
        assert g[-7 + e] != 0.0


# ---- 5. the mask ----------------------------------------------------------------------------------------------------------------
def test_masked_entries_are_exactly_zero_and_the_others_unchanged():
    layers, q = [1, 23, 23, 7], 5
    sets, (x_lb, x_ub), theta = add.case(layers, q, 17, 3, 3, seed=3, coef=_COEFS[7])
    per = (x_lb, x_ub, 1)
    _, g_all, _ = add.loss_grad(theta, layers, LB, UB, sets, per)
    assert np.all(g_all[-7:] != 0.0)
    for mask in [0, 127, 64 + 13] + [1 << k for k in range(7)]:
        _, g, _ = add.loss_grad(theta, layers, LB, UB, sets, per, mask=mask)
        for k in range(7):
            assert g[-7 + k] == (g_all[-7 + k] if (mask >> k) & 1 else 0.0) and not (g[-7 + k] == 0.0 and np.signbit(g[-7 + k]))
        assert np.array_equal(g[:-7], g_all[:-7])
    assert add.mask_of(["a1", "d3"]) == 0b1000010


def test_float32_sweep_is_the_same_algebra():
    """the float32 sweep (what measures the helper's own float32 error for the GPU test) tracks float64 at float32 accuracy"""
    layers, q = [1, 23, 23, 7], 5
    sets, (x_lb, x_ub), theta = add.case(layers, q, 17, 3, 3, seed=3, coef=_COEFS[7])
    per = (x_lb, x_ub, 1)
    l64, g64, _ = add.loss_grad(theta, layers, LB, UB, sets, per)
    l32, g32, _ = add.loss_grad(theta, layers, LB, UB, sets, per, dtype=np.float32)
    assert 0.0 < abs(l32 - l64) / l64 < 1e-4 and 0.0 < rel(g32, g64) < 1e-3


# ---- 6. the soliton ------------------------------------------------------------------------------------------------------------
def test_soliton_satisfies_kdv():
    """u_t + a1 u u_x + d3 u_xxx = 0 by torch autograd at 50 random (x, t), to 1e-9 of max |u_t|; below 1e-4 at the walls
    between the default snapshots"""
    import torch
    sys.path.insert(0, os.path.join(PKG, "1d-kdv"))
    import kdvutil
    rs = np.random.RandomState(0)
    xn, tn = rs.uniform(-1, 1, 50), rs.uniform(0.2, 0.8, 50)
    x = torch.tensor(xn, dtype=torch.float64, requires_grad=True)
    t = torch.tensor(tn, dtype=torch.float64, requires_grad=True)
    a1, d3, c, x0 = kdvutil.A1, kdvutil.D3, kdvutil.C, kdvutil.X0
    u = (3.0 * c / a1) / torch.cosh(0.5 * np.sqrt(c / d3) * (x - c * t - x0)) ** 2
    assert np.allclose(u.detach().numpy(), kdvutil.soliton(xn, tn), rtol=1e-14, atol=0.0)
    u_t = torch.autograd.grad(u.sum(), t, create_graph=True)[0]
    u_x = torch.autograd.grad(u.sum(), x, create_graph=True)[0]
    u_xx = torch.autograd.grad(u_x.sum(), x, create_graph=True)[0]
    u_xxx = torch.autograd.grad(u_xx.sum(), x, create_graph=True)[0]
    f = (u_t + a1 * u * u_x + d3 * u_xxx).detach().numpy()
    scale = float(np.max(np.abs(u_t.detach().numpy())))
    assert scale > 0.1 and np.max(np.abs(f)) <= 1e-9 * scale, (np.max(np.abs(f)), scale)
    tt = np.linspace(0.2, 0.8, 61)
    assert max(np.max(kdvutil.soliton(-1.0, tt)), np.max(kdvutil.soliton(1.0, tt))) < 1e-4
    assert kdvutil.KDV_COEFFS == (0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0025)


# ---- 7. header and binding ---------------------------------------------------------------------------------------------------
def test_enum_binding_and_abi_version():
    import pinn_native
    text = open(os.path.join(ROOT, "include", "pinn_hip.h")).read()
    assert re.search(r"PINN_PDE_ADRD_DISC\s*=\s*9\b", text)
    assert pinn_native.pde_kind("adrd_disc") == 9 and pinn_native.DISC_PDE_KINDS["adrd_disc"] == 9
    assert pinn_native.DISC_PDE_KINDS["adr_disc"] == 7 and pinn_native.DISC_PDE_KINDS["adr_disc_ide"] == 8
    assert pinn_native.PDE_KINDS == {"burgers": 0, "burgers_ide": 1, "schrodinger": 2, "burgers_disc": 3,
                                     "burgers_disc_ide": 4, "adr": 5, "adr_ide": 6}
    assert pinn_native.ADR_COEFF_NAMES == ("a0", "a1", "nu", "r1", "r2", "r3")
    assert pinn_native.ADRD_COEFF_NAMES == ("a0", "a1", "nu", "r1", "r2", "r3", "d3")
    assert pinn_native.adr_trainable_mask(["a1", "d3"], pinn_native.ADRD_COEFF_NAMES) == 0b1000010
    with pytest.raises(ValueError, match="unknown adr coefficient"):
        pinn_native.adr_trainable_mask(["d3"])
    assert pinn_native.load().pinn_abi_version() == 6
    src = open(os.path.join(ROOT, "pinns-tf2.0_amd", "csrc", "kernels_disc.h")).read()
    assert re.search(r"DISC_ADRD = 3\b", src) and re.search(r"DISC_ADR_IDE = 2\b", src)


_HP = {"layers": [1, 20, 20, 8], "tf_epochs": 1, "tf_lr": 0.01, "tf_b1": 0.9, "tf_eps": None, "nt_epochs": 1,
       "nt_lr": 0.8, "nt_ncorr": 50, "log_frequency": 1}


@pytest.mark.parametrize("extra,match", [
    ({"adr_trainable": ["d3", "d4"]}, "adr_trainable"),
    ({"adr_init": [0.0, 1.0, 0.1, 0.0, 0.0, 0.0]}, "adr_init"),
    ({"adr_trainable": ["nu"], "adr_init": [0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.1]}, "nu must be positive to be trained"),
    ({"adr_init": [0.0, 1.0, -0.1, 0.0, 0.0, 0.0, 0.1]}, "adr_init"),
], ids=["unknown-name", "six-values", "nu-bit-with-nu-0", "negative-nu"])
def test_hp_options_of_the_script_kind_need_no_device(extra, match):
    import neuralnetwork as nn
    with pytest.raises(ValueError, match=match):
        nn.NeuralNetwork(dict(_HP, **extra), None, np.array(UB), np.array(LB), pde="adrd_disc")
    assert nn.ADRD_NAMES == nn.ADR_NAMES + ("d3",)
