"""CPU: the advection-diffusion-reaction kind with trainable coefficients (PINN_PDE_ADR_IDE, pde="adr_ide") without a device.

  * tests/helpers/adr_ide_ref.py, the numpy restatement the GPU tests use, pinned against torch autograd in float64 (all six
    coefficient entries and the net entries, at the bound tests/test_adr_host.py uses for adr_ref) and against the
    reference-made identification fixtures tests/golden/burgers_ide_eval*.npz (at the tolerances tests/test_oracle_vs_golden.py
    applies to them);
  * the restatement's own float32 / float64 rounding on the tail entries stays inside the entrywise bound the GPU test uses,
    and it meets the central-difference check of the GPU test;
  * hp parsing and the refusals of utils/neuralnetwork.py that need no device, the header and the symbol table."""
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT, golden

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import adr_ide_ref  # noqa: E402
import adr_ref  # noqa: E402
import grad_entries as ge  # noqa: E402

LB, UB = np.array([-1.0, 0.0]), np.array([1.0, 1.0])
NETS = {"8x20": [2] + [20] * 8 + [1], "3x33": [2, 33, 33, 33, 1]}


def rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300)


def _weights(layers, seed):
    from oracle import init
    w = init.glorot_flat(layers)
    return w + 0.05 * np.random.RandomState(seed).standard_normal(w.size)


def _sets(seed, n_f=300, n_u=60, n_b=40):
    rs = np.random.RandomState(seed)
    X_f = LB + (UB - LB) * rs.uniform(size=(n_f, 2))
    X_u = np.column_stack([rs.uniform(-1, 1, n_u), np.zeros(n_u)])
    u = (X_u[:, 0:1] ** 2) * np.cos(np.pi * X_u[:, 0:1])
    tb = rs.uniform(0, 1, n_b)
    return X_f, X_u, u, np.column_stack([np.full(n_b, -1.0), tb]), np.column_stack([np.full(n_b, 1.0), tb])


def _torch_loss_grad(theta, layers, X_f, X_u, u, X_lo, X_hi):
    """the loss spelled with nested autograd.grad, backward to theta = [net | a0, a1, log nu, r1, r2, r3]"""
    import torch
    torch.set_num_threads(4)
    th = torch.tensor(theta, dtype=torch.float64, requires_grad=True)
    lb, ub = torch.tensor(LB), torch.tensor(UB)
    n_net = adr_ide_ref.n_net(layers)

    def net(x, t):
        h = 2.0 * (torch.cat([x, t], dim=1) - lb) / (ub - lb) - 1.0
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

    def channels(X):
        x = torch.tensor(X[:, 0:1], requires_grad=True)
        t = torch.tensor(X[:, 1:2], requires_grad=True)
        uu = net(x, t)
        ones = torch.ones_like(uu)
        u_x, u_t = torch.autograd.grad(uu, [x, t], ones, create_graph=True)
        u_xx = torch.autograd.grad(u_x, x, ones, create_graph=True)[0]
        return uu, u_x, u_t, u_xx

    a0, a1, lnu, r1, r2, r3 = (th[n_net + k] for k in range(6))
    uu, u_x, u_t, u_xx = channels(X_f)
    f = u_t + (a0 + a1 * uu) * u_x - torch.exp(lnu) * u_xx + r1 * uu + r2 * uu ** 2 + r3 * uu ** 3
    loss = torch.mean(f ** 2) + torch.mean((channels(X_u)[0] - torch.tensor(u)) ** 2)
    ul, ul_x, _, _ = channels(X_lo)
    uh, uh_x, _, _ = channels(X_hi)
    loss = loss + torch.mean((ul - uh) ** 2) + torch.mean((ul_x - uh_x) ** 2)
    loss.backward()
    return float(loss.detach()), th.grad.numpy().copy()


# ---- 1. the restatement against autograd --------------------------------------------------------------------------------
@pytest.mark.parametrize("net", sorted(NETS))
@pytest.mark.parametrize("name", sorted(adr_ref.COEFF_SETS))
def test_restatement_against_torch_autograd(net, name):
    """the bound of tests/test_adr_host.py: 1e-14 in the loss, 1e-13 in the gradient (whole vector); the six tail entries
    also each against their own size"""
    layers, coeffs = NETS[net], adr_ref.COEFF_SETS[name]
    theta = adr_ide_ref.pack(_weights(layers, 5), coeffs)
    X_f, X_u, u, X_lo, X_hi = _sets(9)
    lo, go, ex = adr_ide_ref.loss_grad(theta, layers, LB, UB, X_f, X_u, u, X_lo, X_hi)
    lt, gt = _torch_loss_grad(theta, layers, X_f, X_u, u, X_lo, X_hi)
    tail = np.abs(go[-6:] - gt[-6:]) / np.abs(gt[-6:])
    print("adr_ide_ref vs autograd %s %s: loss %.2e grad %.2e tail %s" % (net, name, abs(lo - lt) / abs(lt), rel(go, gt), tail))
    assert ex["mse_b"] > 0 and ex["mse_u"] > 0 and ex["mse_f"] > 0
    assert abs(lo - lt) / abs(lt) < 1e-14
    assert rel(go, gt) < 1e-13
    assert np.all(gt[-6:] != 0.0) and np.max(tail) < 1e-12
    # the net entries are adr_ref's at the same coefficients, and the loss is
    la, ga, _ = adr_ref.adr_loss_grad(theta[:-6], layers, LB, UB, X_f, X_u, u, X_lo, X_hi, coeffs)
    assert abs(lo - la) / la < 1e-14 and rel(go[:-6], ga) < 1e-13


def test_masked_entries_are_exactly_zero_and_the_others_unchanged():
    layers = NETS["8x20"]
    theta = adr_ide_ref.pack(_weights(layers, 5), adr_ref.ALL_NONZERO)
    S = _sets(9)
    _, g_all, _ = adr_ide_ref.loss_grad(theta, layers, LB, UB, *S)
    for mask in (0, 1, 4, adr_ide_ref.mask_of(["nu", "r1", "r3"]), 63):
        _, g, _ = adr_ide_ref.loss_grad(theta, layers, LB, UB, *S, mask=mask)
        for k in range(6):
            assert g[-6 + k] == (g_all[-6 + k] if (mask >> k) & 1 else 0.0)
        assert np.array_equal(g[:-6], g_all[:-6])
    assert adr_ide_ref.mask_of(["nu", "r1", "r3"]) == 0b101100


# ---- 2. the reference-made identification fixtures -----------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["_small", ""])
def test_restatement_against_the_reference_made_identification_fixture(tag):
    """Burgers identification is the kind with collocation = data = X_u, mask {a1, nu}, tail [0, lambda_1, lambda_2, 0, 0, 0];
    tolerances of tests/test_oracle_vs_golden.py::test_burgers_identification"""
    g = np.load(golden("burgers_ide_eval%s.npz" % tag))
    X_u, u = g["X_u"], g["u"]
    lb, ub = np.array([-1.0, 0.0]), np.array([1.0, 0.99])
    layers = [2] + [20] * 8 + [1]
    w0 = g["w0"]
    theta = np.concatenate([w0[:-2], [0.0, w0[-2], w0[-1], 0.0, 0.0, 0.0]])
    loss, grad, ex = adr_ide_ref.loss_grad(theta, layers, lb, ub, X_u, X_u, u, None, None, mask=adr_ide_ref.mask_of(["a1", "nu"]))
    assert abs(loss - float(g["loss"])) < 1e-14
    assert rel(grad[:-6], g["grad"][:-2]) < 1e-12
    assert abs(grad[-5] - g["grad"][-2]) < 1e-15 and abs(grad[-4] - g["grad"][-1]) < 1e-15
    assert grad[-6] == 0.0 and np.all(grad[-3:] == 0.0)
    assert np.max(np.abs(ex["f"][:64, 0] - g["f_first"])) < 1e-13


# ---- the restatement against the bounds the GPU test uses ------------------------------------------------------------------
def _gpu_like_sets(N_f, n_0=512, n_b=50, seed=3):
    rs = np.random.RandomState(seed)
    X_f = LB + (UB - LB) * rs.uniform(size=(N_f, 2))
    x0 = rs.uniform(-1, 1, n_0)
    X_u = np.column_stack([x0, np.zeros(n_0)])
    u = (x0 * x0 * np.cos(np.pi * x0)).reshape(-1, 1)
    tb = rs.uniform(0, 1, n_b)
    return X_f, X_u, u, np.column_stack([np.full(n_b, -1.0), tb]), np.column_stack([np.full(n_b, 1.0), tb])


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_tail_entries_of_the_restatement_stay_inside_the_entrywise_bound(dtype):
    """plain arithmetic of the compute dtype against the wider one, each tail entry on its own scale A_k = sum |fb df/dp_k|:
    its error is what the bound K * max(plain_error, 32 u) is made of, so the restatement alone sits inside it"""
    if dtype == "f64" and not ge.longdouble_is_wider():
        pytest.skip("np.longdouble is no wider than float64 on this host")
    layers = NETS["8x20"]
    theta = adr_ide_ref.pack(_weights(layers, 7), adr_ref.ALL_NONZERO)
    S = _gpu_like_sets(2048)
    dt = ge.DTYPES[dtype]
    _, g, A, _ = adr_ide_ref.restate(theta, layers, LB, UB, *S, dtype=dt)
    _, gw, _, _ = adr_ide_ref.restate(theta, layers, LB, UB, *S, dtype=ge.wider(dt))
    dev = np.abs(g[-6:].astype(np.longdouble) - gw[-6:].astype(np.longdouble)) / A[-6:]
    u = ge.unit_roundoff(dt)
    bound = ge.K[("w20", dtype)] * max(float(np.max(dev)), ge.FLOOR_ULPS * u)
    print("tail plain error %s: %s u, bound %.1f u" % (dtype, np.asarray(dev / u, dtype=np.float64), bound / u))
    assert np.all(A[-6:] > 0) and float(np.max(dev)) < bound


def test_the_restatement_meets_the_central_difference_check():
    """the loss is exactly quadratic in the five raw coefficients, so (L(p + h e_k) - L(p - h e_k)) / 2h is gradient entry k
    up to the rounding of the two loss values: 8 u max L / h with h = 2^-10"""
    layers = NETS["8x20"]
    theta = adr_ide_ref.pack(_weights(layers, 7), adr_ref.ALL_NONZERO)
    S = _gpu_like_sets(2048)
    h = 2.0 ** -10
    _, g, _ = adr_ide_ref.loss_grad(theta, layers, LB, UB, *S)
    for k in (0, 1, 3, 4, 5):
        tp, tm = theta.copy(), theta.copy()
        tp[-6 + k] += h
        tm[-6 + k] -= h
        Lp = adr_ide_ref.loss_grad(tp, layers, LB, UB, *S)[0]
        Lm = adr_ide_ref.loss_grad(tm, layers, LB, UB, *S)[0]
        bound = 8 * ge.unit_roundoff(np.float64) * max(Lp, Lm) / h
        assert abs((Lp - Lm) / (2 * h) - g[-6 + k]) < bound, (k, (Lp - Lm) / (2 * h), g[-6 + k], bound)


# ---- 3. surface without a device ----------------------------------------------------------------------------------------------
def _hp(**kw):
    hp = {"layers": [2, 20, 20, 20, 20, 1], "tf_epochs": 1, "tf_lr": 0.01, "tf_b1": 0.9, "tf_eps": None,
          "nt_epochs": 1, "nt_lr": 0.8, "nt_ncorr": 50, "log_frequency": 1}
    hp.update(kw)
    return hp


def test_hp_parsing_and_refusals_need_no_device(monkeypatch):
    import neuralnetwork as nn
    names, init = nn._adr_ide_options(_hp(adr_trainable=["r3", "nu"], adr_init=[0, 0, 1e-3, -1, 0, 1]))
    assert names == ("nu", "r3") and init == (0.0, 0.0, 1e-3, -1.0, 0.0, 1.0)
    names, init = nn._adr_ide_options(_hp())
    assert names == () and init[:2] == (0.0, 1.0) and init[2] > 0
    with pytest.raises(ValueError, match="adr_trainable.*'r4'"):
        nn._adr_ide_options(_hp(adr_trainable=["nu", "r4"]))
    with pytest.raises(ValueError, match="adr_trainable"):
        nn._adr_ide_options(_hp(adr_trainable="nu"))
    for bad_nu in (0.0, -1e-4):
        with pytest.raises(ValueError, match="adr_init.*nu"):
            nn._adr_ide_options(_hp(adr_init=[0, 0, bad_nu, -5, 0, 5]))
    with pytest.raises(ValueError, match="adr_init"):
        nn._adr_ide_options(_hp(adr_init=[0, 0, 1e-4, -5, 0]))
    with pytest.raises(ValueError, match="adr_init"):
        nn._adr_ide_options(_hp(adr_init=[0, 0, 1e-4, np.nan, 0, 5]))
    # the option checks of "adr": RAD allowed, self-adaptive weights and a data-parallel world refused with the key named
    assert nn._resample_options(_hp(resample="rad", resample_every=10), "adr_ide")[0] == "rad"
    with pytest.raises(ValueError, match="sa_weights.*adr_ide"):
        nn._sa_options(_hp(sa_weights=True), "adr_ide")
    # a bad option is refused by the constructor before any engine is made
    with pytest.raises(ValueError, match="adr_trainable"):
        nn.NeuralNetwork(_hp(adr_trainable=["nu", "r4"]), None, UB, LB, pde="adr_ide")
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setenv("LOCAL_RANK", "0")
    with pytest.raises(ValueError, match='"adr_ide".*data-parallel'):
        nn.NeuralNetwork(_hp(), None, UB, LB, pde="adr_ide")


def test_names_to_mask():
    import pinn_native
    assert pinn_native.ADR_COEFF_NAMES == adr_ide_ref.NAMES
    assert pinn_native.adr_trainable_mask(["nu", "r1", "r3"]) == 0b101100
    assert pinn_native.adr_trainable_mask([]) == 0 and pinn_native.adr_trainable_mask(63) == 63
    assert pinn_native.adr_trainable_mask("a0") == 1
    with pytest.raises(ValueError, match="unknown adr coefficient 'r4'"):
        pinn_native.adr_trainable_mask(["r4"])


def test_enum_symbols_and_abi_version():
    import pinn_native
    text = open(os.path.join(ROOT, "include", "pinn_hip.h")).read()
    assert re.search(r"PINN_PDE_ADR_IDE\s*=\s*6\b", text)
    assert pinn_native.pde_kind("adr_ide") == 6 and pinn_native.pde_kind("adr") == 5
    with pytest.raises(ValueError, match="adr_ide"):
        pinn_native.pde_kind("allen-cahn")
    assert re.search(r"int pinn_set_pde_trainable\(pinn_ctx\* c, int mask\);", text)
    assert {"pinn_set_pde_trainable", "pinn_get_pde_params"} <= set(pinn_native.exported_symbols())
    lib = pinn_native.load()
    assert hasattr(lib, "pinn_set_pde_trainable") and hasattr(lib, "pinn_get_pde_params")
    assert lib.pinn_abi_version() == 6
    src = open(os.path.join(ROOT, "pinns-tf2.0_amd", "csrc", "kernels_generic.h")).read()
    assert re.search(r"constexpr int PDE_ADR_IDE = 4;", src)
