"""CPU: the numpy restatement of the adr2 kind (tests/helpers/adr2_ref.py), which tests/test_gpu_adr2.py holds the PDE_ADR2
kernels of csrc/kernels_generic.h to.  Pinned against torch float64 autograd (nested autograd.grad for u_xx and u_tt) and,
where kappa = 0, b = 1, gamma = 0, against tests/helpers/adr_src_ref.py with `==`; then the exact fields of 1d-wave/ and
2d-helmholtz/, the header, the binding and the hp refusals."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from conftest import PKG, ROOT

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import adr2_ref  # noqa: E402
import adr_src_ref  # noqa: E402


def rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300)


def case(lb, ub, seed, layers=(2, 9, 9, 1)):
    """33 collocation points with a source, 17 data points, 3 pairs, 5 wall points with all three terms"""
    from oracle import init
    rs = np.random.RandomState(seed)
    lb, ub = np.asarray(lb, dtype=np.float64), np.asarray(ub, dtype=np.float64)
    layers = list(layers)
    w = init.glorot_flat(layers) + 0.1 * rs.standard_normal(adr_src_ref.mlp.n_params(layers))
    pts = lambda n: lb + (ub - lb) * rs.uniform(size=(n, 2))    # noqa: E731
    X_f, X_u, X_w = pts(33), pts(17), pts(5)
    u = rs.uniform(-1, 1, (17, 1))
    tb = lb[1] + (ub[1] - lb[1]) * rs.uniform(size=3)
    X_lo, X_hi = np.column_stack([np.full(3, lb[0]), tb]), np.column_stack([np.full(3, ub[0]), tb])
    s = rs.uniform(-1, 1, 33)
    alpha, beta, gamma, g = (rs.uniform(0.3, 1.5, 5) * np.where(rs.uniform(size=5) < 0.5, -1.0, 1.0) for _ in range(4))
    return dict(w=w, layers=layers, lb=lb, ub=ub, X_f=X_f, X_u=X_u, u=u, X_lo=X_lo, X_hi=X_hi, s=s, X_w=X_w, alpha=alpha,
                beta=beta, gamma=gamma, g=g)


def helper(c, coeffs, **kw):
    return adr2_ref.adr2_loss_grad(c["w"], c["layers"], c["lb"], c["ub"], c["X_f"], c["X_u"], c["u"], c["X_lo"], c["X_hi"],
                                   coeffs, c["s"], c["X_w"], c["alpha"], c["beta"], c["gamma"], c["g"], **kw)


def _torch_loss_grad(c, coeffs):
    import torch
    torch.set_num_threads(4)
    th = torch.tensor(c["w"], dtype=torch.float64, requires_grad=True)
    lb, ub = torch.tensor(c["lb"]), torch.tensor(c["ub"])
    layers = c["layers"]
    a0, a1, nu, r1, r2, r3, b, kappa = coeffs

    def net(x, t):
        h = 2.0 * (torch.stack([x, t], dim=1) - lb) / (ub - lb) - 1.0
        off, n = 0, len(layers) - 1
        for i, (fi, fo) in enumerate(zip(layers[:-1], layers[1:])):
            W = th[off:off + fi * fo].reshape(fi, fo)
            off += fi * fo
            bb = th[off:off + fo]
            off += fo
            h = h @ W + bb
            if i < n - 1:
                h = torch.tanh(h)
        return h[:, 0]

    def channels(X):
        x = torch.tensor(X[:, 0], requires_grad=True)
        t = torch.tensor(X[:, 1], requires_grad=True)
        u = net(x, t)
        u_x, u_t = torch.autograd.grad(u.sum(), (x, t), create_graph=True)
        u_xx = torch.autograd.grad(u_x.sum(), x, create_graph=True)[0]
        u_tt = torch.autograd.grad(u_t.sum(), t, create_graph=True)[0]
        return u, u_x, u_t, u_xx, u_tt

    u, u_x, u_t, u_xx, u_tt = channels(c["X_f"])
    f = b * u_t + (a0 + a1 * u) * u_x - nu * (u_xx + kappa * u_tt) + r1 * u + r2 * u ** 2 + r3 * u ** 3 - torch.tensor(c["s"])
    loss = torch.mean(f ** 2)
    loss = loss + torch.mean((channels(c["X_u"])[0] - torch.tensor(c["u"][:, 0])) ** 2)
    lo, hi = channels(c["X_lo"]), channels(c["X_hi"])
    loss = loss + torch.mean((lo[0] - hi[0]) ** 2 + (lo[1] - hi[1]) ** 2)
    uw = channels(c["X_w"])
    r = torch.tensor(c["alpha"]) * uw[0] + torch.tensor(c["beta"]) * uw[1] + torch.tensor(c["gamma"]) * uw[2] - torch.tensor(c["g"])
    loss = loss + torch.mean(r ** 2)
    loss.backward()
    return float(loss.detach()), th.grad.numpy().copy(), f.detach().numpy(), r.detach().numpy()


# ---- 1. against autograd ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lb,ub", [([-1.0, 0.0], [1.0, 2.0]), ([0.5, -2.0], [3.0, -1.0])], ids=["box-a", "box-b"])
def test_helper_against_torch_autograd(lb, ub):
    """[2, 9, 9, 1], two boxes (sx != st in the second), all eight coefficients non-zero.  The bounds of
    tests/test_adrd_disc_host.py: 1e-14 in the loss, 1e-13 in the gradient, relative"""
    c = case(lb, ub, seed=5)
    coeffs = adr2_ref.COEFF_SETS["all"]
    assert np.all(np.array(coeffs) != 0.0)
    if lb[0] == 0.5:                    # the second box: the two input scales differ
        assert 2.0 / (c["ub"][0] - c["lb"][0]) != 2.0 / (c["ub"][1] - c["lb"][1])
    lo, go, ex = helper(c, coeffs)
    lt, gt, ft, rt = _torch_loss_grad(c, coeffs)
    print("loss %.2e grad %.2e f %.2e r %.2e" % (abs(lo - lt) / lt, rel(go, gt), rel(ex["f"].ravel(), ft), rel(ex["r"], rt)))
    assert min(ex["mse_f"], ex["mse_u"], ex["mse_b"], ex["mse_w"]) > 0.0
    assert abs(lo - lt) / abs(lt) < 1e-14
    assert rel(go, gt) < 1e-13
    assert rel(ex["f"].ravel(), ft) < 1e-13 and rel(ex["r"], rt) < 1e-13
    f_at = adr2_ref.residual(c["w"], c["layers"], c["lb"], c["ub"], c["X_f"], coeffs, c["s"])
    r_at = adr2_ref.wall_residual(c["w"], c["layers"], c["lb"], c["ub"], c["X_w"], c["alpha"], c["beta"], c["gamma"], c["g"], coeffs)
    assert np.array_equal(f_at, ex["f"]) and np.array_equal(r_at, ex["r"])


def test_kappa_term_matters_in_every_part():
    """kappa moves the residual part, the wall part's gradient and nothing else of the loss: a helper that dropped a kappa term
    would not pass the autograd test by luck"""
    c = case([-1.0, 0.0], [1.0, 2.0], seed=5)
    co = list(adr2_ref.COEFF_SETS["all"])
    l1, g1, e1 = helper(c, co)
    co[7] = 0.0
    l0, g0, e0 = helper(c, co)
    assert abs(e1["mse_f"] - e0["mse_f"]) > 1e-5 * e0["mse_f"] and rel(g1, g0) > 1e-5     # (nine orders above rounding)
    assert e1["mse_u"] == e0["mse_u"] and e1["mse_b"] == e0["mse_b"] and e1["mse_w"] == e0["mse_w"]


# ---- 2. the adr kind embedded -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_source", [True, False])
def test_degenerate_vector_is_adr_src_ref(with_source):
    """kappa = 0, b = 1, gamma = 0: adr_src_ref's loss, gradient, residuals and terms, with =="""
    c = case([-1.0, 0.0], [1.0, 2.0], seed=9)
    co = adr2_ref.COEFF_SETS["adr"]
    assert co[6] == 1.0 and co[7] == 0.0
    c = dict(c, gamma=np.zeros(5), s=c["s"] if with_source else None)
    l2, g2, e2 = helper(c, co)
    l1, g1, e1 = adr_src_ref.src_loss_grad(c["w"], c["layers"], c["lb"], c["ub"], c["X_f"], c["X_u"], c["u"], c["X_lo"], c["X_hi"],
                                           co[:6], c["s"], c["X_w"], c["alpha"], c["beta"], c["g"])
    assert l2 == l1 and np.all(g2 == g1)
    assert np.all(e2["f"] == e1["f"]) and np.all(e2["r"] == e1["r"])
    assert all(e2[k] == e1[k] for k in ("mse_f", "mse_u", "mse_b", "mse_w"))


def test_float32_sweep_is_the_same_algebra():
    """the float32 sweep (what measures the helper's own float32 error for the GPU test) tracks float64 at float32 accuracy"""
    c = case([-1.0, 0.0], [1.0, 2.0], seed=5)
    co = adr2_ref.COEFF_SETS["all"]
    l64, g64, _ = helper(c, co)
    l32, g32, e32 = helper(c, co, dtype=np.float32)
    assert g32.dtype == np.float32 and e32["f"].dtype == np.float32
    assert 0.0 < abs(l32 - l64) / l64 < 1e-4 and 0.0 < rel(g32, g64) < 1e-3


# ---- 3. the scripts' exact fields -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("equation", ["wave", "telegraph", "klein_gordon"])
def test_wave_field_satisfies_its_equation(equation):
    """b u_t - nu (u_xx + kappa u_tt) + r1 u + r3 u^3 = s by torch autograd at 50 random (x, t), to 1e-9 of max |u_tt|; the
    walls and the initial velocity are zero"""
    import torch
    sys.path.insert(0, os.path.join(PKG, "1d-wave"))
    import waveutil
    rs = np.random.RandomState(0)
    xn, tn = rs.uniform(-1, 1, 50), rs.uniform(0, 1, 50)
    x = torch.tensor(xn, requires_grad=True)
    t = torch.tensor(tn, requires_grad=True)
    c, pi = waveutil.C, np.pi
    u = torch.sin(pi * x) * torch.cos(c * pi * t) + 0.5 * torch.sin(2 * pi * x) * torch.cos(2 * c * pi * t)
    assert np.allclose(u.detach().numpy(), waveutil.exact_solution(xn, tn), rtol=1e-13, atol=1e-15)
    u_x, u_t = torch.autograd.grad(u.sum(), (x, t), create_graph=True)
    u_xx = torch.autograd.grad(u_x.sum(), x, create_graph=True)[0]
    u_tt = torch.autograd.grad(u_t.sum(), t, create_graph=True)[0]
    a0, a1, nu, r1, r2, r3, b, kappa = waveutil.adr2_coeffs(equation)
    assert (a0, a1, r2) == (0.0, 0.0, 0.0) and nu == c * c and kappa == -1.0 / (c * c)
    s = torch.tensor(waveutil.source(np.column_stack([xn, tn]), equation))
    f = (b * u_t - nu * (u_xx + kappa * u_tt) + r1 * u + r3 * u ** 3 - s).detach().numpy()
    scale = float(np.max(np.abs(u_tt.detach().numpy())))
    assert scale > 1.0 and np.max(np.abs(f)) <= 1e-9 * scale, (np.max(np.abs(f)), scale)
    if equation == "wave":
        assert np.all(waveutil.source(np.column_stack([xn, tn]), equation) == 0.0)
    tt = np.linspace(0, 1, 11)
    assert np.max(np.abs(waveutil.exact_solution(np.array([-1.0, 1.0])[:, None], tt))) < 1e-14
    assert np.allclose(u_t.detach().numpy(), waveutil.exact_velocity(xn, tn), rtol=1e-12, atol=1e-13)
    assert np.all(waveutil.exact_velocity(xn, 0.0) == 0.0)


def test_helmholtz_field_satisfies_its_equation():
    """-Laplace u - k^2 u = s for u* = sin(pi x) sin(4 pi y) by torch autograd, to 1e-9 of max |Laplace u|; zero on the walls"""
    import torch
    sys.path.insert(0, os.path.join(PKG, "2d-helmholtz"))
    import helmholtzutil as hu
    rs = np.random.RandomState(1)
    xn, yn = rs.uniform(-1, 1, 50), rs.uniform(-1, 1, 50)
    x = torch.tensor(xn, requires_grad=True)
    y = torch.tensor(yn, requires_grad=True)
    u = torch.sin(np.pi * x) * torch.sin(4 * np.pi * y)
    assert np.allclose(u.detach().numpy(), hu.exact_solution(xn, yn), rtol=1e-13, atol=1e-15)
    u_x, u_y = torch.autograd.grad(u.sum(), (x, y), create_graph=True)
    u_xx = torch.autograd.grad(u_x.sum(), x, create_graph=True)[0]
    u_yy = torch.autograd.grad(u_y.sum(), y, create_graph=True)[0]
    lap = (u_xx + u_yy).detach().numpy()
    k = 4.0
    assert hu.adr2_coeffs(k) == (0.0, 0.0, 1.0, -k * k, 0.0, 0.0, 0.0, 1.0)
    f = -lap - k * k * u.detach().numpy() - hu.source(np.column_stack([xn, yn]), k)
    scale = float(np.max(np.abs(lap)))
    assert scale > 10.0 and np.max(np.abs(f)) <= 1e-9 * scale, (np.max(np.abs(f)), scale)
    e = np.linspace(-1, 1, 9)
    for X in (np.column_stack([np.full(9, -1.0), e]), np.column_stack([np.full(9, 1.0), e]),
              np.column_stack([e, np.full(9, -1.0)]), np.column_stack([e, np.full(9, 1.0)])):
        assert np.max(np.abs(hu.exact_solution(X[:, 0], X[:, 1]))) < 1e-14


# ---- 4. header and binding ---------------------------------------------------------------------------------------------------
def test_enum_binding_and_abi_version():
    import pinn_native
    text = open(os.path.join(ROOT, "include", "pinn_hip.h")).read()
    assert re.search(r"PINN_PDE_ADR2\s*=\s*10\b", text)
    assert pinn_native.ADR2_PDE_KINDS == {"adr2": 10} and pinn_native.pde_kind("adr2") == 10
    assert pinn_native.PDE_KINDS == {"burgers": 0, "burgers_ide": 1, "schrodinger": 2, "burgers_disc": 3,
                                     "burgers_disc_ide": 4, "adr": 5, "adr_ide": 6}
    assert pinn_native.DISC_PDE_KINDS == {"adr_disc": 7, "adr_disc_ide": 8, "adrd_disc": 9}
    assert pinn_native.ADR2_COEFF_NAMES == ("a0", "a1", "nu", "r1", "r2", "r3", "b", "kappa")
    with pytest.raises(ValueError, match="pde must be one of"):
        pinn_native.pde_kind("adr3")
    assert pinn_native.load().pinn_abi_version() == 6
    src = open(os.path.join(ROOT, "pinns-tf2.0_amd", "csrc", "kernels_generic.h")).read()
    assert re.search(r"PDE_ADR2 = 9\b", src)


def test_set_robin3_is_exported_with_its_declared_signature():
    """the symbol is in the library, the header declares eight arguments, the binding passes eight of the same types"""
    import pinn_native
    lib = pinn_native.load()
    fn = lib.pinn_set_robin3
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pinn_hip.h")).read(), flags=re.S)
    m = re.search(r"int\s+pinn_set_robin3\s*\(([^)]*)\)\s*;", text)
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["pinn_ctx* c", "const double* X_w", "const double* alpha", "const double* beta", "const double* gamma",
                    "const double* g", "int64_t n", "int64_t n_total"]
    dp = ctypes.POINTER(ctypes.c_double)
    assert fn.restype is ctypes.c_int
    assert list(fn.argtypes) == [ctypes.c_void_p, dp, dp, dp, dp, dp, ctypes.c_int64, ctypes.c_int64]
    assert hasattr(pinn_native.Engine, "set_robin3")
    # refusals that need no context and no device: the arrays are looked at first
    one = (ctypes.c_double * 2)(0.0, 0.5)
    z, nan = (ctypes.c_double * 1)(0.0), (ctypes.c_double * 1)(float("nan"))
    assert fn(None, one, z, z, z, z, 1, 1) == -1 and b"alpha = beta = gamma = 0" in lib.pinn_last_error()
    assert fn(None, one, z, z, nan, z, 1, 1) == -1 and b"not finite" in lib.pinn_last_error()
    assert fn(None, one, z, z, z, z, 2, 1) == -1 and b"bad counts" in lib.pinn_last_error()


_HP = {"layers": [2, 20, 20, 1], "tf_epochs": 1, "tf_lr": 0.01, "tf_b1": 0.9, "tf_eps": None, "nt_epochs": 1,
       "nt_lr": 0.8, "nt_ncorr": 50, "log_frequency": 1}


@pytest.mark.parametrize("extra,match", [
    ({"adr2": {"kapa": 1.0}}, "unknown coefficient"),
    ({"adr2": [0.0, 1.0, 0.1, 0.0, 0.0, 0.0]}, "eight numbers"),
    ({"adr2": {"kappa": float("inf")}}, "finite"),
    ({"adr2": 3.0}, "dict of names"),
    ({"point_weights": True}, "point_weights"),
    ({"sa_weights": True}, "sa_weights"),
    ({"resample": "rad", "resample_every": 5}, "rad"),
], ids=["unknown-name", "six-values", "non-finite", "a-number", "point-weights", "sa-weights", "rad"])
def test_hp_options_of_the_script_kind_need_no_device(extra, match):
    import neuralnetwork as nn
    with pytest.raises(ValueError, match=match):
        nn.NeuralNetwork(dict(_HP, **extra), None, np.array([1.0, 1.0]), np.array([-1.0, 0.0]), pde="adr2")
    assert nn.ADR2_NAMES == nn.ADR_NAMES + ("b", "kappa")
    assert nn._adr2_options({"adr2": {"kappa": -0.25, "b": 0.0}}) == (0.0, 1.0, 0.01 / np.pi, 0.0, 0.0, 0.0, 0.0, -0.25)
    assert nn._adr2_options({}) == (0.0, 1.0, 0.01 / np.pi, 0.0, 0.0, 0.0, 1.0, 0.0)
