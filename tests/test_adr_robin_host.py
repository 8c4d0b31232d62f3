"""CPU: Robin points of the adr kind (include/pinn_hip.h pinn_set_robin / pinn_robin_residual, the PDE_ADR_ROBIN variants of
csrc/kernels_generic.h and csrc/kernels_fused20d.h, pinn_native.Engine.set_robin, NeuralNetwork._set_robin) without a device.

  * tests/helpers/adr_robin_ref.py, the numpy restatement the GPU tests use: against torch autograd in float64 (u_x by
    autograd.grad) at the bound tests/test_adr_host.py holds adr_ref to; with no Robin points it IS adr_ref (bit for bit);
    Dirichlet rows (1, 0, g) give adr_ref's data term of the same points;
  * the two symbols, their ctypes signatures, the ABI version; the refusals of pinn_set_robin that need no context (the
    arrays are checked first), Engine.set_robin's ValueErrors with the library stubbed out, NeuralNetwork._set_robin's;
    (a context of another kind needs a device to exist: that refusal is in tests/test_gpu_adr_robin.py)
  * 1d-heat/heatutil.py: the eigenvalue, and the exact field against the equation and both wall conditions.
"""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from conftest import PKG, ROOT

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
sys.path.insert(0, os.path.join(PKG, "utils"))
sys.path.insert(0, os.path.join(PKG, "1d-heat"))
import adr_ref  # noqa: E402
import adr_robin_ref  # noqa: E402

LB, UB = np.array([-1.0, 0.0]), np.array([1.0, 1.0])
LAYERS = [2] + [20] * 8 + [1]
ROBIN_SYMBOLS = {"pinn_set_robin": 7, "pinn_robin_residual": 3}


def rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300)


def _weights(layers, seed=5):
    from oracle import init
    w = init.glorot_flat(layers)
    return w + 0.05 * np.random.RandomState(seed).standard_normal(w.size)


def _sets(seed=9, n_f=256, n_u=64, n_b=7, n_w=33):
    rs = np.random.RandomState(seed)
    X_f = LB + (UB - LB) * rs.uniform(size=(n_f, 2))
    X_u = np.column_stack([rs.uniform(-1, 1, n_u), np.zeros(n_u)])
    u = (X_u[:, 0:1] ** 2) * np.cos(np.pi * X_u[:, 0:1])
    tb = rs.uniform(0, 1, n_b)
    X_lo, X_hi = np.column_stack([np.full(n_b, -1.0), tb]), np.column_stack([np.full(n_b, 1.0), tb])
    X_w = np.column_stack([np.where(np.arange(n_w) % 2, 1.0, -1.0), rs.uniform(0, 1, n_w)])
    alpha, beta, g = rs.uniform(-1.5, 1.5, n_w), rs.uniform(-1.5, 1.5, n_w), rs.uniform(-1, 1, n_w)
    alpha[::5] = 0.0
    beta[(np.arange(n_w) % 7 == 3) & (alpha != 0.0)] = 0.0           # (a row with both 0 constrains nothing and is refused)
    assert not np.any((alpha == 0) & (beta == 0)) and np.any(alpha == 0) and np.any(beta == 0)
    return (X_f, X_u, u, X_lo, X_hi), (X_w, alpha, beta, g)


def _torch_loss_grad(w, layers, X_f, X_u, u, X_lo, X_hi, coeffs, X_w, alpha, beta, g):
    import torch
    torch.set_num_threads(4)
    a0, a1, nu, r1, r2, r3 = coeffs
    wt = torch.tensor(w, dtype=torch.float64, requires_grad=True)
    lb, ub = torch.tensor(LB), torch.tensor(UB)

    def net(x, t):
        h = 2.0 * (torch.cat([x, t], dim=1) - lb) / (ub - lb) - 1.0
        off = 0
        for i, (fi, fo) in enumerate(zip(layers[:-1], layers[1:])):
            W = wt[off:off + fi * fo].reshape(fi, fo)
            b = wt[off + fi * fo:off + fi * fo + fo]
            off += fi * fo + fo
            h = h @ W + b
            if i < len(layers) - 2:
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

    col = lambda v: torch.tensor(np.asarray(v, dtype=np.float64).reshape(-1, 1))      # noqa: E731
    uu, u_x, u_t, u_xx = channels(X_f)
    f = u_t + (a0 + a1 * uu) * u_x - nu * u_xx + r1 * uu + r2 * uu ** 2 + r3 * uu ** 3
    loss = torch.mean(f ** 2)
    loss = loss + torch.mean((channels(X_u)[0] - torch.tensor(u)) ** 2)
    ul, ul_x, _, _ = channels(X_lo)
    uh, uh_x, _, _ = channels(X_hi)
    loss = loss + torch.mean((ul - uh) ** 2) + torch.mean((ul_x - uh_x) ** 2)
    uw, uw_x, _, _ = channels(X_w)
    r = col(alpha) * uw + col(beta) * uw_x - col(g)
    loss = loss + torch.mean(r ** 2)
    loss.backward()
    return float(loss.detach()), wt.grad.numpy().copy(), r.detach().numpy().ravel()


# ---- 1. the restatement against autograd ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(adr_ref.COEFF_SETS))
def test_restatement_against_torch_autograd(name):
    """8 x 20, N_f = 256, 64 data points, 7 pairs, 33 Robin points with rows alpha = 0 and rows beta = 0; asserted at
    tests/test_adr_host.py's 1e-14 (loss) / 1e-13 (gradient, by its largest entry)"""
    base, rob = _sets()
    co = adr_ref.COEFF_SETS[name]
    w = _weights(LAYERS)
    lo, go, ex = adr_robin_ref.robin_loss_grad(w, LAYERS, LB, UB, *base, co, *rob)
    lt, gt, rt = _torch_loss_grad(w, LAYERS, *base, co, *rob)
    print("adr_robin_ref vs autograd %s: loss %.2e grad %.2e r %.2e" % (name, abs(lo - lt) / abs(lt), rel(go, gt), rel(ex["r"], rt)))
    assert ex["mse_w"] > 0 and ex["r"].shape == (33,)
    assert abs(lo - lt) / abs(lt) < 1e-14
    assert rel(go, gt) < 1e-13
    assert rel(ex["r"], rt) < 1e-13
    assert np.array_equal(ex["r"], adr_robin_ref.robin_residual(w, LAYERS, LB, UB, *rob))


# ---- 2. no Robin points: adr_ref itself ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["allen_cahn", "all_nonzero"])
def test_no_robin_points_is_the_plain_oracle_bit_for_bit(name):
    base, _ = _sets()
    co = adr_ref.COEFF_SETS[name]
    w = _weights(LAYERS)
    lo, go, ex = adr_ref.adr_loss_grad(w, LAYERS, LB, UB, *base, co)
    for rob in ((), (None, None, None, None), (np.zeros((0, 2)), np.zeros(0), np.zeros(0), np.zeros(0))):
        l1, g1, e1 = adr_robin_ref.robin_loss_grad(w, LAYERS, LB, UB, *base, co, *rob)
        assert l1 == lo and np.array_equal(g1, go)
        assert e1["mse_w"] == 0.0 and e1["r"].size == 0
        assert (e1["mse_f"], e1["mse_u"], e1["mse_b"]) == (ex["mse_f"], ex["mse_u"], ex["mse_b"])


# ---- 3. Dirichlet rows are data points ---------------------------------------------------------------------------------
def test_dirichlet_rows_equal_the_data_term_of_the_same_points():
    (X_f, X_u, u, X_lo, X_hi), (X_w, _, _, g) = _sets()
    co = adr_ref.ALLEN_CAHN
    w = _weights(LAYERS)
    # the points as Robin rows (1, 0, g), no data set ...
    l_r, g_r, e_r = adr_robin_ref.robin_loss_grad(w, LAYERS, LB, UB, X_f, None, None, X_lo, X_hi, co, X_w, 1.0, 0.0, g)
    # ... and as data points with the same count
    l_d, g_d, e_d = adr_ref.adr_loss_grad(w, LAYERS, LB, UB, X_f, X_w, g.reshape(-1, 1), X_lo, X_hi, co)
    assert e_r["mse_u"] == 0.0 and e_r["mse_b"] == e_d["mse_b"]                 # mse_w is a part of its own in the helper;
    assert abs(e_r["mse_w"] - e_d["mse_u"]) <= 1e-15 * e_d["mse_u"]             # the device adds it to the boundary part
    assert abs(l_r - l_d) <= 1e-15 * l_d
    assert rel(g_r, g_d) < 1e-13


# ---- 4. the C surface --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ROBIN_SYMBOLS))
def test_robin_symbols_are_declared_exported_and_typed(name):
    import pinn_native
    lib = pinn_native.load()
    header = open(os.path.join(ROOT, "include", "pinn_hip.h")).read()
    proto = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header)
    assert proto, "%s is not declared" % name
    assert name in pinn_native.exported_symbols()
    res, args = pinn_native._SIGNATURES[name]
    fn = getattr(lib, name)
    assert fn.restype is res is ctypes.c_int and list(fn.argtypes) == list(args)
    assert len([a for a in proto.group(1).split(",") if a.strip()]) == len(args) == ROBIN_SYMBOLS[name]
    assert lib.pinn_abi_version() == 6
    assert "the ABI version stays 6" in header[header.index("Robin points of the adr kind"):header.index("int pinn_set_robin")]


# ---- 5. refusals before any device work -----------------------------------------------------------------------------------
def _arr(*v):
    return (ctypes.c_double * len(v))(*v)


def test_set_robin_refuses_bad_arguments_before_it_looks_at_the_context():
    """pinn_set_robin checks its arrays first (they need no context), so these refusals are reached without a device; each is
    PINN_EINVAL with its reason in pinn_last_error"""
    import pinn_native
    lib = pinn_native.load()
    X, one, zero = _arr(0.0, 0.5, 1.0, 0.5), _arr(1.0, 1.0), _arr(0.0, 0.0)
    cases = [
        ((X, one, one, zero, 2, 1), b"bad counts"),                      # n_total < n
        ((X, one, one, zero, -1, 1), b"bad counts"),                     # n < 0
        ((None, one, one, zero, 2, 2), b"null array"),
        ((X, None, one, zero, 2, 2), b"null array"),
        ((X, one, None, zero, 2, 2), b"null array"),
        ((X, one, one, None, 2, 2), b"null array"),
        ((X, _arr(1.0, 0.0), _arr(1.0, 0.0), zero, 2, 2), b"alpha = beta = 0"),
        ((_arr(0.0, np.nan, 1.0, 0.5), one, one, zero, 2, 2), b"not finite"),
        ((_arr(0.0, 0.5, np.inf, 0.5), one, one, zero, 2, 2), b"not finite"),
        ((X, _arr(1.0, np.nan), one, zero, 2, 2), b"not finite"),
        ((X, one, _arr(-np.inf, 1.0), zero, 2, 2), b"not finite"),
        ((X, one, one, _arr(0.0, np.nan), 2, 2), b"not finite"),
    ]
    for args, why in cases:
        assert lib.pinn_set_robin(None, *args) == -1                     # PINN_EINVAL
        assert why in lib.pinn_last_error(), (why, lib.pinn_last_error())
    # good arrays: the null context is what is left to refuse
    assert lib.pinn_set_robin(None, X, one, one, zero, 2, 2) == -1 and b"null context" in lib.pinn_last_error()
    assert lib.pinn_set_robin(None, None, None, None, None, 0, 0) == -1 and b"null context" in lib.pinn_last_error()
    assert lib.pinn_robin_residual(None, one, 2) == -1
    for m in ("set_robin", "robin_residual"):
        assert hasattr(pinn_native.Engine, m)


class _Lib(object):
    def __init__(self):
        self.seen = []

    def pinn_set_robin(self, h, X, a, b, g, n, n_total):
        self.seen.append((n, n_total, [X[i] for i in range(2 * n)], [a[i] for i in range(n)], [b[i] for i in range(n)],
                          [g[i] for i in range(n)]))
        return 0


def _stub_engine():
    import pinn_native
    eng = pinn_native.Engine.__new__(pinn_native.Engine)
    eng._lib, eng._h, eng.n_u, eng.n_f, eng.n_b, eng.n_w = _Lib(), None, 0, 0, 0, 0
    return eng


def test_engine_set_robin_broadcasts_scalars_and_counts():
    eng = _stub_engine()
    eng.set_robin([[0.0, 0.1], [1.0, 0.2], [1.0, 0.3]], 2.0, [1.0, 0.0, 1.0], 0.0)
    assert eng.n_w == 3
    assert eng._lib.seen[-1] == (3, 3, [0.0, 0.1, 1.0, 0.2, 1.0, 0.3], [2.0, 2.0, 2.0], [1.0, 0.0, 1.0], [0.0, 0.0, 0.0])
    eng.set_robin(np.zeros((2, 2)), [0.0, 1.0], 1.0, [0.5, -0.5], n_total=10)
    assert eng._lib.seen[-1][:2] == (2, 10) and eng.n_w == 2
    eng.set_robin(np.zeros((0, 2)), 1.0, 0.0, 0.0)                      # removes the class
    assert eng._lib.seen[-1][:2] == (0, 0) and eng.n_w == 0


@pytest.mark.parametrize("args, match", [
    ((np.zeros((3, 3)), 1.0, 1.0, 0.0), "X_w"),
    ((np.zeros(5), 1.0, 1.0, 0.0), "X_w"),
    ((np.zeros((3, 2)), [1.0, 1.0], 1.0, 0.0), "alpha"),
    ((np.zeros((3, 2)), 1.0, np.ones(4), 0.0), "beta"),
    ((np.zeros((3, 2)), 1.0, 1.0, np.zeros(2)), "g "),
    ((np.zeros((3, 2)), np.nan, 1.0, 0.0), "alpha.*finite"),
    ((np.zeros((3, 2)), 1.0, [1.0, np.inf, 1.0], 0.0), "beta.*finite"),
    ((np.zeros((3, 2)), 1.0, 1.0, [0.0, 0.0, np.nan]), "g .*finite"),
    ((np.array([[0.0, np.nan], [0.0, 0.0], [0.0, 0.0]]), 1.0, 1.0, 0.0), "X_w.*finite"),
    ((np.zeros((3, 2)), [1.0, 0.0, 1.0], [0.0, 0.0, 1.0], 0.0), "alpha = beta = 0"),
    ((np.zeros((3, 2)), 0.0, 0.0, 0.0), "alpha = beta = 0"),
])
def test_engine_set_robin_raises_value_errors_before_any_library_call(args, match):
    eng = _stub_engine()
    eng.n_w = 5
    with pytest.raises(ValueError, match=match):
        eng.set_robin(*args)
    assert eng._lib.seen == [] and eng.n_w == 5
    with pytest.raises(ValueError, match="n_total"):
        eng.set_robin(np.zeros((3, 2)), 1.0, 1.0, 0.0, n_total=2)
    assert eng._lib.seen == []


# ---- 6. NeuralNetwork._set_robin, engine stubbed ---------------------------------------------------------------------------
class _Engine(object):
    def __init__(self, layers, lb, ub, pde="burgers", dtype="f64", device=0):
        self.n_params, self.w, self.calls, self.pde = 5, np.zeros(5), [], pde
        self.n_f = self.n_u = self.n_b = self.n_w = 0

    def set_weights(self, w): self.w = np.array(w, dtype=np.float64)
    def get_weights(self): return self.w.copy()
    def adam_init(self, *a): pass
    def pw_adam_init(self, *r): pass
    def set_pde_trainable(self, *a): pass
    def set_robin(self, X_w, alpha, beta, g, n_total=None): self.n_w = len(X_w); self.calls.append(("robin", len(X_w)))


def _hp(**kw):
    hp = {"layers": [2, 20, 20, 20, 20, 1], "tf_epochs": 1, "tf_lr": 0.01, "tf_b1": 0.9, "tf_eps": None,
          "nt_epochs": 1, "nt_lr": 0.8, "nt_ncorr": 50, "log_frequency": 1}
    hp.update(kw)
    return hp


def _nn(monkeypatch, pde, **kw):
    import neuralnetwork
    from logger import Logger
    monkeypatch.setattr(neuralnetwork, "Engine", _Engine)
    hp = _hp(**kw)
    return neuralnetwork.NeuralNetwork(hp, Logger(hp), UB, LB, pde=pde)


def test_neuralnetwork_set_robin_passes_through_for_the_adr_kind(monkeypatch):
    nn = _nn(monkeypatch, "adr")
    nn._set_robin(np.zeros((4, 2)), 1.0, 0.0, 0.0)
    assert nn._engine.calls == [("robin", 4)]
    nn = _nn(monkeypatch, "adr", resample_every=10, resample="rad")            # redraws go with Robin points
    nn._set_robin(np.zeros((4, 2)), 0.0, 1.0, 0.0)
    assert nn._engine.calls == [("robin", 4)]


@pytest.mark.parametrize("pde, kw, match", [
    ("adr", {"point_weights": True}, "_set_robin.*point_weights"),
    ("burgers", {}, "_set_robin.*adr.*burgers"),
    ("adr_ide", {"adr_trainable": ["nu"]}, "_set_robin.*adr.*adr_ide"),
    ("schrodinger", {"layers": [2, 20, 20, 2]}, "_set_robin.*adr.*schrodinger"),
])
def test_neuralnetwork_set_robin_refuses_by_name(monkeypatch, pde, kw, match):
    nn = _nn(monkeypatch, pde, **kw)
    with pytest.raises(ValueError, match=match):
        nn._set_robin(np.zeros((4, 2)), 1.0, 0.0, 0.0)
    assert nn._engine.calls == []


def test_a_data_parallel_launch_stays_refused_for_the_kind(monkeypatch):
    import neuralnetwork
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setenv("LOCAL_RANK", "0")
    with pytest.raises(ValueError, match='"adr".*data-parallel'):
        neuralnetwork.NeuralNetwork(_hp(), None, UB, LB, pde="adr")


# ---- 7. heatutil -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", [0.1, 1.0, 10.0])
def test_first_root_and_the_exact_field(h):
    import heatutil as hu
    mu = hu.first_root(h)
    assert 0.0 < mu < np.pi / 2
    assert abs(mu * np.tan(mu) - h) <= 1e-14
    # the field against the equation and both walls: central differences with steps that keep truncation (d^2 / 6 times a
    # third / fourth derivative of size <= mu^4 < 5) and rounding (2^-52 / d^2) under the 1e-6 asserted
    nu, d = 0.1, 1e-3
    u = lambda x, t: hu.exact_solution(x, t, nu, h)                               # noqa: E731
    x, t = np.meshgrid(np.linspace(0.05, 0.95, 13), np.linspace(0.05, 0.95, 11))
    u_t = (u(x, t + d) - u(x, t - d)) / (2 * d)
    u_xx = (u(x + d, t) - 2 * u(x, t) + u(x - d, t)) / (d * d)
    assert np.max(np.abs(u_t - nu * u_xx)) < 1e-6
    tw = np.linspace(0.0, 1.0, 21)
    ux0 = (u(d, tw) - u(-d, tw)) / (2 * d)
    ux1 = (u(1 + d, tw) - u(1 - d, tw)) / (2 * d)
    assert np.max(np.abs(ux0)) < 1e-6                                             # insulated
    assert np.max(np.abs(ux1 + h * u(1.0, tw))) < 1e-6                            # Newton cooling
    assert np.array_equal(u(x, 0 * t), np.cos(mu * x))


def test_heat_prep_data_shapes_and_wall_rows():
    import heatutil as hu
    np.random.seed(1234)
    (x, t, X, T, Exact_u, X_star, u_star, X_u, u, X_f, X_w, alpha, beta, g, ub, lb) = hu.prep_data(32, 20, 500, nu=0.1, h=2.0)
    assert X_star.shape == (hu.N_X * hu.N_T, 2) and u_star.shape == (hu.N_X * hu.N_T, 1)
    assert X_u.shape == (32, 2) and u.shape == (32, 1) and np.all(X_u[:, 1] == 0.0)
    assert X_f.shape == (500, 2) and np.all(X_f >= lb) and np.all(X_f <= ub)
    assert X_w.shape == (40, 2) and np.all(X_w[:20, 0] == 0.0) and np.all(X_w[20:, 0] == 1.0)
    assert np.all(alpha[:20] == 0.0) and np.all(alpha[20:] == 2.0) and np.all(beta == 1.0) and np.all(g == 0.0)
    assert hu.adr_coeffs(0.1) == (0.0, 0.0, 0.1, 0.0, 0.0, 0.0)
    assert list(lb) == [0.0, 0.0] and list(ub) == [1.0, 1.0]
