"""CPU: the source term of the adr kind (include/pinn_hip.h pinn_set_source, the PDE_ADR_SRC variants of
csrc/kernels_generic.h and csrc/kernels_fused20d.h, pinn_native.Engine.set_source, NeuralNetwork._set_source, 1d-mms) without
a device.

  * tests/helpers/adr_src_ref.py, the numpy restatement the GPU tests use: against torch autograd in float64 at Robin's
    host pins (1e-14 loss, 1e-13 gradient); with a zero source it IS adr_ref (bit for bit);
  * 1d-mms/mmsutil.py: for every equation s = N[u*] against torch autograd of u*; walls and initial data are u*'s;
  * the symbol, its ctypes signature, the ABI version, the header text; the refusals of pinn_set_source that need no
    context (the array is checked first); Engine.set_source's and NeuralNetwork._set_source's ValueErrors with the library
    stubbed out.  (A context of another kind needs a device to exist: those refusals are in tests/test_gpu_adr_source.py.)
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
sys.path.insert(0, os.path.join(PKG, "1d-mms"))
import adr_ref  # noqa: E402
import adr_src_ref  # noqa: E402

LB, UB = np.array([-1.0, 0.0]), np.array([1.0, 1.0])


def rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300)


def layers_of(depth):
    return [2] + [20] * depth + [1]


def source_of(X):
    return np.sin(3.0 * X[:, 0]) * np.exp(-X[:, 1]) + 0.5


def _weights(layers, seed=5):
    from oracle import init
    w = init.glorot_flat(layers)
    return w + 0.05 * np.random.RandomState(seed).standard_normal(w.size)


def _sets(seed=9, n_f=2048, n_u=512, n_b=7, n_w=33):
    rs = np.random.RandomState(seed)
    X_f = LB + (UB - LB) * rs.uniform(size=(n_f, 2))
    X_u = np.column_stack([rs.uniform(-1, 1, n_u), np.zeros(n_u)])
    u = (X_u[:, 0:1] ** 2) * np.cos(np.pi * X_u[:, 0:1])
    tb = rs.uniform(0, 1, n_b)
    X_lo, X_hi = np.column_stack([np.full(n_b, -1.0), tb]), np.column_stack([np.full(n_b, 1.0), tb])
    X_w = np.column_stack([np.where(np.arange(n_w) % 2, 1.0, -1.0), rs.uniform(0, 1, n_w)])
    alpha, beta, g = rs.uniform(-1.5, 1.5, n_w), rs.uniform(-1.5, 1.5, n_w), rs.uniform(-1, 1, n_w)
    alpha[::5] = 0.0
    return (X_f, X_u, u, X_lo, X_hi), (X_w, alpha, beta, g)


def _torch_loss_grad(w, layers, X_f, X_u, u, X_lo, X_hi, coeffs, s, X_w, alpha, beta, g):
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
    f = u_t + (a0 + a1 * uu) * u_x - nu * u_xx + r1 * uu + r2 * uu ** 2 + r3 * uu ** 3 - col(s)
    loss = torch.mean(f ** 2)
    loss = loss + torch.mean((channels(X_u)[0] - torch.tensor(u)) ** 2)
    ul, ul_x, _, _ = channels(X_lo)
    uh, uh_x, _, _ = channels(X_hi)
    loss = loss + torch.mean((ul - uh) ** 2) + torch.mean((ul_x - uh_x) ** 2)
    uw, uw_x, _, _ = channels(X_w)
    r = col(alpha) * uw + col(beta) * uw_x - col(g)
    loss = loss + torch.mean(r ** 2)
    loss.backward()
    return float(loss.detach()), wt.grad.numpy().copy(), f.detach().numpy()


# ---- 1. the restatement against autograd ------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [4, 8])
@pytest.mark.parametrize("name", sorted(adr_ref.COEFF_SETS))
def test_restatement_against_torch_autograd(name, depth):
    """N_f = 2048, n_0 = 512, 7 pairs, 33 Robin points, s_i = sin(3 x_i) exp(-t_i) + 0.5; asserted at Robin's host pins,
    1e-14 (loss) / 1e-13 (gradient, by its largest entry).  The source must matter: the loss moves by more than 1e-3 against
    s = 0 (printed: 12 % to 131 %), eleven orders above the bound, so a restatement that ignores s fails by as much."""
    base, rob = _sets()
    layers, co = layers_of(depth), adr_ref.COEFF_SETS[name]
    w = _weights(layers)
    s = source_of(base[0])
    lo, go, ex = adr_src_ref.src_loss_grad(w, layers, LB, UB, *base, co, s, *rob)
    lt, gt, ft = _torch_loss_grad(w, layers, *base, co, s, *rob)
    l0 = adr_src_ref.src_loss_grad(w, layers, LB, UB, *base, co, None, *rob)[0]
    print("adr_src_ref vs autograd %s depth %d: loss %.2e grad %.2e f %.2e | loss moved by %.0f %%" % (
        name, depth, abs(lo - lt) / abs(lt), rel(go, gt), rel(ex["f"], ft), 100 * abs(lo - l0) / l0))
    assert abs(lo - lt) / abs(lt) < 1e-14
    assert rel(go, gt) < 1e-13
    assert rel(ex["f"], ft) < 1e-13
    assert abs(lo - l0) / l0 > 1e-3
    assert np.array_equal(ex["f"], adr_src_ref.residual(w, layers, LB, UB, base[0], co, s))


# ---- 2. a zero source: adr_ref itself ------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [4, 8])
@pytest.mark.parametrize("name", sorted(adr_ref.COEFF_SETS))
def test_zero_source_is_the_plain_oracle_bit_for_bit(name, depth):
    base, _ = _sets()
    layers, co = layers_of(depth), adr_ref.COEFF_SETS[name]
    w = _weights(layers)
    lo, go, ex = adr_ref.adr_loss_grad(w, layers, LB, UB, *base, co)
    for s in (None, np.zeros(len(base[0])), -np.zeros(len(base[0]))):
        l1, g1, e1 = adr_src_ref.src_loss_grad(w, layers, LB, UB, *base, co, s)
        assert l1 == lo and np.array_equal(g1, go) and np.array_equal(e1["f"], ex["f"])
        assert (e1["mse_f"], e1["mse_u"], e1["mse_b"], e1["mse_w"]) == (ex["mse_f"], ex["mse_u"], ex["mse_b"], 0.0)
    with pytest.raises(ValueError, match="one value per collocation point"):
        adr_src_ref.src_loss_grad(w, layers, LB, UB, *base, co, np.zeros(5))


# ---- 3. mmsutil -------------------------------------------------------------------------------------------------------------
def test_mms_equations_are_the_named_five():
    import mmsutil as mu
    assert sorted(mu.EQUATIONS) == ["advection_diffusion", "allen_cahn", "burgers", "fisher_kpp", "heat"]
    for name in ("burgers", "allen_cahn", "fisher_kpp", "advection_diffusion"):
        assert list(mu.adr_coeffs(name)) == [float(v) for v in adr_ref.COEFF_SETS[name]]
    assert mu.adr_coeffs("heat") == (0.0, 0.0, 0.1, 0.0, 0.0, 0.0)
    with pytest.raises(ValueError, match="equation"):
        mu.adr_coeffs("wave")


@pytest.mark.parametrize("name", ["burgers", "allen_cahn", "fisher_kpp", "advection_diffusion", "heat"])
def test_mms_source_is_the_operator_on_the_exact_field(name):
    """s = N[u*] from the closed-form derivatives against torch autograd of u* itself, to 1e-12 (the values are O(10):
    pi^2 u* dominates; autograd and the closed form differ by a few roundings of such terms)"""
    import torch
    import mmsutil as mu
    rs = np.random.RandomState(4)
    X = LB + (UB - LB) * rs.uniform(size=(500, 2))
    X[:4] = [[-1.0, 0.0], [1.0, 1.0], [0.0, 0.0], [-1.0, 1.0]]
    x = torch.tensor(X[:, 0], requires_grad=True)
    t = torch.tensor(X[:, 1], requires_grad=True)
    u = torch.exp(-t) * torch.sin(np.pi * x) + 0.3 * t * torch.cos(2.0 * np.pi * x)
    ones = torch.ones_like(u)
    u_x, u_t = torch.autograd.grad(u, [x, t], ones, create_graph=True)
    u_xx = torch.autograd.grad(u_x, x, ones)[0]
    a0, a1, nu, r1, r2, r3 = mu.adr_coeffs(name)
    ref = (u_t + (a0 + a1 * u) * u_x - nu * u_xx + r1 * u + r2 * u ** 2 + r3 * u ** 3).detach().numpy()
    s = mu.source(X, mu.adr_coeffs(name))
    assert s.shape == (500,)
    assert np.max(np.abs(s - ref)) < 1e-12 * max(1.0, np.max(np.abs(ref)))
    assert np.max(np.abs(mu.exact_solution(X[:, 0], X[:, 1]) - u.detach().numpy())) < 1e-15


@pytest.mark.parametrize("walls", ["dirichlet", "periodic"])
def test_mms_prep_data_walls_and_initial_data_are_the_exact_fields(walls):
    import mmsutil as mu
    np.random.seed(1234)
    (x, t, X, T, Exact_u, X_star, u_star, X_u, u, X_f, wall, ub, lb) = mu.prep_data(32, 20, 500, walls=walls)
    assert X_star.shape == (mu.N_X * mu.N_T, 2) and u_star.shape == (mu.N_X * mu.N_T, 1)
    assert np.array_equal(u_star.ravel(), mu.exact_solution(X_star[:, 0], X_star[:, 1]))
    assert X_u.shape == (32, 2) and np.all(X_u[:, 1] == 0.0) and np.array_equal(u.ravel(), np.sin(np.pi * X_u[:, 0]))
    assert X_f.shape == (500, 2) and np.all(X_f >= lb) and np.all(X_f <= ub)
    assert list(lb) == [-1.0, 0.0] and list(ub) == [1.0, 1.0] and wall[0] == walls
    if walls == "dirichlet":
        _, X_w, alpha, beta, g = wall
        assert X_w.shape == (40, 2) and np.all(X_w[:20, 0] == -1.0) and np.all(X_w[20:, 0] == 1.0)
        assert np.all(alpha == 1.0) and np.all(beta == 0.0)
        assert np.array_equal(g, mu.exact_solution(X_w[:, 0], X_w[:, 1]))
    else:
        _, X_lo, X_hi = wall
        assert X_lo.shape == X_hi.shape == (20, 2) and np.all(X_lo[:, 0] == -1.0) and np.all(X_hi[:, 0] == 1.0)
        assert np.array_equal(X_lo[:, 1], X_hi[:, 1])
        # u* is 2-periodic in x: value and slope agree across the pair
        cl, ch = mu.exact_channels(X_lo[:, 0], X_lo[:, 1]), mu.exact_channels(X_hi[:, 0], X_hi[:, 1])
        assert np.max(np.abs(cl[0] - ch[0])) < 1e-15 and np.max(np.abs(cl[1] - ch[1])) < 1e-14
    with pytest.raises(ValueError, match="walls"):
        mu.prep_data(4, 4, 4, walls="neumann")


# ---- 4. the C surface --------------------------------------------------------------------------------------------------
def test_source_symbol_is_declared_exported_and_typed():
    import pinn_native
    lib = pinn_native.load()
    header = open(os.path.join(ROOT, "include", "pinn_hip.h")).read()
    proto = re.search(r"\bint\s+pinn_set_source\s*\(([^)]*)\)\s*;", header)
    assert proto, "pinn_set_source is not declared"
    assert "pinn_set_source" in pinn_native.exported_symbols()
    res, args = pinn_native._SIGNATURES["pinn_set_source"]
    fn = lib.pinn_set_source
    assert fn.restype is res is ctypes.c_int and list(fn.argtypes) == list(args)
    assert list(args) == [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.c_int64]
    assert len([a for a in proto.group(1).split(",") if a.strip()]) == 3
    assert lib.pinn_abi_version() == 6
    # the block stands behind pinn_robin_residual and says what the issue fixes
    text = header[header.index("int pinn_robin_residual"):header.index("int pinn_set_source")]
    assert "Source term of the adr kind" in text and "the ABI version stays 6" in text
    for phrase in ("PINN_ESTATE", "pinn_get_collocation still works", "pinn_residual_at cannot know s", "operator part",
                   "pinn_rad_collocation is refused", "bit-identical"):
        assert phrase in text, phrase
    # Robin's block is where tests/test_adr_robin_host.py slices it
    assert "the ABI version stays 6" in header[header.index("Robin points of the adr kind"):header.index("int pinn_set_robin")]


# ---- 5. refusals before any device work -----------------------------------------------------------------------------------
def _arr(*v):
    return (ctypes.c_double * len(v))(*v)


def test_set_source_refuses_bad_arguments_before_it_looks_at_the_context():
    """pinn_set_source checks its array first (it needs no context), so these refusals are reached without a device; each is
    PINN_EINVAL and pinn_last_error names pinn_set_source"""
    import pinn_native
    lib = pinn_native.load()
    cases = [
        ((None, 3), b"null array"),
        ((_arr(0.0, 1.0), -1), b"bad count"),
        ((None, -2), b"bad count"),
        ((_arr(0.0, np.nan, 1.0), 3), b"not finite"),
        ((_arr(np.inf, 0.0), 2), b"not finite"),
        ((_arr(0.0, -np.inf), 2), b"not finite"),
    ]
    for args, why in cases:
        assert lib.pinn_set_source(None, *args) == -1                    # PINN_EINVAL
        err = lib.pinn_last_error()
        assert why in err and b"pinn_set_source" in err, (why, err)
    # a good array, or the removal: the null context is what is left to refuse
    assert lib.pinn_set_source(None, _arr(0.0, 1.0), 2) == -1 and b"pinn_set_source: null context" in lib.pinn_last_error()
    assert lib.pinn_set_source(None, None, 0) == -1 and b"pinn_set_source: null context" in lib.pinn_last_error()


class _Lib(object):
    def __init__(self):
        self.seen = []

    def pinn_set_source(self, h, s, n):
        self.seen.append((n, None if s is None else [s[i] for i in range(n)]))
        return 0


def _stub_engine(n_f=3):
    import pinn_native
    eng = pinn_native.Engine.__new__(pinn_native.Engine)
    eng._lib, eng._h, eng.n_u, eng.n_f, eng.n_b, eng.n_w, eng.n_out = _Lib(), None, 0, n_f, 0, 0, 1
    return eng


def test_engine_set_source_passes_values_and_tracks_has_source():
    eng = _stub_engine()
    assert eng.has_source is False
    eng.set_source([0.5, -1.0, 2.0])
    assert eng._lib.seen[-1] == (3, [0.5, -1.0, 2.0]) and eng.has_source is True
    eng.set_source(np.array([[1.0], [2.0], [3.0]]))                      # a column is taken as [n]
    assert eng._lib.seen[-1] == (3, [1.0, 2.0, 3.0])
    eng.set_source(None)
    assert eng._lib.seen[-1] == (0, None) and eng.has_source is False


@pytest.mark.parametrize("s, match", [
    (np.zeros(2), "one value per collocation point"),
    (np.zeros(4), "one value per collocation point"),
    (np.zeros((3, 2)), "one value per collocation point"),
    ([0.0, np.nan, 0.0], "finite"),
    ([0.0, 0.0, np.inf], "finite"),
])
def test_engine_set_source_raises_value_errors_before_any_library_call(s, match):
    eng = _stub_engine()
    with pytest.raises(ValueError, match=match):
        eng.set_source(s)
    assert eng._lib.seen == [] and eng.has_source is False
    with pytest.raises(ValueError, match="empty"):
        _stub_engine(0).set_source(np.zeros(0))


def test_engine_residual_at_wants_the_source_where_the_context_holds_one():
    eng = _stub_engine()
    eng._has_source = True
    with pytest.raises(ValueError, match="residual_at.*source"):
        eng.residual_at(np.zeros((3, 2)))
    with pytest.raises(ValueError, match="one value per point"):
        eng.residual_at(np.zeros((3, 2)), source=np.zeros(2))


# ---- 6. NeuralNetwork._set_source, engine stubbed ---------------------------------------------------------------------------
class _Engine(object):
    def __init__(self, layers, lb, ub, pde="burgers", dtype="f64", device=0):
        self.n_params, self.w, self.calls, self.pde = 5, np.zeros(5), [], pde
        self.n_f = self.n_u = self.n_b = self.n_w = 0
        self.X = np.zeros((0, 2))

    def set_weights(self, w): self.w = np.array(w, dtype=np.float64)
    def get_weights(self): return self.w.copy()
    def adam_init(self, *a): pass
    def pw_adam_init(self, *r): pass
    def set_pde_trainable(self, *a): pass
    def set_collocation(self, X, n_total=None): self.X = np.array(X); self.n_f = len(X)
    def get_collocation(self): return self.X.copy()
    def set_source(self, s): self.calls.append(("source", None if s is None else np.array(s, dtype=np.float64)))


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


def test_neuralnetwork_set_source_takes_an_array_or_a_callable(monkeypatch):
    X = np.array([[0.0, 0.1], [0.5, 0.2], [-0.5, 0.3]])
    nn = _nn(monkeypatch, "adr")
    nn._set_collocation(X)
    nn._set_source([1.0, 2.0, 3.0])
    assert nn._engine.calls[-1][0] == "source" and list(nn._engine.calls[-1][1]) == [1.0, 2.0, 3.0]
    nn._set_source(lambda P: P[:, 0] + 10.0 * P[:, 1])                   # evaluated at the engine's own points
    assert np.array_equal(nn._engine.calls[-1][1], X[:, 0] + 10.0 * X[:, 1])
    nn._set_source(None)
    assert nn._engine.calls[-1] == ("source", None)
    nn = _nn(monkeypatch, "adr", resample_every=10)                      # a callable goes with LHS redraws
    nn._set_collocation(X)
    nn._set_source(lambda P: P[:, 0])
    assert len(nn._engine.calls) == 1


@pytest.mark.parametrize("pde, kw, s, match", [
    ("burgers", {}, [0.0], "_set_source.*adr.*burgers"),
    ("adr_ide", {"adr_trainable": ["nu"]}, [0.0], "_set_source.*adr.*adr_ide"),
    ("schrodinger", {"layers": [2, 20, 20, 2]}, [0.0], "_set_source.*adr.*schrodinger"),
    ("adr", {"resample_every": 10, "resample": "rad"}, (lambda P: P[:, 0]), "_set_source.*rad"),
    ("adr", {"point_weights": True}, [0.0], "_set_source.*point_weights"),
    ("adr", {"resample_every": 10}, [0.0], "_set_source.*array.*resample_every"),
])
def test_neuralnetwork_set_source_refuses_by_name(monkeypatch, pde, kw, s, match):
    nn = _nn(monkeypatch, pde, **kw)
    with pytest.raises(ValueError, match=match):
        nn._set_source(s)
    assert nn._engine.calls == []


def test_neuralnetwork_set_source_refuses_a_data_parallel_launch(monkeypatch):
    nn = _nn(monkeypatch, "adr")
    nn._dp = object()                                                     # (the kind itself refuses world > 1 at construction)
    with pytest.raises(ValueError, match="_set_source.*data-parallel"):
        nn._set_source([0.0])
    assert nn._engine.calls == []
