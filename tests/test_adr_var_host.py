"""CPU: per-point coefficient fields of the adr kind (include/pinn_hip.h pinn_set_coef_fields, the PDE_ADR_VAR variants of
csrc/kernels_generic.h and csrc/kernels_fused20d.h, pinn_native.Engine.set_coef_fields, NeuralNetwork._set_coef_fields,
1d-mms/inf_cont_mms_var.py) without a device.

  * tests/helpers/adr_var_ref.py, the numpy restatement the GPU tests use: against torch autograd in float64 at the sibling
    host pins (1e-14 loss, 1e-13 gradient); with every row the constant set it IS adr_src_ref (bit for bit);
  * the test fields of tests/helpers/adr_var_cells.py move the loss of every GPU cell by at least 10 % against the
    constant-coefficient restatement, so no cell is vacuous;
  * 1d-mms/mmsutil.py: for every medium N_K[u*] - s = 0 with the derivatives of u* by torch autograd;
  * the symbol, its ctypes signature, the ABI version, the header text; the refusals of pinn_set_coef_fields that need no
    context (the array is checked first); Engine.set_coef_fields' and NeuralNetwork._set_coef_fields' behaviour and
    ValueErrors with the library stubbed out.  (A context needs a device to exist: those refusals are in
    tests/test_gpu_adr_var.py.)
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
import adr_var_cells as cells  # noqa: E402
import adr_var_ref  # noqa: E402

LB, UB = cells.LB, cells.UB


def rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300)


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


def _torch_loss_grad(w, layers, X_f, X_u, u, X_lo, X_hi, K, s, X_w, alpha, beta, g):
    import torch
    torch.set_num_threads(4)
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
    a0, a1, nu, r1, r2, r3 = (col(K[:, j]) for j in range(6))
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
    """N_f = 2048, n_0 = 512, 7 pairs, 33 Robin points, the test fields and the source of the GPU file; asserted at the
    sibling host pins, 1e-14 (loss) / 1e-13 (gradient, by its largest entry)"""
    base, rob = _sets()
    layers, co = cells.layers_of(depth), adr_ref.COEFF_SETS[name]
    w = _weights(layers)
    K, s = cells.fields_of(base[0], co), cells.source_of(base[0])
    lo, go, ex = adr_var_ref.var_loss_grad(w, layers, LB, UB, *base, K, s, *rob)
    lt, gt, ft = _torch_loss_grad(w, layers, *base, K, s, *rob)
    l0 = adr_src_ref.src_loss_grad(w, layers, LB, UB, *base, co, s, *rob)[0]
    print("adr_var_ref vs autograd %s depth %d: loss %.2e grad %.2e f %.2e | loss moved by %.0f %%" % (
        name, depth, abs(lo - lt) / abs(lt), rel(go, gt), rel(ex["f"], ft), 100 * abs(lo - l0) / l0))
    assert abs(lo - lt) / abs(lt) < 1e-14
    assert rel(go, gt) < 1e-13
    assert rel(ex["f"], ft) < 1e-13
    assert abs(lo - l0) / l0 > 0.1
    assert np.array_equal(ex["f"], adr_var_ref.residual(w, layers, LB, UB, base[0], K, s))


# ---- 2. constant rows: adr_src_ref itself --------------------------------------------------------------------------------
@pytest.mark.parametrize("with_source", [False, True])
@pytest.mark.parametrize("depth", [4, 8])
@pytest.mark.parametrize("name", sorted(adr_ref.COEFF_SETS))
def test_constant_rows_are_the_source_oracle_bit_for_bit(name, depth, with_source):
    base, rob = _sets()
    layers, co = cells.layers_of(depth), adr_ref.COEFF_SETS[name]
    w = _weights(layers)
    s = cells.source_of(base[0]) if with_source else None
    lo, go, ex = adr_src_ref.src_loss_grad(w, layers, LB, UB, *base, co, s, *rob)
    K = adr_var_ref.constant_rows(co, len(base[0]))
    assert K.shape == (2048, 6) and np.array_equal(K[17], np.asarray(co, dtype=np.float64))
    l1, g1, e1 = adr_var_ref.var_loss_grad(w, layers, LB, UB, *base, K, s, *rob)
    assert l1 == lo and np.array_equal(g1, go) and np.array_equal(e1["f"], ex["f"]) and np.array_equal(e1["r"], ex["r"])
    assert (e1["mse_f"], e1["mse_u"], e1["mse_b"], e1["mse_w"]) == (ex["mse_f"], ex["mse_u"], ex["mse_b"], ex["mse_w"])
    assert np.array_equal(adr_var_ref.residual(w, layers, LB, UB, base[0], K, s), adr_src_ref.residual(w, layers, LB, UB, base[0], co, s))
    with pytest.raises(ValueError, match="one row of six coefficients per collocation point"):
        adr_var_ref.var_loss_grad(w, layers, LB, UB, *base, K[:5], s)
    with pytest.raises(ValueError, match="one row of six coefficients per collocation point"):
        adr_var_ref.var_loss_grad(w, layers, LB, UB, *base, K[:, :5], s)


# ---- 3. no GPU cell is vacuous ------------------------------------------------------------------------------------------
def test_fields_are_distinct_in_every_column_and_keep_nu_positive():
    X_f = cells.point_sets(2048, 512, 50)[0]
    for name, co in adr_ref.COEFF_SETS.items():
        K = cells.fields_of(X_f, co)
        assert K.shape == (2048, 6) and np.all(np.isfinite(K)) and np.all(K[:, 2] > 0.0)
        assert len(np.unique(K.ravel())) == K.size, name          # distinct over points AND columns
        # no entry near its constant: |b (1 + 0.3 m) - c| >= 0.7 (|c| + 3) - |c| = 2.1 - 0.3 |c| >= 0.6 for |c| <= 5
        assert np.min(np.abs(K - np.asarray(co, dtype=np.float64))) >= 0.6 - 1e-12


@pytest.mark.parametrize("cell", cells.all_cells(), ids=lambda c: c[0])
def test_fields_move_the_loss_of_every_gpu_cell_by_ten_percent(cell):
    lo, lc = cells.reference(*cell[1:])[0], cells.constant_loss(*cell[1:])
    print("%s: loss with the fields %.6e, with the constant set %.6e: moved by %.1f %%" % (cell[0], lo, lc, 100 * abs(lo - lc) / lc))
    assert abs(lo - lc) / lc >= 0.10


def test_cells_cover_the_blocks_offsets_and_robin_counts():
    assert sorted(cells.OFFSETS) == [0, 1, 14, 15, 50, 64]
    assert all(2 * n_b + n_0 == off for off, (n_b, n_0) in cells.OFFSETS.items())
    assert cells.BLOCKS == (1, 15, 16, 17, 64, 2048)
    assert len(cells.alignment_cells()) == 36 and len(cells.variant_cells()) == 6
    assert sorted({c[6] for c in cells.robin_cells()}) == [0, 1, 50] and {c[7] for c in cells.robin_cells()} == {True, False}
    assert [c[2] for c in cells.equation_cells()] == sorted(adr_ref.COEFF_SETS)


# ---- 4. mmsutil -------------------------------------------------------------------------------------------------------------
def test_mms_media_are_the_named_three():
    import mmsutil as mu
    assert mu.MEDIA == ("graded_rod", "shear_flow", "graded_reaction")
    with pytest.raises(ValueError, match="medium"):
        mu.medium_fields(np.zeros((1, 2)), "porous")
    X = np.array([[-1.0, 0.0], [0.0, 0.5], [0.25, 1.0], [1.0, 0.3]])
    x, t = X[:, 0], X[:, 1]
    K = mu.medium_fields(X, "graded_rod")
    assert np.allclose(K[:, 2], 0.1 * (1.0 + 0.8 * np.tanh(8.0 * x)), rtol=0, atol=1e-16) and np.all(K[:, 2] > 0)
    assert np.all(K[:, [1, 3, 4, 5]] == 0.0)
    # a0 = -nu'(x): the conservative form; nu' by a central difference of nu itself
    h = 1e-6
    dnu = (mu.medium_fields(X + [h, 0], "graded_rod")[:, 2] - mu.medium_fields(X - [h, 0], "graded_rod")[:, 2]) / (2 * h)
    assert np.max(np.abs(K[:, 0] + dnu)) < 1e-9
    K = mu.medium_fields(X, "shear_flow")
    assert np.array_equal(K[:, 0], 0.7 + 0.3 * np.sin(np.pi * x) * np.cos(np.pi * t)) and np.all(K[:, 2] == 0.05)
    assert np.all(K[:, [1, 3, 4, 5]] == 0.0)
    K = mu.medium_fields(X, "graded_reaction")
    assert np.array_equal(K[:, 3], -5.0 * (1.0 + 0.5 * x)) and np.all(K[:, 5] == 5.0) and np.all(K[:, 2] == 1e-4)
    assert np.all(K[:, [0, 1, 4]] == 0.0)
    with pytest.raises(ValueError, match="one row of six"):
        mu.source_var(X, K[:3])


@pytest.mark.parametrize("medium", ["graded_rod", "shear_flow", "graded_reaction"])
def test_mms_variable_coefficient_source_is_the_operator_on_the_exact_field(medium):
    """N_K[u*] - s = 0 to 1e-12 (relative to the values, O(10)), the derivatives of u* by torch autograd; for the rod also in
    its conservative form, u_t - (nu u_x)_x with nu(x) differentiated by autograd"""
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
    u_xx = torch.autograd.grad(u_x, x, ones, create_graph=True)[0]
    K = mu.medium_fields(X, medium)
    a0, a1, nu, r1, r2, r3 = (torch.tensor(K[:, j]) for j in range(6))
    ref = (u_t + (a0 + a1 * u) * u_x - nu * u_xx + r1 * u + r2 * u ** 2 + r3 * u ** 3).detach().numpy()
    s = mu.source_var(X, K)
    assert s.shape == (500,)
    scale = max(1.0, np.max(np.abs(ref)))
    assert np.max(np.abs(ref - s)) < 1e-12 * scale
    if medium == "graded_rod":
        nu_t = 0.1 * (1.0 + 0.8 * torch.tanh(8.0 * x))
        flux_x = torch.autograd.grad(nu_t * u_x, x, ones)[0]
        cons = (u_t - flux_x).detach().numpy()
        assert np.max(np.abs(cons - s)) < 1e-12 * scale
    # and with constant rows it is the constant-coefficient source
    co = mu.adr_coeffs("fisher_kpp")
    assert np.array_equal(mu.source_var(X, adr_var_ref.constant_rows(co, 500)), mu.source(X, co))


# ---- 5. the C surface --------------------------------------------------------------------------------------------------
def test_coef_fields_symbol_is_declared_exported_and_typed():
    import pinn_native
    lib = pinn_native.load()
    header = open(os.path.join(ROOT, "include", "pinn_hip.h")).read()
    proto = re.search(r"\bint\s+pinn_set_coef_fields\s*\(([^)]*)\)\s*;", header)
    assert proto, "pinn_set_coef_fields is not declared"
    assert "pinn_set_coef_fields" in pinn_native.exported_symbols()
    res, args = pinn_native._SIGNATURES["pinn_set_coef_fields"]
    fn = lib.pinn_set_coef_fields
    assert fn.restype is res is ctypes.c_int and list(fn.argtypes) == list(args)
    assert list(args) == [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.c_int64]
    assert len([a for a in proto.group(1).split(",") if a.strip()]) == 3
    assert lib.pinn_abi_version() == 6
    # the block stands behind pinn_set_source and says what the issue fixes
    text = header[header.index("int pinn_set_source"):header.index("int pinn_set_coef_fields")]
    assert "Coefficient fields of the adr kind" in text and "the ABI version stays 6" in text
    for phrase in ("PINN_ESTATE", "pinn_get_collocation still works", "pinn_residual_at returns", "not known at foreign points",
                   "pinn_rad_collocation is refused", "bit-identical", "count again after removal", "names both",
                   "-(nu(x) u_x)_x"):
        assert phrase in text, phrase
    # the source's block is where tests/test_adr_source_host.py slices it
    assert "Source term of the adr kind" in header[header.index("int pinn_robin_residual"):header.index("int pinn_set_source")]


def _arr(*v):
    return (ctypes.c_double * len(v))(*v)


def test_set_coef_fields_refuses_bad_arguments_before_it_looks_at_the_context():
    """pinn_set_coef_fields checks its array first (it needs no context), so these refusals are reached without a device; each
    is PINN_EINVAL and pinn_last_error names pinn_set_coef_fields"""
    import pinn_native
    lib = pinn_native.load()
    good = [0.1, 0.2, 0.3, 0.4, 0.5, 0.6]
    cases = [
        ((None, 3), b"null array"),
        ((_arr(*good), -1), b"bad count"),
        ((None, -2), b"bad count"),
        ((_arr(*(good + [0.0, np.nan, 1.0, 0.0, 0.0, 0.0])), 2), b"coefficient 1 of row 1 is not finite"),
        ((_arr(np.inf, 0.0, 0.1, 0.0, 0.0, 0.0), 1), b"coefficient 0 of row 0 is not finite"),
        ((_arr(0.0, 0.0, 0.1, 0.0, 0.0, -np.inf), 1), b"coefficient 5 of row 0 is not finite"),
    ]
    for args, why in cases:
        assert lib.pinn_set_coef_fields(None, *args) == -1                    # PINN_EINVAL
        err = lib.pinn_last_error()
        assert why in err and b"pinn_set_coef_fields" in err, (why, err)
    # a good table, or the removal: the null context is what is left to refuse
    assert lib.pinn_set_coef_fields(None, _arr(*good), 1) == -1 and b"pinn_set_coef_fields: null context" in lib.pinn_last_error()
    assert lib.pinn_set_coef_fields(None, None, 0) == -1 and b"pinn_set_coef_fields: null context" in lib.pinn_last_error()


# ---- 6. Engine.set_coef_fields, library stubbed ----------------------------------------------------------------------------
class _Lib(object):
    def __init__(self):
        self.seen = []

    def pinn_set_coef_fields(self, h, K, n):
        self.seen.append((n, None if K is None else [K[i] for i in range(6 * n)]))
        return 0


def _stub_engine(n_f=2):
    import pinn_native
    eng = pinn_native.Engine.__new__(pinn_native.Engine)
    eng._lib, eng._h, eng.n_u, eng.n_f, eng.n_b, eng.n_w, eng.n_out = _Lib(), None, 0, n_f, 0, 0, 1
    return eng


def test_engine_set_coef_fields_passes_rows_and_tracks_has_coef_fields():
    eng = _stub_engine()
    assert eng.has_coef_fields is False
    K = [[1.0, 2.0, 3.0, 4.0, 5.0, 6.0], [7.0, 8.0, 9.0, 10.0, 11.0, 12.0]]
    eng.set_coef_fields(K)
    assert eng._lib.seen[-1] == (2, [float(v) for v in range(1, 13)]) and eng.has_coef_fields is True
    eng.set_coef_fields(np.asfortranarray(np.array(K)))                  # row-major is what the library gets
    assert eng._lib.seen[-1] == (2, [float(v) for v in range(1, 13)])
    eng.set_coef_fields(None)
    assert eng._lib.seen[-1] == (0, None) and eng.has_coef_fields is False


@pytest.mark.parametrize("K, match", [
    (np.zeros((2, 5)), r"\[n_f, 6\]"),
    (np.zeros(12), r"\[n_f, 6\]"),
    (np.zeros((6, 2)), r"\[n_f, 6\]"),
    (np.zeros((2, 6, 1)), r"\[n_f, 6\]"),
    (np.zeros((3, 6)), "one row per collocation point"),
    (np.zeros((1, 6)), "one row per collocation point"),
    ([[0.0, np.nan, 0.0, 0.0, 0.0, 0.0]] * 2, "finite"),
    ([[0.0, 0.0, 0.0, 0.0, 0.0, np.inf]] * 2, "finite"),
])
def test_engine_set_coef_fields_raises_value_errors_before_any_library_call(K, match):
    eng = _stub_engine()
    with pytest.raises(ValueError, match=match):
        eng.set_coef_fields(K)
    assert eng._lib.seen == [] and eng.has_coef_fields is False
    with pytest.raises(ValueError, match="empty"):
        _stub_engine(0).set_coef_fields(np.zeros((0, 6)))


# ---- 7. NeuralNetwork._set_coef_fields, engine stubbed ----------------------------------------------------------------------
CONST = [0.3, -0.8, 0.02, 0.6, -0.4, 1.5]


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
    def get_pde_params(self): return np.array(CONST)
    def set_collocation(self, X, n_total=None): self.X = np.array(X); self.n_f = len(X)
    def get_collocation(self): return self.X.copy()
    def set_source(self, s): self.calls.append(("source", None if s is None else np.array(s, dtype=np.float64)))
    def set_coef_fields(self, K): self.calls.append(("fields", None if K is None else np.array(K, dtype=np.float64)))


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


X3 = np.array([[0.0, 0.1], [0.5, 0.2], [-0.5, 0.3]])


def _rows(P):
    return np.column_stack([P[:, 0] + j + 10.0 * P[:, 1] for j in range(6)])


def test_neuralnetwork_set_coef_fields_takes_an_array_a_callable_or_a_dict(monkeypatch):
    nn = _nn(monkeypatch, "adr")
    nn._set_collocation(X3)
    K = np.arange(18.0).reshape(3, 6)
    nn._set_coef_fields(K)
    assert nn._engine.calls[-1][0] == "fields" and np.array_equal(nn._engine.calls[-1][1], K)
    nn._set_coef_fields(_rows)                                            # evaluated at the engine's own points
    assert np.array_equal(nn._engine.calls[-1][1], _rows(X3))
    # a dict: the named columns, the others the model's constants
    nn._set_coef_fields({"nu": [0.1, 0.2, 0.3], "a0": lambda P: -P[:, 0]})
    want = np.tile(CONST, (3, 1))
    want[:, 2] = [0.1, 0.2, 0.3]
    want[:, 0] = -X3[:, 0]
    assert np.array_equal(nn._engine.calls[-1][1], want)
    nn._set_coef_fields({"r3": np.array([[5.0], [6.0], [7.0]])})          # a column [n, 1] is taken as [n]
    want = np.tile(CONST, (3, 1))
    want[:, 5] = [5.0, 6.0, 7.0]
    assert np.array_equal(nn._engine.calls[-1][1], want)
    nn._set_coef_fields({})                                               # nothing named: constant rows
    assert np.array_equal(nn._engine.calls[-1][1], np.tile(CONST, (3, 1)))
    with pytest.raises(ValueError, match="_set_coef_fields: column 'nu' must hold one value per collocation point \\(3\\), got 2"):
        nn._set_coef_fields({"nu": [0.1, 0.2]})
    n_calls = len(nn._engine.calls)
    nn._set_coef_fields(None)
    assert nn._engine.calls[-1] == ("fields", None) and len(nn._engine.calls) == n_calls + 1


def test_neuralnetwork_callables_follow_redraws_and_arrays_do_not(monkeypatch):
    X_new = np.array([[0.9, 0.9], [0.8, 0.8], [0.7, 0.7]])
    # a callable, with a callable source: both are set again at the new points, from one get_collocation
    nn = _nn(monkeypatch, "adr", resample_every=10)
    nn._set_collocation(X3)
    nn._set_coef_fields(_rows)
    nn._set_source(lambda P: P[:, 0])
    nn._engine.X, nn._engine.calls = X_new, []
    nn._follow_redraw()
    assert [c[0] for c in nn._engine.calls] == ["source", "fields"]
    assert np.array_equal(nn._engine.calls[0][1], X_new[:, 0]) and np.array_equal(nn._engine.calls[1][1], _rows(X_new))
    # a dict with a callable follows; the constants are read again
    nn = _nn(monkeypatch, "adr", resample_every=10)
    nn._set_collocation(X3)
    nn._set_coef_fields({"a0": lambda P: 2.0 * P[:, 1]})
    nn._engine.X, nn._engine.calls = X_new, []
    nn._follow_redraw()
    want = np.tile(CONST, (3, 1))
    want[:, 0] = 2.0 * X_new[:, 1]
    assert len(nn._engine.calls) == 1 and np.array_equal(nn._engine.calls[0][1], want)
    # an array, a dict of arrays, and removal: nothing follows
    for k in (np.zeros((3, 6)), {"nu": [0.1, 0.2, 0.3]}, None):
        nn = _nn(monkeypatch, "adr")
        nn._set_collocation(X3)
        nn._set_coef_fields(_rows)
        nn._set_coef_fields(k)
        nn._engine.calls = []
        nn._follow_redraw()
        assert nn._engine.calls == []


@pytest.mark.parametrize("pde, kw, k, match", [
    ("burgers", {}, np.zeros((1, 6)), "_set_coef_fields.*adr.*burgers"),
    ("adr_ide", {"adr_trainable": ["nu"]}, np.zeros((1, 6)), "_set_coef_fields.*adr.*adr_ide"),
    ("schrodinger", {"layers": [2, 20, 20, 2]}, np.zeros((1, 6)), "_set_coef_fields.*adr.*schrodinger"),
    ("adr", {"resample_every": 10, "resample": "rad"}, _rows, "_set_coef_fields.*rad"),
    ("adr", {"point_weights": True}, np.zeros((1, 6)), "_set_coef_fields.*point_weights"),
    ("adr", {"resample_every": 10}, np.zeros((1, 6)), "_set_coef_fields.*array.*resample_every"),
    ("adr", {"resample_every": 10}, {"nu": [0.1]}, "_set_coef_fields.*array.*resample_every"),
    ("adr", {"resample_every": 10}, {"nu": [0.1], "a0": (lambda P: P[:, 0])}, "_set_coef_fields.*array.*resample_every"),
    ("adr", {}, {"mu": [0.1]}, "_set_coef_fields: unknown coefficient 'mu'"),
    ("adr", {}, {"nu": [0.1], "r4": [0.1]}, "_set_coef_fields: unknown coefficient 'r4'"),
])
def test_neuralnetwork_set_coef_fields_refuses_by_name(monkeypatch, pde, kw, k, match):
    nn = _nn(monkeypatch, pde, **kw)
    with pytest.raises(ValueError, match=match):
        nn._set_coef_fields(k)
    assert nn._engine.calls == []


def test_neuralnetwork_set_coef_fields_refuses_a_data_parallel_launch(monkeypatch):
    nn = _nn(monkeypatch, "adr")
    nn._dp = object()                                                     # (the kind itself refuses world > 1 at construction)
    with pytest.raises(ValueError, match="_set_coef_fields.*data-parallel"):
        nn._set_coef_fields(np.zeros((1, 6)))
    assert nn._engine.calls == []
