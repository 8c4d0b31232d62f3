"""CPU: per-point loss weights of the adr kind (include/pinn_hip.h pinn_pw_*, k_fused20d<PDE_ADR, .., SAW> of csrc/kernels_fused20d.h,
pinn_native.Engine.pw_*, utils/neuralnetwork.py hp["point_weights"]) without a device.

  * tests/helpers/adr_pw_ref.py, the numpy restatement the GPU tests use: with unit weights it IS adr_ref.adr_loss_grad (bit for
    bit); against torch autograd in theta and in the three lambda classes (the tolerances tests/test_adr_host.py holds adr_ref
    to); central differences in single lambda entries;
  * the conditioning of the 50-step trajectory the GPU test follows to 1e-8: the same run with the rows of every class
    permuted (only the summation order changes) must stay within 1e-10;
  * _pw_options' acceptances and refusals, the four symbols and their ctypes signatures, the ABI version;
  * NeuralNetwork's start-value schedule and summary line with the engine stubbed out, the ensemble's refusal.
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
import adr_pw_ref  # noqa: E402
import adr_ref  # noqa: E402

LB, UB = adr_pw_ref.LB, adr_pw_ref.UB
PW_SYMBOLS = {"pinn_pw_set": 7, "pinn_pw_get": 7, "pinn_pw_adam_init": 4, "pinn_pw_disable": 1}


def rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300)


def _small(H, seed=5, n_f=300, n_u=60, n_b=40):
    c = adr_pw_ref.trajectory_case(H, seed=seed, n_f=n_f, n_u=n_u, n_b=n_b)
    return c, (c["w0"], c["layers"], LB, UB, c["X_f"], c["X_u"], c["u"], c["X_lo"], c["X_hi"])


# ---- the restatement --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [4, 8])
@pytest.mark.parametrize("name", ["allen_cahn", "all_nonzero"])
def test_unit_weights_are_the_plain_oracle_bit_for_bit(H, name):
    c, args = _small(H)
    co = adr_ref.COEFF_SETS[name]
    lo, go, ex = adr_ref.adr_loss_grad(*args, co)
    for lam in ((None, None, None), tuple(np.ones(len(c[k])) for k in ("lam_u", "lam_f", "lam_b"))):
        l1, g1, terms, _ = adr_pw_ref.loss_grad(*args, co, *lam)
        assert l1 == lo and np.array_equal(g1, go)
        assert terms == (ex["mse_f"], ex["mse_u"], ex["mse_b"])
    # empty data and boundary sets
    a2 = args[:5] + (None, None, None, None)
    lo, go, _ = adr_ref.adr_loss_grad(*a2, co)
    l1, g1, _, dl = adr_pw_ref.loss_grad(*a2, co)
    assert l1 == lo and np.array_equal(g1, go) and dl[0].size == 0 and dl[2].size == 0


def _torch_loss_grad(w, layers, X_f, X_u, u, X_lo, X_hi, coeffs, lam_u, lam_f, lam_b):
    import torch
    torch.set_num_threads(4)
    a0, a1, nu, r1, r2, r3 = coeffs
    wt = torch.tensor(w, dtype=torch.float64, requires_grad=True)
    lams = [torch.tensor(np.asarray(l).reshape(-1, 1), dtype=torch.float64, requires_grad=True) for l in (lam_u, lam_f, lam_b)]
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

    uu, u_x, u_t, u_xx = channels(X_f)
    f = u_t + (a0 + a1 * uu) * u_x - nu * u_xx + r1 * uu + r2 * uu ** 2 + r3 * uu ** 3
    loss = torch.mean((lams[1] * f) ** 2)
    loss = loss + torch.mean((lams[0] * (channels(X_u)[0] - torch.tensor(u))) ** 2)
    ul, ul_x, _, _ = channels(X_lo)
    uh, uh_x, _, _ = channels(X_hi)
    loss = loss + torch.mean((lams[2] * (ul - uh)) ** 2) + torch.mean((lams[2] * (ul_x - uh_x)) ** 2)
    loss.backward()
    return float(loss.detach()), wt.grad.numpy().copy(), [l.grad.numpy().ravel().copy() for l in lams]


@pytest.mark.parametrize("H", [4, 8])
@pytest.mark.parametrize("name", ["allen_cahn", "all_nonzero"])
def test_restatement_against_torch_autograd_in_theta_and_lambda(H, name):
    """asserted at test_adr_host.py's 1e-14 (loss) / 1e-13 (gradients, by their largest entry)"""
    c, args = _small(H)
    co = adr_ref.COEFF_SETS[name]
    lam = (c["lam_u"], c["lam_f"], c["lam_b"])
    lo, go, terms, dl = adr_pw_ref.loss_grad(*args, co, *lam)
    lt, gt, dlt = _torch_loss_grad(c["w0"], c["layers"], c["X_f"], c["X_u"], c["u"], c["X_lo"], c["X_hi"], co, *lam)
    print("adr_pw_ref vs autograd H=%d %s: loss %.2e theta %.2e lambda %s" % (
        H, name, abs(lo - lt) / abs(lt), rel(go, gt), ["%.2e" % rel(a, b) for a, b in zip(dl, dlt)]))
    assert min(terms) > 0 and abs(sum(terms) - lo) <= 1e-15 * lo
    assert abs(lo - lt) / abs(lt) < 1e-14
    assert rel(go, gt) < 1e-13
    for a, b in zip(dl, dlt):
        assert rel(a, b) < 1e-13


@pytest.mark.parametrize("H", [4, 8])
@pytest.mark.parametrize("name", ["allen_cahn", "all_nonzero"])
def test_lambda_gradient_against_central_differences(H, name):
    """L is quadratic in every lambda, so a central difference has no truncation error: what is left is the rounding of the two
    losses, <= 8 u L / h with h = 2^-10 (each loss a few u L off, their difference divided by 2 h)"""
    c, args = _small(H)
    co = adr_ref.COEFF_SETS[name]
    lam = [c["lam_u"], c["lam_f"], c["lam_b"]]
    L, _, _, dl = adr_pw_ref.loss_grad(*args, co, *lam)
    h, u_ = 2.0 ** -10, 2.0 ** -53
    bound = 8 * u_ * L / h
    worst = 0.0
    for k in range(3):
        for i in (0, 3, len(lam[k]) - 1):
            lp, lm = [x.copy() for x in lam], [x.copy() for x in lam]
            lp[k][i] += h
            lm[k][i] -= h
            fd = (adr_pw_ref.loss_only(*args, co, *lp) - adr_pw_ref.loss_only(*args, co, *lm)) / (2 * h)
            worst = max(worst, abs(fd - dl[k][i]))
            assert abs(fd - dl[k][i]) <= bound, (k, i, fd, dl[k][i], bound)
    print("central differences H=%d %s: worst %.2e, bound %.2e" % (H, name, worst, bound))


@pytest.mark.parametrize("H", [4, 8])
@pytest.mark.parametrize("name", ["allen_cahn", "all_nonzero"])
def test_trajectory_is_well_conditioned_under_row_permutations(H, name):
    """the GPU test follows this 50-step run to 1e-8; a device sums in another order than numpy, so the same run with every
    class's rows permuted must agree far inside that: 1e-10"""
    case = adr_pw_ref.trajectory_case(H)
    co = adr_ref.COEFF_SETS[name]
    w0, lam0, l0 = adr_pw_ref.run_trajectory(case, co)
    rs = np.random.RandomState(2)
    perm = [rs.permutation(len(case[k])) for k in ("lam_u", "lam_f", "lam_b")]
    w1, lam1, l1 = adr_pw_ref.run_trajectory(case, co, perm)
    dw = np.max(np.abs(w1 - w0))
    dlam = [np.max(np.abs(a - b)) for a, b in zip(lam1, lam0)]
    dl = np.max(np.abs(l1 - l0) / l0)
    moved = [np.max(np.abs(a - case[k])) for a, k in zip(lam0, ("lam_u", "lam_f", "lam_b"))]
    print("H=%d %s: theta %.1e lambda %s loss %.1e; moved %s" % (H, name, dw, ["%.1e" % d for d in dlam], dl,
                                                                ["%.2f" % m for m in moved]))
    assert dw <= 1e-10 and max(dlam) <= 1e-10 and dl <= 1e-10
    assert min(moved) > 1e-4


# ---- hp validation, no device -----------------------------------------------------------------------------------------
def _hp(**kw):
    hp = {"layers": [2, 20, 20, 20, 20, 1], "tf_epochs": 1, "tf_lr": 0.01, "tf_b1": 0.9, "tf_eps": None,
          "nt_epochs": 1, "nt_lr": 0.8, "nt_ncorr": 50, "log_frequency": 1}
    hp.update(kw)
    return hp


def test_pw_options_accepts():
    import neuralnetwork as nn
    assert nn._pw_options(_hp(), "adr") is None
    assert nn._pw_options(_hp(pw_init=[10, 1, 1]), "burgers") is None              # the switch is point_weights
    assert nn._pw_options(_hp(point_weights=True), "adr") == ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0))
    assert nn._pw_options(_hp(point_weights=True, pw_init=[10, 1, 1], pw_lr=[0, 0.01, 0]), "adr") == (
        (10.0, 1.0, 1.0), (0.0, 0.01, 0.0))
    assert nn._pw_options(_hp(point_weights=True, pw_init=2, pw_lr=0.5), "adr") == ((2.0, 2.0, 2.0), (0.5, 0.5, 0.5))
    for depth in (4, 6, 8):                                                         # the depths of kernel path 7
        assert nn._pw_options(_hp(point_weights=True, layers=[2] + [20] * depth + [1]), "adr") is not None
    # redraws go with a plain collocation class
    assert nn._pw_options(_hp(point_weights=True, pw_init=[10, 1, 3], pw_lr=[0.1, 0, 0.1], resample_every=10,
                              resample="rad"), "adr") == ((10.0, 1.0, 3.0), (0.1, 0.0, 0.1))


@pytest.mark.parametrize("kw, pde, match", [
    ({}, "burgers", "point_weights.*burgers"),
    ({}, "adr_ide", "point_weights.*adr_ide"),
    ({}, "schrodinger", "point_weights.*schrodinger"),
    ({"dtype": "f32"}, "adr", "point_weights.*dtype"),
    ({"sa_weights": True}, "adr", "point_weights.*sa_weights"),
    ({"resample_every": 10, "pw_init": [1, 2, 1]}, "adr", "point_weights.*resample"),
    ({"resample_every": 10, "resample": "rad", "pw_lr": [0, 0.01, 0]}, "adr", "point_weights.*resample"),
    ({"resample_every": 10, "pw_lr": 0.01}, "adr", "point_weights.*resample"),
    # layers the float64 width-20 kernel (path 7) does not take: another width, another depth, two outputs
    ({"layers": [2, 32, 32, 32, 32, 1]}, "adr", "point_weights.*layers"),
    ({"layers": [2, 20, 20, 20, 20, 20, 1]}, "adr", "point_weights.*layers"),
    ({"layers": [2, 20, 20, 1]}, "adr", "point_weights.*layers"),
    ({"layers": [2, 20, 20, 20, 30, 1]}, "adr", "point_weights.*layers"),
    ({"layers": [2, 20, 20, 20, 20, 2]}, "adr", "point_weights.*layers"),
    ({"pw_init": [1, 2]}, "adr", "pw_init"),
    ({"pw_init": "big"}, "adr", "pw_init"),
    ({"pw_init": [1, float("nan"), 1]}, "adr", "pw_init"),
    ({"pw_lr": [0, -0.1, 0]}, "adr", "pw_lr"),
    ({"pw_lr": [0, float("inf"), 0]}, "adr", "pw_lr"),
    ({"pw_lr": True}, "adr", "pw_lr"),
])
def test_pw_options_refuses_with_the_key_named(kw, pde, match):
    import neuralnetwork as nn
    with pytest.raises(ValueError, match=match):
        nn._pw_options(_hp(point_weights=True, **kw), pde)


def test_sa_weights_with_adr_keeps_its_own_refusal():
    import neuralnetwork as nn
    with pytest.raises(ValueError, match="sa_weights.*adr"):
        nn._sa_options(_hp(sa_weights=True, point_weights=True), "adr")


# ---- the C surface ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PW_SYMBOLS))
def test_pw_symbols_are_declared_exported_and_typed(name):
    import pinn_native
    lib = pinn_native.load()
    header = open(os.path.join(ROOT, "include", "pinn_hip.h")).read()
    proto = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header)
    assert proto, "%s is not declared" % name
    assert name in pinn_native.exported_symbols()
    res, args = pinn_native._SIGNATURES[name]
    fn = getattr(lib, name)
    assert fn.restype is res is ctypes.c_int and list(fn.argtypes) == list(args)
    assert len([a for a in proto.group(1).split(",") if a.strip()]) == len(args) == PW_SYMBOLS[name]
    assert lib.pinn_abi_version() == 6


def test_pw_calls_refuse_a_null_context_and_the_engine_has_the_wrappers():
    import pinn_native
    lib = pinn_native.load()
    one = (ctypes.c_double * 1)(1.0)
    assert lib.pinn_pw_set(None, one, 1, one, 1, one, 1) == -1          # PINN_EINVAL
    assert lib.pinn_pw_get(None, one, 1, one, 1, one, 1) == -1
    assert lib.pinn_pw_adam_init(None, 0.0, 0.01, 0.0) == -1
    assert lib.pinn_pw_disable(None) == -1
    for m in ("pw_set", "pw_get", "pw_adam_init", "pw_disable"):
        assert hasattr(pinn_native.Engine, m)


def test_engine_wrappers_pass_the_arguments_through():
    import pinn_native
    seen = []

    class _Lib(object):
        def pinn_pw_set(self, h, pu, nu_, pf, nf, pb, nb):
            seen.append(("set", nu_, nf, nb, pu is None, pf[nf - 1], pb[0]))
            return 0

        def pinn_pw_adam_init(self, h, ru, rf, rb):
            seen.append(("rates", ru, rf, rb))
            return 0

        def pinn_pw_disable(self, h):
            seen.append(("off",))
            return 0

    eng = pinn_native.Engine.__new__(pinn_native.Engine)
    eng._lib, eng._h, eng.n_u, eng.n_f, eng.n_b = _Lib(), None, 3, 5, 2
    eng.pw_set(None, np.arange(5.0), [7.0, 8.0])
    eng.pw_adam_init(0.05, 0.02)
    eng.pw_disable()
    assert seen == [("set", 3, 5, 2, True, 4.0, 7.0), ("rates", 0.05, 0.02, 0.0), ("off",)]


# ---- NeuralNetwork wiring, engine stubbed ------------------------------------------------------------------------------
class _Engine(object):
    """records the set, weight and optimiser calls of NeuralNetwork"""

    def __init__(self, layers, lb, ub, pde="burgers", dtype="f64", device=0):
        self.n_params, self.w, self.calls, self.pde = 5, np.zeros(5), [], pde
        self.n_f = self.n_u = self.n_b = 0
        self.lb_total = self.lb_done = 0

    def set_weights(self, w): self.w = np.array(w, dtype=np.float64)
    def get_weights(self): return self.w.copy()
    def adam_init(self, *a): self.calls.append(("adam_init",))
    def set_data(self, X, u, n_total=None): self.n_u = len(X); self.calls.append(("data", len(X)))
    def set_collocation(self, X, n_total=None): self.n_f = len(X); self.calls.append(("colloc", len(X)))
    def set_boundary(self, lo, hi, n_total=None): self.n_b = len(lo); self.calls.append(("pairs", len(lo)))
    def set_pde_params(self, *p): pass
    def status(self): return 0, 0
    def adam_run(self, n, want_losses=True): self.calls.append(("adam", n)); return np.ones(n)
    def adam_enqueue(self, n): self.calls.append(("adam", n)); return n
    def adam_collect(self, ticket): return np.ones(ticket)
    def lbfgs_begin(self, n, *a): self.calls.append(("lbfgs_begin", n)); self.lb_total, self.lb_done = n, 0

    def lbfgs_run(self, n):
        self.calls.append(("lbfgs", n))
        k = min(n, self.lb_total - self.lb_done)
        its = np.arange(self.lb_done + 1, self.lb_done + k + 1, dtype=np.int32)
        self.lb_done += k
        return its, np.ones(k), int(self.lb_done >= self.lb_total)

    def lbfgs_enqueue(self, n): return self.lbfgs_run(n)
    def lbfgs_collect(self, r): return r
    def weights_snapshot(self, slot): pass
    def pw_adam_init(self, *r): self.calls.append(("pw_rates",) + r)

    def pw_set(self, lam_u, lam_f, lam_b):
        self.calls.append(("pw_set",) + tuple((len(l), set(np.asarray(l).tolist())) for l in (lam_u, lam_f, lam_b)))

    def pw_get(self): return np.full(self.n_u, 10.0), np.linspace(1.0, 3.0, self.n_f), np.ones(self.n_b)


def _fit(monkeypatch, capsys, hp, n_f=1000, n_u=4, n_b=3):
    import neuralnetwork
    from logger import Logger
    monkeypatch.setattr(neuralnetwork, "Engine", _Engine)
    hp = _hp(tf_epochs=35, nt_epochs=12, log_frequency=10, **hp)
    nn = neuralnetwork.NeuralNetwork(hp, Logger(hp), UB, LB, pde="adr")
    nn._set_collocation(np.zeros((n_f, 2)))
    nn._set_boundary(np.zeros((n_b, 2)), np.ones((n_b, 2)))
    nn.logger.set_error_fn(lambda: 0.5)
    nn.fit(np.arange(2.0 * n_u).reshape(n_u, 2), np.zeros((n_u, 1)))
    return nn, nn._engine.calls, capsys.readouterr().out


@pytest.mark.parametrize("async_log", [False, True])
def test_start_values_are_applied_once_after_the_sets_and_before_adam(monkeypatch, capsys, async_log):
    nn, calls, out = _fit(monkeypatch, capsys, dict(point_weights=True, pw_init=[10, 1, 1], pw_lr=[0, 0.01, 0],
                                                      async_log=async_log))
    names = [c[0] for c in calls]
    assert names.count("pw_set") == 1 and names.count("data") == 1
    assert max(names.index(k) for k in ("data", "colloc", "pairs")) < names.index("pw_set") < names.index("adam") \
        < names.index("lbfgs_begin")
    assert calls[names.index("pw_set")] == ("pw_set", (4, {10.0}), (1000, {1.0}), (3, {1.0}))
    assert ("pw_rates", 0.0, 0.01, 0.0) in calls and names.index("pw_rates") < names.index("pw_set")
    lam = nn.get_point_weights()
    assert [l.shape for l in lam] == [(4,), (1000,), (3,)]
    lines = [l for l in out.splitlines() if l.startswith("Point weights:")]
    assert len(lines) == 1 and "data min 1.0000e+01" in lines[0] and "collocation min 1.0000e+00 median 2.0000e+00" in lines[0]
    assert out.index("Training finished") < out.index("Point weights:")


def test_point_weights_default_off(monkeypatch, capsys):
    nn, calls, out = _fit(monkeypatch, capsys, {})
    assert not any(c[0].startswith("pw_") for c in calls) and "Point weights:" not in out
    with pytest.raises(ValueError, match="point_weights"):
        nn.get_point_weights()


def test_ensemble_refuses_point_weights(monkeypatch):
    import ensemble

    def _no_engine(*a, **k):
        raise AssertionError("an engine was made")

    monkeypatch.setattr(ensemble, "Ensemble", _no_engine)
    with pytest.raises(ValueError, match="point_weights"):
        ensemble.NeuralNetworkEnsemble(_hp(point_weights=True), None, [1.0, 1.0], [-1.0, 0.0], [{}, {}])
