"""CPU: self-adaptive point weights (include/pinn_hip.h pinn_sa_*, the SAW variants of csrc/kernels_fused20d.h,
pinn_native.Engine.sa_*, utils/neuralnetwork.py hp["sa_weights"]) -- the exported symbols and their ctypes signatures, the
null-context refusal, the numpy restatement (tests/helpers/sa_ref.py) against finite differences, and NeuralNetwork's
start-value schedule and hp refusals with the engine stubbed out."""
import contextlib
import ctypes
import io
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import sa_ref  # noqa: E402

SA_SYMBOLS = {"pinn_sa_set_weights": 5, "pinn_sa_get_weights": 5, "pinn_sa_adam_init": 2, "pinn_sa_disable": 1}


def _utils():
    p = os.path.join(ROOT, "pinns-tf2.0_amd", "utils")
    if p not in sys.path:
        sys.path.insert(0, p)


# ---- the C surface ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SA_SYMBOLS))
def test_sa_symbols_are_declared_exported_and_typed(name):
    import pinn_native
    lib = pinn_native.load()
    header = open(os.path.join(ROOT, "include", "pinn_hip.h")).read()
    proto = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header)
    assert proto, "%s is not declared" % name
    assert name in pinn_native.exported_symbols()
    res, args = pinn_native._SIGNATURES[name]
    fn = getattr(lib, name)
    assert fn.restype is res is ctypes.c_int and list(fn.argtypes) == list(args)
    assert len([a for a in proto.group(1).split(",") if a.strip()]) == len(args) == SA_SYMBOLS[name]
    assert lib.pinn_abi_version() == 6


def test_sa_calls_refuse_a_null_context():
    import pinn_native
    lib = pinn_native.load()
    one = (ctypes.c_double * 1)(1.0)
    assert lib.pinn_sa_set_weights(None, one, 1, one, 1) == -1          # PINN_EINVAL
    assert lib.pinn_sa_get_weights(None, one, 1, one, 1) == -1
    assert lib.pinn_sa_adam_init(None, 0.01) == -1
    assert lib.pinn_sa_disable(None) == -1
    for m in ("sa_set_weights", "sa_get_weights", "sa_adam_init", "sa_disable"):
        assert hasattr(pinn_native.Engine, m)


def test_engine_wrappers_pass_the_arguments_through():
    import pinn_native
    seen = []

    class _Lib(object):
        def pinn_sa_set_weights(self, h, pu, nu_, pf, nf):
            seen.append(("set", nu_, nf, pu[0], pf[nf - 1]))
            return 0

        def pinn_sa_adam_init(self, h, lr):
            seen.append(("lr", lr))
            return 0

        def pinn_sa_disable(self, h):
            seen.append(("off",))
            return 0

    eng = pinn_native.Engine.__new__(pinn_native.Engine)
    eng._lib, eng._h, eng.n_u, eng.n_f = _Lib(), None, 3, 5
    eng.sa_set_weights([2.0, 1.0, 1.0], np.arange(5.0))
    eng.sa_adam_init(0.005)
    eng.sa_disable()
    assert seen == [("set", 3, 5, 2.0, 4.0), ("lr", 0.005), ("off",)]


# ---- the restatement --------------------------------------------------------------------------------------------------
def _problem(rs, n_f=40, n_u=12, layers=(2, 5, 5, 1)):
    from oracle import init
    layers = list(layers)
    lb, ub = np.array([-1.0, 0.0]), np.array([1.0, 0.99])
    X_f = np.column_stack([rs.uniform(-1, 1, n_f), rs.uniform(0, 0.99, n_f)])
    X_u = np.column_stack([rs.uniform(-1, 1, n_u), rs.uniform(0, 0.99, n_u)])
    u = np.sin(np.pi * X_u[:, :1])
    return layers, lb, ub, X_f, X_u, u, init.glorot_flat(layers)


def test_restatement_lambda_gradient_matches_finite_differences():
    rs = np.random.RandomState(3)
    layers, lb, ub, X_f, X_u, u, w = _problem(rs)
    nu = 0.01 / np.pi
    lam_u, lam_f = rs.uniform(0.5, 2.0, X_u.shape[0]), rs.uniform(0.5, 2.0, X_f.shape[0])
    _, _, _, gu, gf = sa_ref.loss_grad(w, layers, lb, ub, X_f, X_u, u, nu, lam_u, lam_f)
    h = 1e-6
    for k, (lam, g) in enumerate(((lam_u, gu), (lam_f, gf))):
        for i in (0, 3, len(lam) - 1):
            lp, lm = lam.copy(), lam.copy()
            lp[i] += h
            lm[i] -= h
            args = (lp, lam_f) if k == 0 else (lam_u, lp)
            argm = (lm, lam_f) if k == 0 else (lam_u, lm)
            fd = (sa_ref.loss_only(w, layers, lb, ub, X_f, X_u, u, nu, *args) -
                  sa_ref.loss_only(w, layers, lb, ub, X_f, X_u, u, nu, *argm)) / (2 * h)
            assert abs(fd - g[i]) <= 1e-6 * abs(g[i]) + 1e-12


def test_restatement_with_unit_weights_is_the_oracle_loss():
    from oracle import pde
    rs = np.random.RandomState(4)
    layers, lb, ub, X_f, X_u, u, w = _problem(rs)
    nu = 0.01 / np.pi
    lo, go, _ = pde.burgers_loss_grad(w, layers, lb, ub, X_f, X_u, u, nu)
    l1, g1, _, _, _ = sa_ref.loss_grad(w, layers, lb, ub, X_f, X_u, u, nu, np.ones(X_u.shape[0]), np.ones(X_f.shape[0]))
    assert abs(l1 - lo) <= 1e-14 * lo and np.max(np.abs(g1 - go)) <= 1e-14 * np.max(np.abs(go))
    # theta gradient against finite differences at random weights
    lam_u, lam_f = rs.uniform(0.5, 2.0, X_u.shape[0]), rs.uniform(0.5, 2.0, X_f.shape[0])
    _, g, _, _, _ = sa_ref.loss_grad(w, layers, lb, ub, X_f, X_u, u, nu, lam_u, lam_f)
    for i in (0, 7, len(w) - 1):
        wp, wm = w.copy(), w.copy()
        wp[i] += 1e-6
        wm[i] -= 1e-6
        fd = (sa_ref.loss_only(wp, layers, lb, ub, X_f, X_u, u, nu, lam_u, lam_f) -
              sa_ref.loss_only(wm, layers, lb, ub, X_f, X_u, u, nu, lam_u, lam_f)) / 2e-6
        assert abs(fd - g[i]) <= 1e-6 * abs(g[i]) + 1e-10


def test_restatement_ascends_in_the_weights():
    rs = np.random.RandomState(5)
    layers, lb, ub, X_f, X_u, u, w = _problem(rs)
    lam_u, lam_f = np.ones(X_u.shape[0]), np.ones(X_f.shape[0])
    _, lu, lf, _ = sa_ref.adam(w, lam_u, lam_f, 5, layers, lb, ub, X_f, X_u, u, 0.01 / np.pi, 1e-3, 0.1)
    assert np.all(lu >= 1.0) and np.all(lf >= 1.0) and lf.max() > 1.0
    _, lu0, lf0, _ = sa_ref.adam(w, lam_u, lam_f, 5, layers, lb, ub, X_f, X_u, u, 0.01 / np.pi, 1e-3, 0.0)
    assert np.array_equal(lu0, lam_u) and np.array_equal(lf0, lam_f)


# ---- NeuralNetwork wiring, engine stubbed ------------------------------------------------------------------------------
class _Engine(object):
    """records the set, weight and optimiser calls of NeuralNetwork"""
    log = None

    def __init__(self, layers, lb, ub, pde="burgers", dtype="f64", device=0):
        self.n_params, self.w, self.calls = 5, np.zeros(5), []
        self.n_f = self.n_u = self.n_b = 0
        self.lb_total = self.lb_done = 0
        type(self).log = self.calls

    def set_weights(self, w): self.w = np.array(w, dtype=np.float64)
    def get_weights(self): return self.w.copy()
    def adam_init(self, *a): self.calls.append(("adam_init",))
    def set_data(self, X, u, n_total=None): self.n_u = len(X); self.calls.append(("data", len(X)))
    def set_collocation(self, X, n_total=None): self.n_f = len(X); self.calls.append(("colloc", len(X)))
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
    def sa_adam_init(self, lr): self.calls.append(("sa_lr", lr))

    def sa_set_weights(self, lam_u, lam_f):
        self.calls.append(("sa_set", len(lam_u), len(lam_f), set(np.asarray(lam_u).tolist()),
                           set(np.asarray(lam_f).tolist())))

    def sa_get_weights(self): return np.ones(self.n_u), np.ones(self.n_f)


def _hp(**kw):
    return dict({"layers": [2, 1], "tf_epochs": 35, "tf_lr": 0.03, "tf_b1": 0.9, "tf_eps": None, "nt_epochs": 12,
                 "nt_lr": 0.8, "nt_ncorr": 50, "log_frequency": 10, "async_log": False}, **kw)


def _run(monkeypatch, hp, n_f=1000, n_u=4):
    _utils()
    import neuralnetwork
    from logger import Logger
    monkeypatch.setattr(neuralnetwork, "Engine", _Engine)
    with contextlib.redirect_stdout(io.StringIO()):
        nn = neuralnetwork.NeuralNetwork(hp, Logger(hp), [1.0, 1.0], [-1.0, 0.0])
        nn._set_collocation(np.zeros((n_f, 2)))
        nn.logger.set_error_fn(lambda: 0.5)
        nn.fit(np.arange(2.0 * n_u).reshape(n_u, 2), np.zeros((n_u, 1)))
    return nn, nn._engine.calls


@pytest.mark.parametrize("async_log", [False, True])
def test_start_values_are_applied_once_after_the_data_and_before_adam(monkeypatch, async_log):
    nn, calls = _run(monkeypatch, _hp(sa_weights=True, sa_init=[2.5, 0.75], async_log=async_log))
    names = [c[0] for c in calls]
    assert names.count("sa_set") == 1 and names.count("data") == 1
    assert names.index("data") < names.index("sa_set") < names.index("adam") < names.index("lbfgs_begin")
    assert calls[names.index("sa_set")] == ("sa_set", 4, 1000, {2.5}, {0.75})
    assert ("sa_lr", 0.03) in calls and names.index("sa_lr") < names.index("sa_set")      # default: tf_lr
    lam_u, lam_f = nn.get_sa_weights()
    assert lam_u.shape == (4,) and lam_f.shape == (1000,)


def test_sa_keys_reach_the_engine_and_default_off(monkeypatch):
    _, calls = _run(monkeypatch, _hp(sa_weights=True, sa_lr=0.0))
    assert ("sa_lr", 0.0) in calls
    assert [c for c in calls if c[0] == "sa_set"] == [("sa_set", 4, 1000, {1.0}, {1.0})]
    nn, off = _run(monkeypatch, _hp())
    assert not any(c[0].startswith("sa_") for c in off)
    with pytest.raises(ValueError, match="sa_weights"):
        nn.get_sa_weights()


@pytest.mark.parametrize("extra,key", [
    ({"dtype": "f32"}, "dtype"),
    ({"dtype": "float32"}, "dtype"),
    ({"resample_every": 10}, "resample_every"),
    ({"resample": "rad", "resample_every": 10}, "resample_every"),
    ({"sa_lr": -1.0}, "sa_lr"),
    ({"sa_lr": float("nan")}, "sa_lr"),
    ({"sa_init": [1.0]}, "sa_init"),
    ({"sa_init": [1.0, float("inf")]}, "sa_init"),
])
def test_bad_sa_hp_is_refused_before_an_engine_is_made(monkeypatch, extra, key):
    _utils()
    import neuralnetwork
    monkeypatch.setattr(neuralnetwork, "Engine", _Engine)
    _Engine.log = None
    with pytest.raises(ValueError, match=re.escape(key)):
        neuralnetwork.NeuralNetwork(_hp(sa_weights=True, **extra), None, [1.0, 1.0], [-1.0, 0.0])
    assert _Engine.log is None


@pytest.mark.parametrize("pde", ["burgers_ide", "schrodinger", "burgers_disc", "burgers_disc_ide"])
def test_sa_is_refused_for_other_models(monkeypatch, pde):
    _utils()
    import neuralnetwork
    monkeypatch.setattr(neuralnetwork, "Engine", _Engine)
    _Engine.log = None
    with pytest.raises(ValueError, match="sa_weights"):
        neuralnetwork.NeuralNetwork(_hp(sa_weights=True), None, [1.0, 1.0], [-1.0, 0.0], pde=pde)
    assert _Engine.log is None


def test_sa_is_refused_in_a_data_parallel_world(monkeypatch):
    _utils()
    import neuralnetwork

    def _no_process_group(*a, **k):
        # the refusal must come first: a real world of 2 would wait here for a second rank that never comes
        raise AssertionError("the data-parallel set-up was reached")

    monkeypatch.setattr(neuralnetwork, "Engine", _Engine)
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setattr(neuralnetwork.parallel, "from_env", _no_process_group)
    monkeypatch.setattr(neuralnetwork.parallel, "init_engine_comm", _no_process_group)
    _Engine.log = None
    with pytest.raises(ValueError, match="data-parallel"):
        neuralnetwork.NeuralNetwork(_hp(sa_weights=True), None, [1.0, 1.0], [-1.0, 0.0])
    assert _Engine.log is None


def test_ensemble_refuses_sa_weights(monkeypatch):
    _utils()
    import ensemble

    def _no_engine(*a, **k):
        raise AssertionError("an engine was made")

    monkeypatch.setattr(ensemble, "Ensemble", _no_engine)
    with pytest.raises(ValueError, match="sa_weights"):
        ensemble.NeuralNetworkEnsemble(_hp(sa_weights=True), None, [1.0, 1.0], [-1.0, 0.0], [{}, {}])
