"""CPU: the per-member point-set surface of ensembles (include/pinn_hip.h pinn_ensk_*, pinn_native.Ensemble set_* /
lhs_collocation, utils/ensemble.py "nu" / "resample_seed" / resample_every) -- exported symbols and ctypes signatures,
the wrapper's shape checks, and NeuralNetworkEnsemble's redraw schedule against NeuralNetwork.tf_optimization's, with the
engines stubbed out."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

ENSK_SYMBOLS = {"pinn_ensk_set_collocation", "pinn_ensk_set_data", "pinn_ensk_set_pde_params",
                "pinn_ensk_lhs_collocation"}
LAYERS8 = [2] + [20] * 8 + [1]


def test_per_member_set_symbols_are_exported_with_the_declared_signatures():
    import pinn_native
    lib = pinn_native.load()
    header = open(os.path.join(ROOT, "include", "pinn_hip.h")).read()
    assert set(re.findall(r"\b(pinn_ensk_[a-z0-9_]+)\s*\(", header)) == ENSK_SYMBOLS
    assert ENSK_SYMBOLS <= set(pinn_native.exported_symbols())
    for name in ENSK_SYMBOLS:
        fn = getattr(lib, name)
        res, args = pinn_native._SIGNATURES[name]
        assert fn.restype is res and list(fn.argtypes) == list(args), name
        proto = re.search(r"\b%s\s*\(([^)]*)\)" % name, header).group(1)
        assert len([a for a in proto.split(",") if a.strip()]) == len(args), name
    assert pinn_native._SIGNATURES["pinn_ensk_lhs_collocation"][1][-1] == ctypes.POINTER(ctypes.c_uint64)
    assert lib.pinn_abi_version() == 6


def test_per_member_calls_refuse_a_null_ensemble():
    import pinn_native
    lib = pinn_native.load()
    x = (ctypes.c_double * 4)()
    s = (ctypes.c_uint64 * 1)()
    assert lib.pinn_ensk_set_collocation(None, x, 1, 1) == -1
    assert lib.pinn_ensk_set_data(None, x, x, 1, 1) == -1
    assert lib.pinn_ensk_set_pde_params(None, x, 1) == -1
    assert lib.pinn_ensk_lhs_collocation(None, 10, 0, 10, s) == -1


class _Lib(object):
    """records the library calls of a pinn_native.Ensemble built without a device"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append(name)
            return 0
        return call


def _wrapper(K=3):
    import pinn_native
    ens = pinn_native.Ensemble.__new__(pinn_native.Ensemble)
    ens._lib, ens._h, ens.n_members, ens.n_params = _Lib(), None, K, 3021
    return ens


def test_wrapper_routes_shared_and_per_member_arrays():
    ens = _wrapper(3)
    ens.set_collocation(np.zeros((10, 2)))
    ens.set_collocation(np.zeros((3, 10, 2)))
    ens.set_data(np.zeros((5, 2)), np.zeros((5, 1)))
    ens.set_data(np.zeros((3, 5, 2)), np.zeros((3, 5, 1)))
    ens.set_data(np.zeros((3, 5, 2)), np.zeros((3, 5)))
    ens.set_pde_params(0.01)
    ens.set_pde_params(np.array([0.01, 0.02, 0.03]))
    ens.lhs_collocation(100, [1, 2, 3])
    ens.lhs_collocation(100, np.array([1, 2, 3], dtype=np.uint64), first=10, count=50)
    assert ens._lib.calls == ["pinn_ens_set_collocation", "pinn_ensk_set_collocation", "pinn_ens_set_data",
                              "pinn_ensk_set_data", "pinn_ensk_set_data", "pinn_ens_set_pde_params",
                              "pinn_ensk_set_pde_params", "pinn_ensk_lhs_collocation", "pinn_ensk_lhs_collocation"]


@pytest.mark.parametrize("call", ["colloc_k", "colloc_cols", "data_k", "data_u", "data_u_k", "nu_k", "seeds_k",
                                  "seeds_float"])
def test_wrapper_raises_value_error_before_any_library_call(call):
    ens = _wrapper(3)
    with pytest.raises(ValueError):
        {"colloc_k": lambda: ens.set_collocation(np.zeros((4, 10, 2))),
         "colloc_cols": lambda: ens.set_collocation(np.zeros((3, 10, 3))),
         "data_k": lambda: ens.set_data(np.zeros((2, 5, 2)), np.zeros((2, 5, 1))),
         "data_u": lambda: ens.set_data(np.zeros((5, 2)), np.zeros((6, 1))),
         "data_u_k": lambda: ens.set_data(np.zeros((3, 5, 2)), np.zeros((5, 3, 1))),
         "nu_k": lambda: ens.set_pde_params(np.array([0.1, 0.2])),
         "seeds_k": lambda: ens.lhs_collocation(100, [1, 2]),
         "seeds_float": lambda: ens.lhs_collocation(100, [1.0, 2.0, 3.0])}[call]()
    assert ens._lib.calls == []


class _StubEnsemble(object):
    """pinn_native.Ensemble without a device: records the calls NeuralNetworkEnsemble makes"""

    def __init__(self, layers, lb, ub, n_members, pde="burgers", dtype="f64", device=0):
        self.n_members, self.log, self.nu = n_members, [], None

    def set_weights(self, W):
        pass

    def set_collocation(self, X_f):
        self.log.append(("colloc", np.shape(X_f)))

    def set_data(self, X_u, u):
        self.log.append(("data", np.shape(X_u), np.shape(u)))

    def set_pde_params(self, nu):
        self.nu = nu

    def lhs_collocation(self, n_design, seeds):
        self.log.append(("lhs", n_design, [int(s) for s in seeds]))

    def adam_init(self, lr, *a):
        pass

    def adam_run(self, n):
        self.log.append(("adam", n))
        return np.zeros((n, self.n_members))

    def status(self):
        return np.zeros(self.n_members, dtype=np.int64), np.zeros(self.n_members, dtype=np.int64)


class _StubEngine(object):
    """pinn_native.Engine without a device: what NeuralNetwork.tf_optimization asks of it"""

    def __init__(self, log):
        self.log, self.n_f = log, 0

    def lhs_collocation(self, n_design, seed, first=0, count=None):
        self.log.append(("lhs", n_design, int(seed)))

    def adam_run(self, n):
        self.log.append(("adam", n))
        return np.zeros(n)


class _Logger(object):
    quiet = True

    def __init__(self, frequency):
        self.frequency = frequency

    def log_train_opt(self, name):
        pass

    def log_train_epoch(self, *a, **k):
        pass

    def get_elapsed(self):
        return ""


def _hp(**kw):
    return dict({"layers": LAYERS8, "tf_epochs": 73, "tf_lr": 0.03, "tf_b1": 0.9, "tf_eps": None, "nt_epochs": 0,
                 "nt_lr": 0.8, "nt_ncorr": 50, "log_frequency": 10}, **kw)


def _solo_schedule(hp, n_design, freq):
    """the (lhs, adam) calls NeuralNetwork.tf_optimization makes for hp, without an engine"""
    import neuralnetwork
    nn = neuralnetwork.NeuralNetwork.__new__(neuralnetwork.NeuralNetwork)
    log = []
    nn._engine, nn.logger, nn.tf_epochs = _StubEngine(log), _Logger(freq), int(hp["tf_epochs"])
    nn._resample_every, nn._resample_seed = int(hp.get("resample_every", 0)), int(hp.get("resample_seed", 1234))
    nn._n_f_total, nn._dp, nn._async_log = n_design, None, False
    nn._bind = lambda X_u, u: None
    nn._log_custom = lambda: ""
    nn.tf_optimization(None, None)
    return log


@pytest.mark.parametrize("every,freq", [(25, 10), (7, 10), (10, 10), (0, 10), (30, 4)])
def test_resampling_schedule_and_seeds_equal_neuralnetwork_per_member(monkeypatch, every, freq):
    import ensemble
    monkeypatch.setattr(ensemble.NeuralNetworkEnsemble, "engine_class", _StubEnsemble)
    hp = _hp(resample_every=every, log_frequency=freq)
    members = [{"seed": 1, "resample_seed": 100}, {"seed": 2, "resample_seed": 2 ** 33 + 5, "nu": 0.02},
               {"seed": 3}]                                          # (the default resample_seed, 1234)
    ens = ensemble.NeuralNetworkEnsemble(hp, _Logger(freq), [1.0, 1.0], [-1.0, 0.0], members)
    ens.set_collocation(np.zeros((3, 500, 2)))
    ens.set_pde_params(0.01)
    assert np.array_equal(ens._engine.nu, [0.01, 0.02, 0.01])
    ens.fit(np.zeros((3, 20, 2)), np.zeros((3, 20, 1)))
    log = ens._engine.log
    assert log[0] == ("colloc", (3, 500, 2)) and log[1] == ("data", (3, 20, 2), (3, 20, 1))
    got = log[2:]
    per_member = [_solo_schedule(dict(hp, **m), 500, freq) for m in members]
    adam = [c for c in per_member[0] if c[0] == "adam"]
    assert [c for c in got if c[0] == "adam"] == adam
    for k in range(3):                                             # the same boundaries and member k's seeds
        assert [c for c in per_member[k] if c[0] == "adam"] == adam
        mine = [(c[0], c[1], c[2][k]) if c[0] == "lhs" else c for c in got]
        assert mine == per_member[k], k
    assert any(c[0] == "lhs" for c in got) == (every > 0)


def test_member_keys_accept_nu_and_resample_seed_and_refuse_unknown(monkeypatch):
    import ensemble
    monkeypatch.setattr(ensemble.NeuralNetworkEnsemble, "engine_class", _StubEnsemble)
    assert {"nu", "resample_seed"} <= set(ensemble.MEMBER_KEYS)
    ens = ensemble.NeuralNetworkEnsemble(_hp(), None, [1.0, 1.0], [-1.0, 0.0], [{"nu": 0.1}, {"resample_seed": 3}])
    assert np.array_equal(ens.resample_seeds, [1234, 3])
    ens.set_pde_params(0.5)
    assert np.array_equal(ens._engine.nu, [0.1, 0.5])
    with pytest.raises(ValueError, match="overrides"):
        ensemble.NeuralNetworkEnsemble(_hp(), None, [1.0, 1.0], [-1.0, 0.0], [{"resample_every": 5}])
