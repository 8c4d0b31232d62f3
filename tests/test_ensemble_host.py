"""CPU: the ensemble surface (include/pinn_hip.h pinn_ens_*, pinn_native.Ensemble, utils/ensemble.py) -- exported symbols
and ctypes signatures, the refusals of pinn_ens_create that come before any device work, and the members' initial weight
vectors against NeuralNetwork._initial_weights with the engine stubbed out."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

ENS_SYMBOLS = {"pinn_ens_create", "pinn_ens_destroy", "pinn_ens_size", "pinn_ens_set_collocation", "pinn_ens_set_data",
               "pinn_ens_set_pde_params", "pinn_ens_set_weights", "pinn_ens_get_weights", "pinn_ens_loss_grad",
               "pinn_ens_adam_init", "pinn_ens_adam_run", "pinn_ens_lbfgs_begin", "pinn_ens_lbfgs_run",
               "pinn_ens_predict", "pinn_ens_error_l2", "pinn_ens_get_status"}

LAYERS8 = [2] + [20] * 8 + [1]


def _c_layers(layers):
    return (ctypes.c_int * len(layers))(*layers)


def test_ensemble_symbols_are_exported_with_the_declared_signatures():
    import pinn_native
    lib = pinn_native.load()
    header = open(os.path.join(ROOT, "include", "pinn_hip.h")).read()
    declared = set(re.findall(r"\b(pinn_ens_[a-z0-9_]+)\s*\(", header))
    assert declared == ENS_SYMBOLS
    assert ENS_SYMBOLS <= set(pinn_native.exported_symbols())
    for name in ENS_SYMBOLS:
        fn = getattr(lib, name)
        res, args = pinn_native._SIGNATURES[name]
        assert fn.restype is res and list(fn.argtypes) == list(args), name
        # argument count of the C prototype
        proto = re.search(r"\b%s\s*\(([^)]*)\)" % name, header).group(1)
        assert len([a for a in proto.split(",") if a.strip()]) == len(args), name
    assert lib.pinn_abi_version() == 6                    # additive: the version stays


@pytest.mark.parametrize("case", ["float32", "schrodinger", "disc", "k0", "k65", "width", "depth"])
def test_ens_create_refuses_before_touching_a_device(case):
    import pinn_native
    lib = pinn_native.load()
    h = ctypes.c_void_p()
    lb = (ctypes.c_double * 2)(-1.0, 0.0)
    ub = (ctypes.c_double * 2)(1.0, 1.0)
    layers, pde, dtype, k, want = LAYERS8, 0, 1, 4, -5
    if case == "float32":
        dtype = 0
    elif case == "schrodinger":
        layers, pde = [2, 100, 100, 100, 100, 2], 2
    elif case == "disc":
        layers, pde = [1, 20, 20, 9], 3
    elif case == "k0":
        k, want = 0, -1
    elif case == "k65":
        k, want = 65, -1
    elif case == "width":
        layers = [2] + [32] * 8 + [1]
    elif case == "depth":
        layers = [2] + [20] * 5 + [1]
    rc = lib.pinn_ens_create(ctypes.byref(h), _c_layers(layers), len(layers), lb, ub, pde, dtype, 0, k)
    assert rc == want, (case, rc, lib.pinn_last_error())
    assert not h.value
    msg = lib.pinn_last_error().decode()
    assert {"float32": "float64", "schrodinger": "Schrodinger", "disc": "discrete-time", "k0": "1..64",
            "k65": "1..64", "width": "width", "depth": "hidden layers"}[case] in msg
    assert lib.pinn_ens_destroy(None) == 0


def test_ensemble_wrapper_raises_on_refusal():
    import pinn_native
    with pytest.raises(pinn_native.PinnNativeError, match="float64"):
        pinn_native.Ensemble(LAYERS8, [-1.0, 0.0], [1.0, 1.0], 3, dtype="f32")
    with pytest.raises(pinn_native.PinnNativeError, match="1..64"):
        pinn_native.Ensemble(LAYERS8, [-1.0, 0.0], [1.0, 1.0], 0)


class _StubEngine(object):
    """what NeuralNetworkEnsemble needs of pinn_native.Ensemble at construction, without a device"""

    def __init__(self, layers, lb, ub, n_members, pde="burgers", dtype="f64", device=0):
        self.layers, self.n_members, self.pde = layers, n_members, pde
        self.weights = None

    def set_weights(self, W):
        self.weights = np.array(W, dtype=np.float64)


@pytest.mark.parametrize("pde", ["burgers", "burgers_ide"])
def test_member_initial_weights_equal_neuralnetwork_initial_weights(monkeypatch, pde):
    import ensemble
    import neuralnetwork
    monkeypatch.setattr(ensemble.NeuralNetworkEnsemble, "engine_class", _StubEngine)
    hp = {"layers": LAYERS8, "tf_epochs": 10, "tf_lr": 0.03, "tf_b1": 0.9, "tf_eps": None, "nt_epochs": 20,
          "nt_lr": 0.8, "nt_ncorr": 50, "log_frequency": 10}
    members = [{"seed": 1}, {"seed": 2, "tf_lr": 0.01}, {"init_scale": 1.0 + 2.0 ** -40}, {"seed": 7, "nt_epochs": 5},
               {"init_scale": 1.0}]
    neuralnetwork.set_seed(99)
    ens = ensemble.NeuralNetworkEnsemble(hp, None, [1.0, 1.0], [-1.0, 0.0], members, pde=pde)
    W = ens._engine.weights
    P = sum(a * b + b for a, b in zip(LAYERS8[:-1], LAYERS8[1:])) + (2 if pde == "burgers_ide" else 0)
    assert W.shape == (5, P)

    class _Solo(object):                                   # NeuralNetwork._initial_weights without an engine
        layers = LAYERS8

        def _extra_params(self):
            return np.array([0.0, -6.0]) if pde == "burgers_ide" else np.zeros(0)

    for k, m in enumerate(members):
        neuralnetwork.set_seed(99)                         # a member without a seed: what a model built first would get
        want = neuralnetwork.NeuralNetwork._initial_weights(_Solo(), dict(hp, **m))
        assert np.array_equal(W[k], want), k
    assert not np.array_equal(W[2], W[4])                  # the perturbed member differs from the plain one
    assert ens.member_hp[1]["tf_lr"] == 0.01 and ens.member_hp[3]["nt_epochs"] == 5
    if pde == "burgers_ide":
        assert np.all(W[:, -2] == 0.0) and np.all(W[:, -1] == -6.0)
    with pytest.raises(ValueError, match="overrides"):
        ensemble.NeuralNetworkEnsemble(hp, None, [1.0, 1.0], [-1.0, 0.0], [{"tf_b1": 0.5}], pde=pde)
