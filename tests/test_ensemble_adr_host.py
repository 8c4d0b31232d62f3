"""CPU: the host surface of ensembles of the adr kind (include/pinn_hip.h pinn_adr_ens_create and its four calls,
pinn_native.AdrEnsemble, utils/ensemble.py pde="adr") -- exported symbols and signatures, the constructors' refusals, which
come before any device is touched, and NeuralNetworkEnsemble's "adr" member key, set_pde_params and _set_boundary with the
engine stubbed out."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

ADR_ENS_SYMBOLS = {"pinn_adr_ens_create", "pinn_adr_ens_set_boundary", "pinn_adr_ensk_set_boundary", "pinn_adr_ensk_set_params",
                   "pinn_adr_ens_get_params"}
EINVAL, EUNSUPPORTED = -1, -5
LAYERS8 = [2] + [20] * 8 + [1]
ALLEN_CAHN, FISHER_KPP = [0.0, 0.0, 1e-4, -5.0, 0.0, 5.0], [0.0, 0.0, 0.01, -2.0, 2.0, 0.0]


def test_adr_ensemble_symbols_are_exported_with_the_declared_signatures():
    import pinn_native
    lib = pinn_native.load()
    header = open(os.path.join(ROOT, "include", "pinn_hip.h")).read()
    assert ADR_ENS_SYMBOLS <= set(pinn_native.exported_symbols())
    for name in ADR_ENS_SYMBOLS:
        fn = getattr(lib, name)
        res, args = pinn_native._SIGNATURES[name]
        assert fn.restype is res and list(fn.argtypes) == list(args), name
        proto = re.search(r"^int %s\s*\(([^)]*)\)" % name, header, flags=re.M).group(1)
        assert len([a for a in proto.split(",") if a.strip()]) == len(args), name
    assert lib.pinn_abi_version() == 6


def _create_adr(lib, layers, K, lb=(-1.0, 0.0), ub=(1.0, 1.0)):
    h = ctypes.c_void_p()
    arr = (ctypes.c_int * len(layers))(*layers)
    lo, hi = (ctypes.c_double * 2)(*lb), (ctypes.c_double * 2)(*ub)
    rc = lib.pinn_adr_ens_create(ctypes.byref(h), arr, len(layers), lo, hi, 0, K)
    return rc, h, lib.pinn_last_error().decode(errors="replace")


@pytest.mark.parametrize("K", [0, -1, 65])
def test_create_adr_refuses_a_bad_member_count_before_touching_a_device(K):
    import pinn_native
    rc, h, msg = _create_adr(pinn_native.load(), LAYERS8, K)
    assert rc == EINVAL and not h and "outside 1..64" in msg


@pytest.mark.parametrize("layers", [[2, 20, 20, 20, 1], [2] + [20] * 5 + [1], [2] + [20] * 10 + [1], [2] + [32] * 8 + [1],
                                    [3] + [20] * 8 + [1], [2] + [20] * 8 + [2], [2, 20, 20, 21, 20, 1], [2, 1]])
def test_create_adr_refuses_other_shapes_before_touching_a_device(layers):
    import pinn_native
    rc, h, msg = _create_adr(pinn_native.load(), layers, 4)
    assert rc == EUNSUPPORTED and not h and "4, 6 or 8 hidden layers" in msg


def test_create_adr_refuses_null_arguments():
    import pinn_native
    lib = pinn_native.load()
    arr = (ctypes.c_int * 10)(*LAYERS8)
    lo = (ctypes.c_double * 2)(-1.0, 0.0)
    assert lib.pinn_adr_ens_create(None, arr, 10, lo, lo, 0, 2) == EINVAL
    h = ctypes.c_void_p()
    assert lib.pinn_adr_ens_create(ctypes.byref(h), arr, 10, None, lo, 0, 2) == EINVAL
    x = (ctypes.c_double * 12)()
    assert lib.pinn_adr_ens_set_boundary(None, x, x, 1, 1) == EINVAL
    assert lib.pinn_adr_ensk_set_boundary(None, x, x, 1, 1) == EINVAL
    assert lib.pinn_adr_ensk_set_params(None, x, 2) == EINVAL
    assert lib.pinn_adr_ens_get_params(None, x, 2) == EINVAL


@pytest.mark.parametrize("pde", ["adr", "adr_ide"])
def test_the_old_constructor_still_refuses_the_adr_kinds(pde):
    import pinn_native
    lib = pinn_native.load()
    h = ctypes.c_void_p()
    arr = (ctypes.c_int * 10)(*LAYERS8)
    lo, hi = (ctypes.c_double * 2)(-1.0, 0.0), (ctypes.c_double * 2)(1.0, 1.0)
    kind = pinn_native.pde_kind(pde)
    assert kind in (5, 6)
    rc = lib.pinn_ens_create(ctypes.byref(h), arr, 10, lo, hi, kind, pinn_native.DTYPES["f64"], 0, 4)
    assert rc == EUNSUPPORTED and not h
    assert "ensembles support Burgers" in lib.pinn_last_error().decode(errors="replace")


# ---- the ctypes wrapper, built without a device ----------------------------------------------------------------------------
class _Lib(object):
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name,) + tuple(a for a in args if isinstance(a, int)))
            return 0
        return call


def _wrapper(K=3):
    import pinn_native
    ens = pinn_native.AdrEnsemble.__new__(pinn_native.AdrEnsemble)
    ens._lib, ens._h, ens.n_members, ens.n_params = _Lib(), None, K, 3021
    return ens


def test_wrapper_routes_shared_and_per_member_arrays():
    import pinn_native
    assert issubclass(pinn_native.AdrEnsemble, pinn_native.Ensemble)
    ens = _wrapper(3)
    ens.set_boundary(np.zeros((7, 2)), np.zeros((7, 2)))
    ens.set_boundary(np.zeros((3, 7, 2)), np.zeros((3, 7, 2)), n_total=9)
    ens.set_pde_params(*ALLEN_CAHN)
    ens.set_pde_params(np.array(ALLEN_CAHN))
    ens.set_pde_params(np.array([ALLEN_CAHN, FISHER_KPP, ALLEN_CAHN]))
    assert ens.get_pde_params().shape == (3, 6)
    assert ens._lib.calls == [("pinn_adr_ens_set_boundary", 7, 7), ("pinn_adr_ensk_set_boundary", 7, 9),
                              ("pinn_ens_set_pde_params", 6), ("pinn_ens_set_pde_params", 6),
                              ("pinn_adr_ensk_set_params", 3), ("pinn_adr_ens_get_params", 3)]


@pytest.mark.parametrize("call", ["pairs_k", "pairs_mixed", "pairs_cols", "rows_k", "rows_cols"])
def test_wrapper_raises_value_error_before_any_library_call(call):
    ens = _wrapper(3)
    with pytest.raises(ValueError):
        {"pairs_k": lambda: ens.set_boundary(np.zeros((4, 7, 2)), np.zeros((4, 7, 2))),
         "pairs_mixed": lambda: ens.set_boundary(np.zeros((7, 2)), np.zeros((3, 7, 2))),
         "pairs_cols": lambda: ens.set_boundary(np.zeros((3, 7, 3)), np.zeros((3, 7, 3))),
         "rows_k": lambda: ens.set_pde_params(np.zeros((2, 6))),
         "rows_cols": lambda: ens.set_pde_params(np.zeros((3, 5)))}[call]()
    assert ens._lib.calls == []


# ---- NeuralNetworkEnsemble(pde="adr") with a stubbed engine class -------------------------------------------------------------
class _StubEnsemble(object):
    def __init__(self, layers, lb, ub, n_members, pde="burgers", dtype="f64", device=0):
        self.n_members, self.pde, self.params, self.pairs = n_members, pde, [], []

    def set_weights(self, W):
        pass

    def set_pde_params(self, p):
        self.params.append(np.array(p, dtype=np.float64))

    def set_boundary(self, X_lb, X_ub):
        self.pairs.append((np.shape(X_lb), np.shape(X_ub)))


def _hp(**kw):
    return dict({"layers": LAYERS8, "tf_epochs": 5, "tf_lr": 0.03, "tf_b1": 0.9, "tf_eps": None, "nt_epochs": 0,
                 "nt_lr": 0.8, "nt_ncorr": 50, "log_frequency": 10}, **kw)


def _nn_ensemble(monkeypatch, members, pde="adr"):
    import ensemble
    monkeypatch.setattr(ensemble.NeuralNetworkEnsemble, "engine_class", _StubEnsemble)
    return ensemble.NeuralNetworkEnsemble(_hp(), None, [1.0, 1.0], [-1.0, 0.0], members, pde=pde)


def test_adr_overrides_reach_set_pde_params_as_rows(monkeypatch):
    import ensemble
    assert "adr" in ensemble.MEMBER_KEYS
    ens = _nn_ensemble(monkeypatch, [{"seed": 1}, {"seed": 2, "adr": FISHER_KPP}, {"seed": 3}])
    assert ens._engine.pde == "adr"
    burgers = [0.0, 1.0, 0.01 / np.pi, 0.0, 0.0, 0.0]
    # the constructor already hands the overrides over, on a new adr context's default for the others
    assert np.array_equal(ens._engine.params[-1], [burgers, FISHER_KPP, burgers])
    ens.set_pde_params(ALLEN_CAHN)                                     # six numbers: a member's override wins
    assert np.array_equal(ens._engine.params[-1], [ALLEN_CAHN, FISHER_KPP, ALLEN_CAHN])
    rows = np.array([ALLEN_CAHN, ALLEN_CAHN, burgers])
    ens.set_pde_params(rows)                                           # [K, 6]: likewise
    assert np.array_equal(ens._engine.params[-1], [ALLEN_CAHN, FISHER_KPP, burgers])
    with pytest.raises(ValueError):
        ens.set_pde_params([0.0, 1.0, 0.01])
    with pytest.raises(ValueError):
        ens.set_pde_params(np.zeros((2, 6)))
    # without overrides six numbers travel as six numbers
    plain = _nn_ensemble(monkeypatch, [{"seed": 1}, {"seed": 2}])
    assert plain._engine.params == []
    plain.set_pde_params(ALLEN_CAHN)
    assert plain._engine.params[-1].shape == (6,) and np.array_equal(plain._engine.params[-1], ALLEN_CAHN)


def test_member_keys_nu_and_adr_are_kind_specific(monkeypatch):
    with pytest.raises(ValueError, match='"nu"'):
        _nn_ensemble(monkeypatch, [{"seed": 1, "nu": 0.01}], pde="adr")
    with pytest.raises(ValueError, match='"adr"'):
        _nn_ensemble(monkeypatch, [{"seed": 1, "adr": ALLEN_CAHN}], pde="burgers")
    with pytest.raises(ValueError, match="six numbers"):
        _nn_ensemble(monkeypatch, [{"seed": 1, "adr": [0.0, 1.0]}], pde="adr")
    bur = _nn_ensemble(monkeypatch, [{"seed": 1}], pde="burgers")
    with pytest.raises(ValueError, match="periodic pairs"):
        bur._set_boundary(np.zeros((4, 2)), np.zeros((4, 2)))


def test_set_boundary_passes_shared_and_per_member_pairs_through(monkeypatch):
    ens = _nn_ensemble(monkeypatch, [{"seed": 1}, {"seed": 2}])
    ens._set_boundary(np.zeros((9, 2)), np.zeros((9, 2)))
    ens._set_boundary(np.zeros((2, 9, 2)), np.zeros((2, 9, 2)))
    assert ens._engine.pairs == [((9, 2), (9, 2)), ((2, 9, 2), (2, 9, 2))]


def test_the_real_engine_class_for_adr_is_the_adr_ensemble():
    import ensemble
    import pinn_native
    assert ensemble.NeuralNetworkEnsemble.engine_class is pinn_native.Ensemble
    assert ensemble.NeuralNetworkEnsemble.adr_engine_class is pinn_native.AdrEnsemble
