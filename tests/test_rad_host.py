"""CPU: residual-based adaptive collocation (include/pinn_hip.h pinn_rad_collocation, csrc/kernels_rad.h,
pinn_native.Engine.rad_collocation, utils/neuralnetwork.py hp["resample"] = "rad") -- the exported symbol and its ctypes
signature, properties of the numpy restatement (tests/helpers/rad_ref.py) on synthetic residuals, and NeuralNetwork's
redraw schedule and hp refusals with the engine stubbed out."""
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
import rad_ref  # noqa: E402


def _utils():
    p = os.path.join(ROOT, "pinns-tf2.0_amd", "utils")
    if p not in sys.path:
        sys.path.insert(0, p)


# ---- the C surface ----------------------------------------------------------------------------------------------------
def test_rad_symbol_is_declared_exported_and_typed():
    import pinn_native
    lib = pinn_native.load()
    header = open(os.path.join(ROOT, "include", "pinn_hip.h")).read()
    proto = re.search(r"\bint\s+pinn_rad_collocation\s*\(([^)]*)\)\s*;", header)
    assert proto, "pinn_rad_collocation is not declared"
    res, args = pinn_native._SIGNATURES["pinn_rad_collocation"]
    assert "pinn_rad_collocation" in pinn_native.exported_symbols()
    fn = lib.pinn_rad_collocation
    assert fn.restype is res and list(fn.argtypes) == list(args)
    assert len([a for a in proto.group(1).split(",") if a.strip()]) == len(args) == 8
    assert args[5] is ctypes.c_uint64 and args[6] is ctypes.c_int and args[7] is ctypes.c_double
    assert lib.pinn_abi_version() == 6
    assert lib.pinn_rad_collocation(None, 10, 0, 10, 100, 1, 1, 1.0) == -1          # PINN_EINVAL, no context
    assert hasattr(pinn_native.Engine, "rad_collocation")


def test_engine_wrapper_passes_the_arguments_through():
    import pinn_native
    seen = []

    class _Lib(object):
        def pinn_rad_collocation(self, *a):
            seen.append(a[1:])
            return 0

    eng = pinn_native.Engine.__new__(pinn_native.Engine)
    eng._lib, eng._h, eng.n_f = _Lib(), None, 0
    eng.rad_collocation(1000, 7, 5000)
    assert seen[-1] == (1000, 0, 1000, 5000, 7, 1, 1.0) and eng.n_f == 1000
    eng.rad_collocation(1000, 2 ** 40 + 3, 100, k=3, c=0.5, first=250, count=250)
    assert seen[-1] == (1000, 250, 250, 100, 2 ** 40 + 3, 3, 0.5) and eng.n_f == 250


# ---- the restatement ----------------------------------------------------------------------------------------------------
def _synthetic(M, seed=0):
    rs = np.random.RandomState(seed)
    return rs.standard_normal(M) * np.exp(rs.uniform(-4, 4, M))


def test_slices_concatenate_to_the_full_draw():
    a = rad_ref.magnitudes(_synthetic(1000), 2)
    w, W = rad_ref.weights(a, 1.0)
    full = rad_ref.draw_indices(w, W, 99, 0, 2003)
    cuts = [0, 1, 700, 1500, 2003]
    parts = [rad_ref.draw_indices(w, W, 99, lo, hi - lo) for lo, hi in zip(cuts[:-1], cuts[1:])]
    assert np.array_equal(np.concatenate(parts), full)


def test_draw_frequencies_follow_the_weights():
    M, n = 50, 200000
    a = rad_ref.magnitudes(np.linspace(0.0, 3.0, M), 1)
    w, W = rad_ref.weights(a, 0.5)
    idx = rad_ref.draw_indices(w, W, 12345, 0, n)
    obs = np.bincount(idx, minlength=M).astype(float)
    exp = n * w.astype(float) / float(W)
    assert exp.min() > 5
    chi2 = float(((obs - exp) ** 2 / exp).sum())
    assert chi2 < 100.0, chi2                      # 49 degrees of freedom: p ~ 2e-5 at 100
    assert obs[0] > 0                              # c > 0: even the zero-residual point is drawn


def test_zero_and_nan_residuals_give_a_uniform_draw():
    M = 64
    for f in (np.zeros(M), np.full(M, np.nan), np.full((M, 2), np.inf)):
        w, W = rad_ref.weights(rad_ref.magnitudes(f, 3), 7.0)
        assert np.array_equal(w, np.ones(M, dtype=np.uint64)) and W == M
        idx = rad_ref.draw_indices(w, W, 5, 0, 64000)
        counts = np.bincount(idx, minlength=M)
        assert counts.min() > 800 and counts.max() < 1200


def test_nonfinite_entries_count_as_zero():
    f = np.array([1.0, np.nan, 2.0, np.inf, -2.0, 1e200])
    a = rad_ref.magnitudes(f, 2)
    assert a.tolist() == [1.0, 0.0, 4.0, 0.0, 4.0, 0.0]             # (1e200)^2 overflows
    w, W = rad_ref.weights(a, 0.0)
    assert w.tolist() == [2 ** 30, 0, 2 ** 32, 0, 2 ** 32, 0] and W == 2 ** 30 + 2 ** 33
    idx = rad_ref.draw_indices(w, W, 3, 0, 5000)
    assert set(np.unique(idx).tolist()) == {0, 2, 4}                   # zero weights are never drawn


def test_the_cdf_total_stays_below_2_63_at_the_limits():
    M, c = 1 << 24, 64.0
    Q = M * (1 << 32)                                                   # every q_i = 2^32
    r = int(np.floor((c * float(Q)) / float(M)))
    W = Q + M * r
    assert r == 64 * (1 << 32) and W < 2 ** 63
    # and the restatement's own arithmetic on a pool of equal residuals at the limit
    w, W2 = rad_ref.weights(np.ones(M), c)
    assert W2 == W and int(np.cumsum(w, dtype=np.uint64)[-1]) == W


def test_weights_are_proportional_to_a_over_mean_plus_c():
    # w_i = s (a_i / mean(a) + c) with s = 2^32 mean(a) / A, up to the floors of q_i and r (one unit each) and c times the
    # floor deficit of Q / M (< 1 unit): relative to the largest weight (>= 2^32) that is 2^-31 at c = 0, (2 + c) 2^-32 in general
    for k, c in ((1, 1.0), (2, 0.0), (4, 64.0), (1, 0.3), (3, 0.0)):
        a = rad_ref.magnitudes(_synthetic(100037, k), k)
        w, W = rad_ref.weights(a, c)
        s = 2.0 ** 32 * a.mean() / a.max()
        want = s * (a / a.mean() + c)
        err = np.abs(w.astype(np.float64) - want) / float(w.max())
        assert err.max() <= (2.0 + c) * 2.0 ** -32, (k, c, err.max())
        if c == 0:
            assert err.max() <= 2.0 ** -31
        assert W == int(w.sum(dtype=np.uint64))


def test_two_outputs_use_the_modulus():
    f = np.array([[3.0, 4.0], [0.0, 0.0], [1.0, 0.0]])
    assert rad_ref.magnitudes(f, 1).tolist() == [5.0, 0.0, 1.0]
    assert rad_ref.magnitudes(f, 2).tolist() == [25.0, 0.0, 1.0]


# ---- NeuralNetwork wiring, engine stubbed ------------------------------------------------------------------------------
class _Engine(object):
    """records the set and optimiser calls of NeuralNetwork"""
    log = None

    def __init__(self, layers, lb, ub, pde="burgers", dtype="f64", device=0):
        self.n_params, self.w, self.calls = 5, np.zeros(5), []
        self.n_f = self.n_u = self.n_b = 0
        self.lb_total = self.lb_done = 0
        type(self).log = self.calls

    def set_weights(self, w): self.w = np.array(w, dtype=np.float64)
    def get_weights(self): return self.w.copy()
    def adam_init(self, *a): pass
    def set_data(self, X, u, n_total=None): pass
    def set_collocation(self, X, n_total=None): self.n_f = len(X); self.calls.append(("colloc", len(X), n_total))
    def status(self): return 0, 0
    def adam_run(self, n, want_losses=True): self.calls.append(("adam", n)); return np.ones(n)
    def lbfgs_begin(self, n, *a): self.calls.append(("lbfgs_begin", n)); self.lb_total, self.lb_done = n, 0

    def lbfgs_run(self, n):
        self.calls.append(("lbfgs", n))
        k = min(n, self.lb_total - self.lb_done)
        its = np.arange(self.lb_done + 1, self.lb_done + k + 1, dtype=np.int32)
        self.lb_done += k
        return its, np.ones(k), int(self.lb_done >= self.lb_total)

    def lhs_collocation(self, n_design, seed, first=0, count=None):
        self.calls.append(("lhs", n_design, seed, first, count))

    def rad_collocation(self, n_design, seed, n_pool, k=1, c=1.0, first=0, count=None):
        self.calls.append(("rad", n_design, seed, n_pool, k, c, first, count))


class _DP(object):
    def __init__(self, world, rank):
        self.world, self.rank = world, rank

    def shard(self, n):
        from pinn_native.parallel import shard_bounds
        return shard_bounds(n, self.world, self.rank)

    def replicas_identical(self, w):
        return True


def _hp(**kw):
    return dict({"layers": [2, 1], "tf_epochs": 35, "tf_lr": 0.03, "tf_b1": 0.9, "tf_eps": None, "nt_epochs": 12,
                 "nt_lr": 0.8, "nt_ncorr": 50, "log_frequency": 10, "async_log": False}, **kw)


def _run(monkeypatch, hp, n_f=1000, dp=None):
    _utils()
    import neuralnetwork
    from logger import Logger
    monkeypatch.setattr(neuralnetwork, "Engine", _Engine)
    with contextlib.redirect_stdout(io.StringIO()):
        nn = neuralnetwork.NeuralNetwork(hp, Logger(hp), [1.0, 1.0], [-1.0, 0.0])
        nn._dp = dp
        nn._set_collocation(np.zeros((n_f, 2)))
        nn.logger.set_error_fn(lambda: 0.5)
        nn.fit(np.zeros((4, 2)), np.zeros((4, 1)))
    return nn, [c for c in nn._engine.calls if c[0] != "colloc"]


def test_rad_redraws_at_every_boundary_with_the_lhs_seeds_and_no_redraw_in_lbfgs(monkeypatch):
    _, calls = _run(monkeypatch, _hp(resample="rad", resample_every=10, resample_seed=40))
    rad = [c for c in calls if c[0] == "rad"]
    assert rad == [("rad", 1000, 40 + e, 10000, 1, 1.0, 0, 1000) for e in (10, 20, 30)]
    assert not any(c[0] == "lhs" for c in calls)
    first_lbfgs = [c[0] for c in calls].index("lbfgs_begin")
    assert all(c[0] != "rad" for c in calls[first_lbfgs:])
    # a redraw sits between the chunks that end and start at its epoch (none at epoch 0)
    assert calls[0][0] == "adam"
    assert [c for c in calls[:first_lbfgs]] == [("adam", 1), ("adam", 9), rad[0], ("adam", 1), ("adam", 9), rad[1],
                                                 ("adam", 1), ("adam", 9), rad[2], ("adam", 1), ("adam", 4)]


def test_rad_keys_reach_the_engine(monkeypatch):
    _, calls = _run(monkeypatch, _hp(resample="rad", resample_every=15, rad_pool=777, rad_k=4, rad_c=64))
    assert [c for c in calls if c[0] == "rad"] == [("rad", 1000, 1234 + e, 777, 4, 64.0, 0, 1000) for e in (15, 30)]
    # the default pool is 10 N_f, at most 2^24
    _, calls = _run(monkeypatch, _hp(resample="rad", resample_every=30, rad_c=0), n_f=2000000)
    assert [c for c in calls if c[0] == "rad"] == [("rad", 2000000, 1234 + 30, 1 << 24, 1, 0.0, 0, 2000000)]


def test_rad_ranks_draw_their_shard_of_one_design(monkeypatch):
    got = []
    for rank in (0, 1):
        nn, calls = _run(monkeypatch, _hp(resample="rad", resample_every=20), n_f=1001, dp=_DP(2, rank))
        got.append([c for c in calls if c[0] == "rad"])
        assert nn._X_f is None                     # gathered again before the next replicated residual
    assert got[0] == [("rad", 1001, 1254, 10010, 1, 1.0, 0, 501)]
    assert got[1] == [("rad", 1001, 1254, 10010, 1, 1.0, 501, 500)]


def test_lhs_sequence_is_unchanged(monkeypatch):
    _, default = _run(monkeypatch, _hp(resample_every=10, resample_seed=40))
    _, explicit = _run(monkeypatch, _hp(resample="lhs", resample_every=10, resample_seed=40, rad_k=3))
    want = [("adam", 1), ("adam", 9), ("lhs", 1000, 50, 0, 1000), ("adam", 1), ("adam", 9), ("lhs", 1000, 60, 0, 1000),
            ("adam", 1), ("adam", 9), ("lhs", 1000, 70, 0, 1000), ("adam", 1), ("adam", 4)]
    assert default[:len(want)] == want and explicit == default
    assert not any(c[0] == "rad" for c in default)
    _, none = _run(monkeypatch, _hp())
    assert not any(c[0] in ("rad", "lhs") for c in none)


@pytest.mark.parametrize("extra,key", [
    ({"resample": "uniform", "resample_every": 10}, "resample"),
    ({"resample": "rad"}, "resample_every"),
    ({"resample": "rad", "resample_every": 0}, "resample_every"),
    ({"resample": "rad", "resample_every": 10, "rad_k": 0}, "rad_k"),
    ({"resample": "rad", "resample_every": 10, "rad_k": 5}, "rad_k"),
    ({"resample": "rad", "resample_every": 10, "rad_k": 1.5}, "rad_k"),
    ({"resample": "rad", "resample_every": 10, "rad_c": -0.5}, "rad_c"),
    ({"resample": "rad", "resample_every": 10, "rad_c": 65.0}, "rad_c"),
    ({"resample": "rad", "resample_every": 10, "rad_c": float("nan")}, "rad_c"),
    ({"resample": "rad", "resample_every": 10, "rad_pool": 0}, "rad_pool"),
    ({"resample": "rad", "resample_every": 10, "rad_pool": (1 << 24) + 1}, "rad_pool"),
])
def test_bad_hp_is_refused_at_construction(monkeypatch, extra, key):
    _utils()
    import neuralnetwork
    monkeypatch.setattr(neuralnetwork, "Engine", _Engine)
    _Engine.log = None
    with pytest.raises(ValueError, match=re.escape(key)):
        neuralnetwork.NeuralNetwork(_hp(**extra), None, [1.0, 1.0], [-1.0, 0.0])
    assert _Engine.log is None                      # refused before an engine was made


@pytest.mark.parametrize("pde", ["burgers_ide", "burgers_disc", "burgers_disc_ide"])
def test_rad_is_refused_for_models_without_a_collocation_set(monkeypatch, pde):
    _utils()
    import neuralnetwork
    monkeypatch.setattr(neuralnetwork, "Engine", _Engine)
    with pytest.raises(ValueError, match="resample"):
        neuralnetwork.NeuralNetwork(_hp(resample="rad", resample_every=10), None, [1.0, 1.0], [-1.0, 0.0], pde=pde)


def test_rad_is_accepted_for_burgers_and_schrodinger(monkeypatch):
    _utils()
    import neuralnetwork
    monkeypatch.setattr(neuralnetwork, "Engine", _Engine)
    for pde in ("burgers", "schrodinger"):
        nn = neuralnetwork.NeuralNetwork(_hp(resample="rad", resample_every=10, rad_k=2, rad_c=0, rad_pool=1 << 24),
                                         None, [1.0, 1.0], [-1.0, 0.0], pde=pde)
        assert (nn._resample, nn._rad_k, nn._rad_c, nn._rad_pool) == ("rad", 2, 0.0, 1 << 24)


def test_ensemble_refuses_rad():
    _utils()
    import ensemble

    class _Stub(object):
        def __init__(self, *a, **k):
            raise AssertionError("an engine was made")

    ensemble_hp = _hp(layers=[2] + [20] * 8 + [1], resample="rad", resample_every=10)
    old = ensemble.NeuralNetworkEnsemble.engine_class
    ensemble.NeuralNetworkEnsemble.engine_class = _Stub
    try:
        with pytest.raises(ValueError, match="resample"):
            ensemble.NeuralNetworkEnsemble(ensemble_hp, None, [1.0, 1.0], [-1.0, 0.0], [{"seed": 1}, {"seed": 2}])
    finally:
        ensemble.NeuralNetworkEnsemble.engine_class = old
