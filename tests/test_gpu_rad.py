"""GPU: residual-based adaptive collocation (include/pinn_hip.h pinn_rad_collocation, csrc/kernels_rad.h) against the numpy
restatement (tests/helpers/rad_ref.py) fed with Engine.residual_at at the oracle's pool: bit-exact draws for Burgers and
Schrodinger in float64 and float32 on every forward path, slices of one design, the loss and gradient on the drawn set,
re-draws, survival across re-assembly, NaN weights, refusals on a live context, NeuralNetwork.fit with hp["resample"] =
"rad", and two data-parallel ranks of the Burgers script."""
import os
import sys

import numpy as np
import pytest

from conftest import PKG

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import rad_ref  # noqa: E402

pytestmark = pytest.mark.gpu

NU = 0.01 / np.pi
B_LB, B_UB = np.array([-1.0, 0.0]), np.array([1.0, 0.99])
S_LB, S_UB = np.array([-5.0, 0.0]), np.array([5.0, np.pi / 2])
CASES = {                                   # name: (layers, pde, dtype) -- the forward path in the comment
    "burgers20_f64": ([2] + [20] * 8 + [1], "burgers", "f64"),          # k_fwd20d
    "burgers20_f32": ([2] + [20] * 8 + [1], "burgers", "f32"),          # k_fwd20f
    "schrodinger100_f64": ([2] + [100] * 4 + [2], "schrodinger", "f64"),   # k_t16_fwd, eight tiles
    "schrodinger100_f32": ([2] + [100] * 4 + [2], "schrodinger", "f32"),
    "burgers32_f64": ([2, 32, 32, 32, 1], "burgers", "f64"),            # chunked k_t16_fwd, four tiles
}
_ENGINES = {}


def _bounds(pde):
    return (S_LB, S_UB) if pde == "schrodinger" else (B_LB, B_UB)


def _fresh(name, adam_steps=20):
    """an engine of this case with data, a host collocation set and the weights after `adam_steps` Adam steps"""
    import pinn_native
    from oracle import init
    layers, pde, dtype = CASES[name]
    lb, ub = _bounds(pde)
    eng = pinn_native.Engine(layers, lb, ub, pde=pde, dtype=dtype)
    rs = np.random.RandomState(3)
    if pde == "schrodinger":
        X0 = np.column_stack([rs.uniform(-5, 5, 50), np.zeros(50)])
        eng.set_data(X0, np.column_stack([2.0 / np.cosh(X0[:, 0]), np.zeros(50)]))
        tb = rs.uniform(0, np.pi / 2, 50)
        eng.set_boundary(np.column_stack([np.full(50, -5.0), tb]), np.column_stack([np.full(50, 5.0), tb]))
    else:
        Xu = np.column_stack([rs.uniform(-1, 1, 100), np.zeros(100)])
        eng.set_data(Xu, -np.sin(np.pi * Xu[:, 0:1]))
        eng.set_pde_params(NU)
    eng.set_collocation(lb + (ub - lb) * rs.uniform(size=(2000, 2)))
    eng.set_weights(init.glorot_flat(layers))
    eng.adam_init(0.003)
    if adam_steps:
        eng.adam_run(adam_steps)
    return eng


def _engine(name):
    if name not in _ENGINES:
        _ENGINES[name] = _fresh(name)
    return _ENGINES[name]


_POOLS = {}


def _pool(name, n_pool, seed):
    """P: the n_pool-point design pinn_lhs_collocation(n_pool, seed) draws on a context of this case, read back from the
    device and equal to oracle.lhs.lhs_points (rounded to float32 for float32 contexts) on both boxes.  (On the Schrodinger
    x range it was not until k_lhs_fill stopped contracting lb + span * v into one fused multiply-add: that shows where
    span * v is inexact and lb != 0; tests/test_gpu_boxes.py.)"""
    import pinn_native
    layers, pde, dtype = CASES[name]
    lb, ub = _bounds(pde)
    key = (pde, dtype)
    if key not in _POOLS:
        _POOLS[key] = pinn_native.Engine(layers, lb, ub, pde=pde, dtype=dtype)
    probe = _POOLS[key]
    probe.lhs_collocation(n_pool, seed)
    P = probe.get_collocation()
    assert np.array_equal(P, rad_ref.pool_points(n_pool, seed, lb, ub, dtype))
    return P


def _expected(eng, name, n_pool, seed, first, count, k, c):
    P = _pool(name, n_pool, seed)
    f = eng.residual_at(P)
    return rad_ref.rad_draw(P, f, seed, first, count, k, c)


@pytest.mark.parametrize("kc", [(1, 1.0), (2, 0.0), (4, 64.0)])
@pytest.mark.parametrize("n_pool", [1, 1000, 100037])
@pytest.mark.parametrize("name", sorted(CASES))
def test_draw_is_bit_exact_against_the_restatement(name, n_pool, kc):
    k, c = kc
    eng = _engine(name)
    seed = 0x5EED0000 + n_pool + 17 * k
    eng.rad_collocation(3000, seed, n_pool, k=k, c=c)
    got = eng.get_collocation()
    want, idx = _expected(eng, name, n_pool, seed, 0, 3000, k, c)
    assert got.shape == (3000, 2)
    assert np.array_equal(got, want), (name, n_pool, kc, int(np.sum(np.any(got != want, axis=1))))
    if n_pool > 1 and (k, c) != (4, 64.0):
        assert len(np.unique(idx)) > 1


def test_slices_drawn_by_separate_calls_concatenate_to_the_full_draw():
    eng = _engine("burgers20_f64")
    eng.rad_collocation(10000, 99, 50000, k=2, c=0.5)
    full = eng.get_collocation()
    parts = []
    for lo, hi in ((0, 2500), (2500, 2501), (2501, 7000), (7000, 10000)):
        eng.rad_collocation(10000, 99, 50000, k=2, c=0.5, first=lo, count=hi - lo)
        parts.append(eng.get_collocation())
    assert np.array_equal(np.vstack(parts), full)
    want, _ = _expected(eng, "burgers20_f64", 50000, 99, 7000, 3000, 2, 0.5)
    assert np.array_equal(parts[-1], want)


@pytest.mark.parametrize("name", ["burgers20_f64", "burgers20_f32", "schrodinger100_f64"])
def test_the_drawn_set_is_what_is_trained_on(name):
    from oracle import pde as opde
    eng = _fresh(name)
    layers, pde, dtype = CASES[name]
    lb, ub = _bounds(pde)
    rs = np.random.RandomState(3)
    n_design = 3000
    eng.rad_collocation(n_design, 5, 20000, k=1, c=1.0, first=1000, count=2000)   # a slice: mean over n_design
    loss, grad, _ = eng.loss_grad()
    Xf = eng.get_collocation()
    w = eng.get_weights()
    if pde == "schrodinger":
        X0 = np.column_stack([rs.uniform(-5, 5, 50), np.zeros(50)])
        uv0 = np.column_stack([2.0 / np.cosh(X0[:, 0]), np.zeros(50)])
        tb = rs.uniform(0, np.pi / 2, 50)
        lo, go, _ = opde.schrodinger_loss_grad(w, layers, lb, ub, Xf, np.column_stack([np.full(50, -5.0), tb]),
                                               np.column_stack([np.full(50, 5.0), tb]), X0, uv0, n_f_total=n_design)
    else:
        Xu = np.column_stack([rs.uniform(-1, 1, 100), np.zeros(100)])
        lo, go, _ = opde.burgers_loss_grad(w, layers, lb, ub, Xf, Xu, -np.sin(np.pi * Xu[:, 0:1]), NU, n_f_total=n_design)
    tl, tg = (1e-12, 1e-11) if dtype == "f64" else (1e-5, 2e-5)
    assert abs(loss - lo) <= tl * max(1.0, abs(lo)), (loss, lo)
    assert np.max(np.abs(grad - go)) <= tg * np.max(np.abs(go))


def test_redraws_replacement_and_survival_across_reassembly():
    eng = _fresh("burgers20_f64")
    eng.rad_collocation(2000, 11, 20000)
    a = eng.get_collocation()
    eng.rad_collocation(2000, 11, 20000)
    assert np.array_equal(eng.get_collocation(), a)
    eng.rad_collocation(2000, 12, 20000)
    b = eng.get_collocation()
    assert not np.array_equal(a, b)
    # a re-assembly (new data set) keeps the drawn points, and training sees them
    rs = np.random.RandomState(8)
    Xu = np.column_stack([rs.uniform(-1, 1, 60), np.zeros(60)])
    eng.set_data(Xu, -np.sin(np.pi * Xu[:, 0:1]))
    assert np.array_equal(eng.get_collocation(), b)
    l1 = eng.loss_grad()[0]
    ref = _fresh("burgers20_f64", adam_steps=20)
    ref.set_data(Xu, -np.sin(np.pi * Xu[:, 0:1]))
    ref.set_collocation(b, n_total=2000)
    assert l1 == ref.loss_grad()[0]
    # a redraw of another size re-assembles; set_collocation and lhs_collocation replace the points
    eng.rad_collocation(2000, 12, 20000, first=0, count=700)
    assert np.array_equal(eng.get_collocation(), b[:700])
    host = np.column_stack([np.linspace(-1, 1, 300), np.linspace(0, 0.99, 300)])
    eng.set_collocation(host)
    assert np.array_equal(eng.get_collocation(), host)
    eng.rad_collocation(2000, 12, 20000)
    assert np.array_equal(eng.get_collocation(), b)
    eng.lhs_collocation(2000, 12)
    from oracle import lhs
    assert np.array_equal(eng.get_collocation(), lhs.lhs_points(2000, 12, B_LB, B_UB)[0])


@pytest.mark.parametrize("name", ["burgers20_f64", "schrodinger100_f32"])
def test_nan_weights_draw_uniformly_and_evaluation_caches_survive(name):
    layers, pde, dtype = CASES[name]
    lb, ub = _bounds(pde)
    eng = _fresh(name)
    grid = np.column_stack([np.repeat(np.linspace(lb[0], ub[0], 64), 40), np.tile(np.linspace(lb[1], ub[1], 40), 64)])
    ref = np.cos(grid[:, 0:1]) * np.ones((1, layers[-1]))
    e1, p1, r1 = eng.error_l2(grid, ref), eng.predict(grid), eng.residual_at(grid)
    eng.rad_collocation(5000, 21, 30000, k=2, c=0.25)
    e2, p2, r2 = eng.error_l2(grid, ref), eng.predict(grid), eng.residual_at(grid)
    assert e1 == e2 and np.array_equal(p1, p2) and np.array_equal(r1, r2)
    w = eng.get_weights()
    w[:] = np.nan
    eng.set_weights(w)
    eng.rad_collocation(5000, 21, 30000, k=2, c=0.25)
    got = eng.get_collocation()
    P = _pool(name, 30000, 21)
    want, idx = rad_ref.rad_draw(P, np.full((30000, layers[-1]), np.nan), 21, 0, 5000, 2, 0.25)
    assert np.array_equal(got, want)
    assert np.all(np.isfinite(got)) and np.all(got >= lb) and np.all(got <= ub)
    assert len(np.unique(idx)) > 4000                      # uniform over the pool: few repeats


def test_refusals_leave_the_set_and_the_context_intact():
    import pinn_native
    eng = _fresh("burgers20_f64")
    eng.rad_collocation(2000, 3, 10000)
    X0 = eng.get_collocation()
    l0 = eng.loss_grad()[0]
    bad = [dict(n_design=0), dict(first=1500, count=600), dict(first=-1), dict(n_pool=0), dict(n_pool=(1 << 24) + 1),
           dict(k=0), dict(k=5), dict(c=-1.0), dict(c=64.5), dict(c=float("nan")), dict(c=float("inf"))]
    for b in bad:
        args = dict(n_design=2000, seed=4, n_pool=10000, k=1, c=1.0, first=0, count=2000)
        args.update(b)
        rc = eng._lib.pinn_rad_collocation(eng._h, args["n_design"], args["first"], args["count"], args["n_pool"],
                                           args["seed"], args["k"], args["c"])
        assert rc == -1, (b, rc)
        assert np.array_equal(eng.get_collocation(), X0), b
        assert eng.loss_grad()[0] == l0, b
    eng.rad_collocation(2000, 3, 1 << 24, k=4, c=64.0)          # the limits themselves are accepted
    assert eng.get_collocation().shape == (2000, 2)
    # models without a collocation set: PINN_EUNSUPPORTED
    ide = pinn_native.Engine([2, 20, 20, 1], B_LB, B_UB, pde="burgers_ide", dtype="f64")
    disc = pinn_native.Engine([1, 20, 20, 5], [-1.0], [1.0], pde="burgers_disc", dtype="f64")
    for e in (ide, disc):
        assert e._lib.pinn_rad_collocation(e._h, 100, 0, 100, 1000, 1, 1, 1.0) == -5
        with pytest.raises(pinn_native.PinnNativeError):
            e.rad_collocation(100, 1, 1000)
    assert ide.n_params > 0 and disc.n_params > 0


# ---- NeuralNetwork.fit --------------------------------------------------------------------------------------------------
def _fit_hp():
    return {"layers": [2] + [20] * 8 + [1], "tf_epochs": 30, "tf_lr": 0.003, "tf_b1": 0.9, "tf_eps": None,
            "nt_epochs": 0, "nt_lr": 0.8, "nt_ncorr": 50, "log_frequency": 10, "dtype": "f64", "seed": 5,
            "resample": "rad", "resample_every": 10, "resample_seed": 300}


def _fit_data():
    rs = np.random.RandomState(4)
    Xu = np.column_stack([rs.uniform(-1, 1, 100), np.zeros(100)])
    Xf = B_LB + (B_UB - B_LB) * rs.uniform(size=(2000, 2))
    return Xu, -np.sin(np.pi * Xu[:, 0:1]), Xf


def _model(hp):
    p = os.path.join(PKG, "utils")
    if p not in sys.path:
        sys.path.insert(0, p)
    import neuralnetwork
    from logger import Logger

    class _Log(Logger):
        def log_train_epoch(self, epoch, loss, custom="", is_iter=False):
            self.record.append((bool(is_iter), int(epoch), float(loss)))

        def log_train_start(self, *a, **k): pass
        def log_train_opt(self, *a, **k): pass
        def log_train_end(self, *a, **k): pass

    log = _Log(hp)
    log.record = []
    Xu, u, Xf = _fit_data()
    nn = neuralnetwork.NeuralNetwork(hp, log, B_UB, B_LB)
    nn._set_collocation(Xf)
    nn._engine.set_pde_params(NU)
    return nn, Xu, u


def test_fit_with_rad_is_reproducible_and_replays_through_engine_calls():
    runs = []
    for _ in range(2):
        nn, Xu, u = _model(_fit_hp())
        nn.fit(Xu, u)
        runs.append((nn.logger.record, nn._engine.get_weights(), nn._engine.get_collocation()))
    assert runs[0][0] == runs[1][0] and len(runs[0][0]) == 30
    assert np.array_equal(runs[0][1], runs[1][1]) and np.array_equal(runs[0][2], runs[1][2])
    # the replay: the same chunks and redraws through Engine calls
    nn, Xu, u = _model(_fit_hp())
    eng = nn._engine
    nn._bind(Xu, u)
    losses, w20 = [], None
    for epoch in (0, 10, 20):
        if epoch:
            if epoch == 20:
                w20 = eng.get_weights()
            eng.rad_collocation(2000, 300 + epoch, 20000, k=1, c=1.0)
        losses += list(eng.adam_run(1)) + list(eng.adam_run(9))
    assert [l for _, _, l in runs[0][0]] == losses
    assert np.array_equal(eng.get_weights(), runs[0][1])
    # the final set is the restatement's draw at the epoch-20 weights
    probe = _fresh("burgers20_f64", adam_steps=0)
    probe.set_weights(w20)
    want, _ = _expected(probe, "burgers20_f64", 20000, 320, 0, 2000, 1, 1.0)
    assert np.array_equal(runs[0][2], want)
    # and RAD moved the set: it differs from the host set and from a uniform LHS redraw
    assert not np.array_equal(runs[0][2], _fit_data()[2])


def test_two_ranks_draw_one_adaptive_design(tmp_path, record):
    from test_gpu_dp_scripts import _launch, _compare
    hp = {"N_u": 100, "N_f": 10000, "layers": [2, 20, 20, 20, 20, 20, 20, 20, 20, 1],
          "tf_epochs": 30, "tf_lr": 0.03, "tf_b1": 0.9, "tf_eps": None,
          "nt_epochs": 20, "nt_lr": 0.8, "nt_ncorr": 50, "log_frequency": 5, "dtype": "f64",
          "resample": "rad", "resample_every": 10, "rad_pool": 50000, "rad_k": 2, "rad_c": 0.5}
    script = os.path.join(PKG, "1d-burgers", "inf_cont_burgers.py")
    single = _launch(script, hp, tmp_path / "one", 1)
    ranks = _launch(script, hp, tmp_path / "two", 2)
    assert [r["n_f_local"] for r in ranks] == [5000, 5000]
    _compare(single, ranks, record, "inf_cont_burgers_rad")
