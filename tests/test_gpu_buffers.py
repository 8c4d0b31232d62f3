"""GPU: who owns the engine's memory (csrc/devbuf.h).  Every test takes pinn_debug_live_buffers -- the count and the bytes of
the device and pinned host blocks this process's engine owns -- before and after, and both numbers must be what they were:
whatever a context or an ensemble allocated on its way goes with it.  (The count is this process's own; the free memory of
the device belongs to everybody who shares it and is not looked at.)  Nets are [2, 20, 20, 1] on one or two 64-point tiles,
except where a feature exists from four hidden layers on only: kernel path 7, which the weighted losses and the ensembles
need.  Nothing here makes an allocation fail: that is tests/test_devbuf_host.py's, on the host."""
import gc
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import adr_ref  # noqa: E402

pytestmark = pytest.mark.gpu

LB, UB = np.array([-1.0, 0.0]), np.array([1.0, 1.0])
SMALL, PATH7 = [2, 20, 20, 1], [2, 20, 20, 20, 20, 1]
NU = 0.01 / np.pi
ADR = adr_ref.COEFF_SETS["allen_cahn"]
EPS = float(np.finfo(float).eps)


@pytest.fixture(autouse=True)
def live():
    """the before / after pair of every test in this file"""
    import pinn_native
    gc.collect()
    before = pinn_native.live_buffers()
    yield before
    gc.collect()
    assert pinn_native.live_buffers() == before, "blocks (count, bytes) left behind"


def _weights(layers, seed=0):
    from oracle import init
    w = init.glorot_flat(layers)
    return w + 0.05 * np.random.RandomState(seed).standard_normal(w.size)


def _points(n, seed):
    return LB + (UB - LB) * np.random.RandomState(seed).uniform(size=(n, 2))


def _data(n, seed):
    x0 = np.random.RandomState(seed).uniform(-1, 1, n)
    return np.column_stack([x0, np.zeros(n)]), -np.sin(np.pi * x0).reshape(-1, 1)


def _pairs(n, seed):
    tb = np.random.RandomState(seed).uniform(0, 1, n)
    return np.column_stack([np.full(n, -1.0), tb]), np.column_stack([np.full(n, 1.0), tb])


def _engine(layers, pde, dtype, n_f=40, n_u=20, n_b=0, seed=1):
    """a context with its sets and weights: n_u + n_f + 2 n_b points (60: one tile)"""
    from pinn_native import Engine
    eng = Engine(layers, LB, UB, pde=pde, dtype=dtype)
    if n_f:
        eng.set_collocation(_points(n_f, seed))
    eng.set_data(*_data(n_u, seed + 1))
    if n_b:
        eng.set_boundary(*_pairs(n_b, seed + 2))
    eng.set_pde_params(*(ADR if pde == "adr" else (NU,)))
    eng.set_weights(_weights(layers))
    return eng


def _walk(eng, foreign=True, source_at=None):
    """every optional buffer group a continuous context has: evaluation, Adam with recorded losses, L-BFGS, the evaluation
    caches, both residuals, the snapshot slots"""
    loss, grad, _ = eng.loss_grad()
    assert np.isfinite(loss) and np.all(np.isfinite(grad))
    eng.adam_init(1e-3)
    assert np.all(np.isfinite(eng.adam_run(3)))
    eng.weights_snapshot(1)
    eng.lbfgs_begin(4, 0.8, 5, EPS)
    assert np.all(np.isfinite(eng.lbfgs_run(2)[1]))
    X = _points(70, 9)                                  # 70 -> 128 evaluation slots
    up = eng.predict(X)
    assert np.all(np.isfinite(up)) and np.isfinite(eng.error_l2(X, up + 1.0))
    assert np.all(np.isfinite(eng.residual()))
    if foreign:
        assert np.all(np.isfinite(eng.residual_at(X, source=source_at(X) if source_at else None)))
    w = eng.get_weights()
    eng.weights_restore(1)
    assert not np.array_equal(eng.get_weights(), w)     # L-BFGS moved them since the snapshot


# ---- 1. every optional buffer group ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_burgers_context_gives_back_every_group(dtype, live):
    import pinn_native
    eng = _engine(SMALL, "burgers", dtype)
    _walk(eng)
    n, b = pinn_native.live_buffers()
    assert n > live[0] + 30 and b > live[1]             # (the counter counts: a walked context holds dozens of blocks)
    eng.close()


def test_adr_context_with_its_extras_gives_back_every_group():
    s = lambda X: 0.3 * np.sin(np.pi * X[:, 0]) * np.exp(-X[:, 1])      # noqa: E731
    for dtype in ("f64", "f32"):                        # Robin points, a source, coefficient fields: both dtypes, path 0
        eng = _engine(SMALL, "adr", dtype, n_f=40, n_u=14, n_b=3)
        Xw = np.column_stack([np.full(5, 1.0), np.linspace(0.1, 0.9, 5)])
        eng.set_robin(Xw, 0.5, 1.0, np.linspace(-0.2, 0.2, 5))
        eng.set_source(s(eng.get_collocation()))
        _walk(eng, source_at=s)
        assert np.all(np.isfinite(eng.robin_residual()))
        K = np.tile(np.asarray(ADR, dtype=np.float64), (40, 1))
        K[:, 2] *= 1.0 + 0.5 * np.linspace(0, 1, 40)
        eng.set_coef_fields(K)
        _walk(eng, foreign=False)                       # (no residual at foreign points while fields are present)
        eng.close()
    # per-point weights: float64 on kernel path 7, so four hidden layers
    eng = _engine(PATH7, "adr", "f64", n_f=40, n_u=14, n_b=3)
    assert eng.kernel_path() == 7
    eng.pw_set(np.full(14, 2.0), None, np.full(3, 0.5))
    eng.pw_adam_init(1e-2, 1e-2, 1e-2)
    _walk(eng)
    assert all(np.all(np.isfinite(a)) for a in eng.pw_get())
    eng.close()


def test_burgers_sa_lhs_and_rad_give_back_every_group():
    from pinn_native import Engine
    eng = Engine(PATH7, LB, UB, pde="burgers", dtype="f64")             # self-adaptive weights: kernel path 7
    eng.set_data(*_data(20, 2))
    eng.lhs_collocation(40, seed=11)
    eng.set_pde_params(NU)
    eng.set_weights(_weights(PATH7))
    assert eng.kernel_path() == 7
    eng.sa_set_weights(np.ones(20), np.ones(40))
    eng.sa_adam_init(1e-2)
    _walk(eng)
    assert all(np.all(np.isfinite(a)) for a in eng.sa_get_weights())
    eng.rad_collocation(40, seed=12, n_pool=200)                        # 200 -> 256 pool slots; the weights start over
    assert np.all(np.isfinite(eng.get_collocation())) and np.isfinite(eng.loss_grad()[0])
    eng.close()


def test_discrete_time_context_gives_back_every_group():
    from oracle import disc
    from pinn_native import Engine
    q, layers = 4, [1, 20, 20, 5]
    W_irk, _ = disc.irk_tables_like_reference(q)
    x0 = np.random.RandomState(0).uniform(-1, 1, (40, 1))
    sets = disc.inference_sets(x0, -np.sin(np.pi * x0), np.array([[-1.0], [1.0]]), 0.8, W_irk)
    eng = Engine(layers, [-1.0], [1.0], pde="burgers_disc", dtype="f64")
    for k, (x, t, M) in enumerate(sets):
        eng.disc_set_stage(k, x, t, M)
    eng.set_pde_params(NU)
    eng.set_weights(_weights(layers))
    loss, grad, _ = eng.loss_grad()
    assert np.isfinite(loss) and np.all(np.isfinite(grad))
    xs = np.linspace(-1, 1, 33)
    assert np.all(np.isfinite(eng.predict(xs))) and np.all(np.isfinite(eng.disc_predict(0, xs)))   # both modes
    eng.close()


# ---- 2. grow, shrink, grow: a kept, larger buffer changes nothing -----------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_grow_shrink_grow_equals_a_fresh_context(dtype):
    from pinn_native import Engine
    X_u, u = _data(20, 4)
    w0 = _weights(SMALL, 5)

    def stage(eng, X_f, n_corr, max_iter):
        """the set, an evaluation, two L-BFGS iterations from w0 -> (loss, gradient at w0, L-BFGS log, weights behind it)"""
        eng.set_collocation(X_f)
        eng.set_weights(w0)
        loss, grad, _ = eng.loss_grad()
        eng.lbfgs_begin(max_iter, 0.8, n_corr, EPS)
        log = eng.lbfgs_run(2)
        return loss, grad, log[1], eng.get_weights()

    def fresh():
        eng = Engine(SMALL, LB, UB, pde="burgers", dtype=dtype)
        eng.set_data(X_u, u)
        eng.set_pde_params(NU)
        return eng

    kept = fresh()
    for i, (n_f, n_corr, max_iter) in enumerate([(64, 5, 4), (192, 20, 40), (64, 5, 4), (256, 20, 40)]):
        X_f = _points(n_f, 20 + i)
        got = stage(kept, X_f, n_corr, max_iter)
        ref_eng = fresh()
        want = stage(ref_eng, X_f, n_corr, max_iter)
        ref_eng.close()
        assert got[0] == want[0] and np.array_equal(got[1], want[1]), (i, n_f)
        assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]), (i, n_f, "L-BFGS")
    kept.close()


# ---- 3. ensembles: members are views of the ensemble's blocks --------------------------------------------------------------
@pytest.mark.parametrize("per_member", [False, True])
@pytest.mark.parametrize("pde", ["burgers", "adr"])
def test_ensemble_gives_back_its_blocks_and_member_0_equals_solo(pde, per_member):
    from pinn_native import AdrEnsemble, Engine, Ensemble
    K, n_b = 3, (3 if pde == "adr" else 0)
    W = np.stack([_weights(PATH7, 30 + k) for k in range(K)])
    sets = [(_points(40, 40 + k),) + _data(14, 50 + k) + _pairs(n_b, 60 + k) for k in range(K if per_member else 1)]
    X_f, X_u, u, X_lo, X_hi = [np.stack(c) for c in zip(*sets)] if per_member else sets[0]
    ens = AdrEnsemble(PATH7, LB, UB, K) if pde == "adr" else Ensemble(PATH7, LB, UB, K, pde="burgers")
    ens.set_collocation(X_f)
    ens.set_data(X_u, u)
    if n_b:
        ens.set_boundary(X_lo, X_hi)
    ens.set_pde_params(*(ADR if pde == "adr" else (NU,)))
    ens.set_weights(W)
    losses, grads, _ = ens.loss_grad()
    ens.adam_init(1e-3)
    steps = ens.adam_run(2)
    W2 = ens.get_weights()
    ens.close()

    solo = Engine(PATH7, LB, UB, pde=pde, dtype="f64")
    solo.set_collocation(sets[0][0])
    solo.set_data(sets[0][1], sets[0][2])
    if n_b:
        solo.set_boundary(sets[0][3], sets[0][4])
    solo.set_pde_params(*(ADR if pde == "adr" else (NU,)))
    solo.set_weights(W[0])
    l, g, _ = solo.loss_grad()
    solo.adam_init(1e-3)
    s_steps = solo.adam_run(2)
    assert losses[0] == l and np.array_equal(grads[0], g)
    assert np.array_equal(steps[:, 0], s_steps) and np.array_equal(W2[0], solo.get_weights())
    solo.close()


# ---- 4. refusals after device work ------------------------------------------------------------------------------------------
def test_refused_ensemble_leaves_nothing(live):
    import pinn_native
    # (a width other than 20 has no kernel path 7; today the shape check in front of pinn_ens_create's device work answers, and
    #  the path refusal behind the base context in ens_build cannot be reached through the ABI -- the count holds either way)
    for cls, kw in ((pinn_native.Ensemble, {"pde": "burgers"}), (pinn_native.AdrEnsemble, {})):
        with pytest.raises(pinn_native.PinnNativeError):
            cls([2, 24, 24, 24, 24, 1], LB, UB, 3, **kw)
        assert pinn_native.live_buffers() == live


def test_context_destroyed_with_a_chunk_in_flight_leaves_nothing():
    eng = _engine(SMALL, "burgers", "f64")
    eng.adam_init(1e-3)
    eng.adam_enqueue(3)                                 # never collected: its pinned buffer and the ring go with the context
    eng.close()
