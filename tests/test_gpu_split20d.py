"""GPU: the split one-tile launch of kernel path 7 (k_split20d, csrc/kernels_fused20d_kernel.h) gives the bits of the plain one.

In a split launch helper workgroups recompute a tile's forward sweep and write the weight-gradient columns of the last hidden
and the output layer into the tile's gradient row; the tile's main workgroup leaves those blocks out.  Two float64 engines
per case, created with PINN_F64_SPLIT=0 and =1 (the switch is read when the engine is created), are compared with
np.array_equal -- loss, loss terms, gradient -- on
  Burgers inference (100 data points) and identification  x  depths 8 and 4  x  canonical weights and a copy scaled so that
  tanh arguments saturate  x  1, 2, 3 and 5 tiles of 64 points:
    1 tile   the helper's second tile is absent
    2 tiles  one pair; the last tile is ragged, so its pad lanes are in the helper's SECOND tile
    3 tiles  an odd count: the last helper serves one tile
    5 tiles  three helpers, the last tile ragged
  (Inference with one tile has 40 data points, not 100: 100 data points alone fill two tiles.)
20 evaluations of the split plan repeat the first bit for bit; 10 Adam + 10 L-BFGS steps at about 1 000 points end at the same
weights with the same L-BFGS loss log.  The gradient rows themselves have no reader in the ABI, so they are compared through
the reduced gradient only.  The launch plan is read through Engine.f64_split on small contexts: nothing large is run.
No tolerance anywhere."""
import contextlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LB, UB = np.array([-1.0, 0.0]), np.array([1.0, 1.0])
NU = 0.01 / np.pi
# tiles -> (collocation points, data points) of the inference sets / total points of the identification sets
POINTS = {1: (20, 40), 2: (20, 100), 3: (60, 100), 5: (177, 100)}


@contextlib.contextmanager
def split_env(value):
    old = os.environ.get("PINN_F64_SPLIT")
    if value is None:
        os.environ.pop("PINN_F64_SPLIT", None)
    else:
        os.environ["PINN_F64_SPLIT"] = value
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("PINN_F64_SPLIT", None)
        else:
            os.environ["PINN_F64_SPLIT"] = old


def point_sets(n_f, n_u, seed=11):
    rs = np.random.RandomState(seed)
    X_f = LB + (UB - LB) * rs.uniform(size=(n_f, 2))
    x0 = rs.uniform(-1, 1, n_u)
    X_u = np.column_stack([x0, rs.uniform(0, 1, n_u)])
    u = (-np.sin(np.pi * x0) * np.exp(-X_u[:, 1])).reshape(-1, 1)
    return X_f, X_u, u


def weights_for(eng, layers, kind):
    from oracle import init
    w = init.glorot_flat(layers)
    if kind == "saturating":
        w = 8.0 * w                              # some units' tanh rounds to +-1 at some points (max_preactivation)
    if eng.n_params == w.size + 2:
        w = np.concatenate([w, [0.0, -6.0]])
    assert eng.n_params == w.size
    return w


def max_preactivation(w, depth, X):
    """largest |z| over the hidden layers and the points X (flat layout: kernel [in][out], then bias, per layer)"""
    h, off, n_in, big = 2.0 * (X - LB) / (UB - LB) - 1.0, 0, 2, 0.0
    for _ in range(depth):
        W = w[off:off + n_in * 20].reshape(n_in, 20); off += n_in * 20
        z = h @ W + w[off:off + 20]; off += 20
        big, h, n_in = max(big, float(np.max(np.abs(z)))), np.tanh(z), 20
    return big


def make_engine(split, pde, depth, n_f, n_u, wkind="canonical"):
    from pinn_native import Engine
    layers = [2] + [20] * depth + [1]
    X_f, X_u, u = point_sets(n_f, n_u)
    with split_env(split):
        eng = Engine(layers, LB, UB, pde=pde, dtype="f64")
    if pde == "burgers":
        eng.set_collocation(X_f); eng.set_data(X_u, u); eng.set_pde_params(NU)
    else:                                            # identification: the data points carry the residual
        eng.set_data(np.vstack([X_f, X_u]), np.vstack([np.tanh(X_f[:, :1] - X_f[:, 1:]), u]))
    assert eng.kernel_path() == 7
    eng.set_weights(weights_for(eng, layers, wkind))
    return eng


@pytest.mark.parametrize("tiles", sorted(POINTS))
@pytest.mark.parametrize("wkind", ["canonical", "saturating"])
@pytest.mark.parametrize("depth", [8, 4])
@pytest.mark.parametrize("pde", ["burgers", "burgers_ide"])
def test_split_launch_gives_the_plain_launch_bit_for_bit(pde, depth, wkind, tiles):
    n_f, n_u = POINTS[tiles]
    assert (n_f + n_u + 63) // 64 == tiles and (tiles == 3 or (n_f + n_u) % 64 != 0)
    plain, split = (make_engine(s, pde, depth, n_f, n_u, wkind) for s in ("0", "1"))
    try:
        assert not plain.f64_split and split.f64_split and split.kernel_path() == 7
        l0, g0, t0 = plain.loss_grad()
        g0, t0 = np.array(g0, copy=True), np.array(t0, copy=True)
        l1, g1, t1 = split.loss_grad()
        g1, t1 = np.array(g1, copy=True), np.array(t1, copy=True)
        print("%s d%d %s %d tiles: loss %.17g / %.17g, %d of %d gradient entries differ" % (
            pde, depth, wkind, tiles, l0, l1, int(np.sum(g0 != g1)), g0.size))
        assert np.isfinite(l0) and np.all(np.isfinite(g0)) and np.any(g0 != 0.0)
        if wkind == "saturating":
            X = np.vstack(point_sets(n_f, n_u)[:2])
            assert max_preactivation(split.get_weights(), depth, X) > 19.0     # 1 - exp(-2 |z|) rounds to 1 there
        assert l0 == l1 and np.array_equal(t0, t1) and np.array_equal(g0, g1)
        for k in range(19):                                   # 20 evaluations of the split plan, the first included
            l2, g2, t2 = split.loss_grad()
            assert l2 == l1 and np.array_equal(g2, g1) and np.array_equal(t2, t1), "evaluation %d differs from the first" % (k + 2)
    finally:
        plain.close(); split.close()


@pytest.mark.parametrize("pde", ["burgers", "burgers_ide"])
def test_adam_and_lbfgs_trajectories_agree(pde):
    out = []
    for s in ("0", "1"):
        eng = make_engine(s, pde, 8, 900, 100)                # 1 000 points, 16 tiles, the last ragged
        try:
            assert eng.f64_split == (s == "1")
            eng.adam_init(1e-3, 0.9, 0.999, 1e-7)
            la = eng.adam_run(10)
            eng.lbfgs_begin(10, 0.8, 50, np.finfo(float).eps)
            it, ll, _ = eng.lbfgs_run(10)
            out.append((np.array(la, copy=True), np.array(it, copy=True), np.array(ll, copy=True), eng.get_weights().copy()))
        finally:
            eng.close()
    (la0, it0, ll0, w0), (la1, it1, ll1, w1) = out
    print("%s: %d L-BFGS entries, last loss %.17g / %.17g" % (pde, ll0.size, ll0[-1], ll1[-1]))
    assert ll0.size > 0 and np.all(np.isfinite(w0))
    assert np.array_equal(la0, la1) and np.array_equal(it0, it1) and np.array_equal(ll0, ll1) and np.array_equal(w0, w1)


def _plan(split, pde="burgers", n_points=200, depth=8):
    eng = make_engine(split, pde, depth, n_points - 100, 100)
    try:
        return eng.f64_split
    finally:
        eng.close()


def test_launch_plan_by_tile_count():
    import pinn_native
    n_cu = pinn_native.device_info(0)["compute_units"]
    fits = lambda tiles: tiles <= n_cu and tiles + (tiles + 1) // 2 <= n_cu
    # the headline set: 10 100 points = 158 tiles, 158 + 79 = 237 workgroups
    assert _plan(None, n_points=10100) == fits(158)
    if n_cu == 256:
        assert _plan(None, n_points=10100) and _plan("auto", n_points=10100)
    # the first tile count whose helpers find no compute units: no split, and a required split is refused
    tiles = next(t for t in range(1, n_cu + 2) if not fits(t))
    assert fits(tiles - 1) and _plan(None, n_points=64 * (tiles - 1))
    assert not _plan(None, n_points=64 * tiles)
    assert not _plan("0", n_points=200)
    with pytest.raises(pinn_native.PinnNativeError, match="PINN_F64_SPLIT=1"):
        _plan("1", n_points=64 * tiles)
    with split_env("yes"):
        with pytest.raises(pinn_native.PinnNativeError, match="PINN_F64_SPLIT"):
            pinn_native.Engine([2] + [20] * 8 + [1], LB, UB, pde="burgers", dtype="f64")


def test_no_split_for_an_ensemble_point_weights_or_the_adr_kind():
    import pinn_native
    layers = [2] + [20] * 8 + [1]
    X_f, X_u, u = point_sets(100, 100)
    with split_env("1"):                      # required where the kernel exists: these contexts have none, and say so
        ens = pinn_native.Ensemble(layers, LB, UB, 2, pde="burgers", dtype="f64")
        try:
            assert ens.f64_split is False
        finally:
            ens.close()
        saw = pinn_native.Engine(layers, LB, UB, pde="burgers", dtype="f64")
        try:
            saw.set_collocation(X_f); saw.set_data(X_u, u); saw.set_pde_params(NU)
            assert saw.f64_split
            saw.sa_set_weights(np.ones(100), np.ones(100))
            assert not saw.f64_split
            saw.sa_disable()
            assert saw.f64_split
        finally:
            saw.close()
        adr = pinn_native.Engine(layers, LB, UB, pde="adr", dtype="f64")
        try:
            adr.set_pde_params(0.0, 0.0, 1e-4, -5.0, 0.0, 5.0)
            adr.set_collocation(X_f); adr.set_data(X_u, u)
            adr.set_kernel_path(7)
            assert adr.kernel_path() == 7 and not adr.f64_split
        finally:
            adr.close()
        f32 = pinn_native.Engine(layers, LB, UB, pde="burgers", dtype="f32")
        try:
            f32.set_collocation(X_f); f32.set_data(X_u, u); f32.set_pde_params(NU)
            assert not f32.f64_split
        finally:
            f32.close()
