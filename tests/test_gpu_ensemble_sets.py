"""GPU: ensembles with a point set and a viscosity per member (pinn_native.Ensemble set_* with [K, ...] arrays,
lhs_collocation; include/pinn_hip.h pinn_ensk_*; utils/ensemble.py "nu" / "resample_seed" / resample_every).  Every
comparison with a solo engine is np.array_equal: member k must be bit-identical to an Engine (or NeuralNetwork) given
member k's points, data, nu and seeds with the same calls."""
import json
import sys

import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu

LB, UB = np.array([-1.0, 0.0]), np.array([1.0, 0.99])
NU = 0.01 / np.pi


def _layers(H):
    return [2] + [20] * H + [1]


def _weights(layers, seed, ide):
    from oracle import init
    rs = np.random.RandomState(seed)
    w = init.glorot_flat(layers) * (1.0 + 0.1 * rs.standard_normal())
    if ide:
        w = np.concatenate([w, [0.1 * seed, -6.0 + 0.2 * seed]])
    return w


def _points(n, seed):
    rs = np.random.RandomState(seed)
    return np.column_stack([rs.uniform(LB[0], UB[0], n), rs.uniform(LB[1], UB[1], n)])


def _member_sets(K, pde, n, n_u=100):
    """member k's (X_f or None, X_u, u, nu): all different"""
    out = []
    for k in range(K):
        X_u = _points(n if pde == "burgers_ide" else n_u, 500 + k)
        u = np.sin(np.pi * X_u[:, :1]) * np.exp(-(1.0 + 0.1 * k) * X_u[:, 1:])
        X_f = None if pde == "burgers_ide" else _points(n, 600 + k)
        out.append((X_f, X_u, u, NU * (1.0 + 0.5 * k)))
    return out


def _solo(layers, pde, s, w):
    import pinn_native
    X_f, X_u, u, nu = s
    eng = pinn_native.Engine(layers, LB, UB, pde=pde, dtype="f64")
    if X_f is not None:
        eng.set_collocation(X_f)
    eng.set_data(X_u, u)
    eng.set_pde_params(nu)
    eng.set_weights(w)
    assert eng.kernel_path() == 7
    return eng


def _ensemble(layers, pde, sets, W):
    import pinn_native
    ens = pinn_native.Ensemble(layers, LB, UB, len(sets), pde=pde)
    if sets[0][0] is not None:
        ens.set_collocation(np.stack([s[0] for s in sets]))
    ens.set_data(np.stack([s[1] for s in sets]), np.stack([s[2] for s in sets]))
    ens.set_pde_params(np.array([s[3] for s in sets]))
    ens.set_weights(W)
    return ens


@pytest.mark.parametrize("n", [10000, 40000])          # one tile per workgroup / tile loop (627 tiles > 256 CUs)
@pytest.mark.parametrize("H", [4, 6, 8])
@pytest.mark.parametrize("pde", ["burgers", "burgers_ide"])
def test_per_member_sets_loss_grad_equal_solo(pde, H, n):
    K, layers, ide = 3, _layers(H), pde == "burgers_ide"
    sets = _member_sets(K, pde, n)
    W = np.stack([_weights(layers, 100 + k, ide) for k in range(K)])
    ens = _ensemble(layers, pde, sets, W)
    losses, grads, terms = ens.loss_grad()
    for k in range(K):
        eng = _solo(layers, pde, sets[k], W[k])
        l, g, t = eng.loss_grad()
        assert losses[k] == l and np.array_equal(grads[k], g) and np.array_equal(terms[k], t), (pde, H, n, k)
        eng.close()
    # the sets really differ: member 0's weights on member 1's set give another loss than on its own
    W2 = W.copy()
    W2[1] = W[0]
    ens.set_weights(W2)
    l2 = ens.loss_grad(want_grad=False)[0]
    assert l2[0] == losses[0] and l2[1] != losses[0]
    ens.close()


def test_per_member_training_equals_solo():
    K, layers = 4, _layers(8)
    sets = _member_sets(K, "burgers", 10000)
    W = np.stack([_weights(layers, 200 + k, False) for k in range(K)])
    lr = np.array([0.03, 0.01, 0.02, 0.03])
    ens = _ensemble(layers, "burgers", sets, W)
    ens.adam_init(lr, 0.9, 0.999, 1e-7)
    L = ens.adam_run(50)
    ens.lbfgs_begin(30, 0.8, 50, np.finfo(float).eps)
    logs = ens.lbfgs_run(30)
    Wf = ens.get_weights()
    for k in range(K):
        eng = _solo(layers, "burgers", sets[k], W[k])
        eng.adam_init(lr[k], 0.9, 0.999, 1e-7)
        assert np.array_equal(eng.adam_run(50), L[:, k]), k
        eng.lbfgs_begin(30, 0.8, 50, np.finfo(float).eps)
        it, ls, done = eng.lbfgs_collect(eng.lbfgs_enqueue(30))
        assert np.array_equal(it, logs[0][k]) and np.array_equal(ls, logs[1][k]) and done == logs[2][k], k
        assert np.array_equal(eng.get_weights(), Wf[k]), k
        eng.close()
    ens.close()


def test_device_lhs_per_member_equals_solo_and_oracle():
    from oracle import lhs, pde
    K, layers, n = 4, _layers(8), 10000
    seeds = np.array([11, 2 ** 40 + 3, 977, 5], dtype=np.uint64)
    sets = _member_sets(K, "burgers", n)
    W = np.stack([_weights(layers, 300 + k, False) for k in range(K)])
    ens = _ensemble(layers, "burgers", sets, W)
    for draw in range(2):                              # a first draw (sets rebuilt), then a redraw in place
        s = seeds + np.uint64(draw)
        ens.lhs_collocation(n, s)
        losses, grads, _ = ens.loss_grad()
        for k in range(K):
            eng = _solo(layers, "burgers", sets[k], W[k])
            eng.lhs_collocation(n, int(s[k]))
            l, g, _ = eng.loss_grad()
            assert losses[k] == l and np.array_equal(grads[k], g), (draw, k)
            eng.close()
    # a shard [first, first + count) of each member's design, against the numpy restatement through the loss
    first, count, n_design = 1000, 6000, 20000
    ens.lhs_collocation(n_design, seeds, first=first, count=count)
    losses, grads, _ = ens.loss_grad()
    for k in range(K):
        X_f = lhs.lhs_points(n_design, int(seeds[k]), LB, UB, first=first, count=count)[0]
        lo, go, _ = pde.burgers_loss_grad(W[k], layers, LB, UB, X_f, sets[k][1], sets[k][2], sets[k][3],
                                          n_f_total=n_design)
        assert abs(losses[k] - lo) <= 1e-12 * abs(lo), k
        assert np.max(np.abs(grads[k] - go)) <= 1e-11 * np.max(np.abs(go)), k
    ens.close()


def test_mixed_modes_broadcast_equals_per_member_copies():
    K, layers, n = 3, _layers(6), 10000
    sets = _member_sets(K, "burgers", n)
    X_f = _points(n, 77)
    W = np.stack([_weights(layers, 400 + k, False) for k in range(K)])
    import pinn_native
    a = pinn_native.Ensemble(layers, LB, UB, K)
    a.set_data(np.stack([s[1] for s in sets]), np.stack([s[2] for s in sets]))
    a.set_collocation(X_f)                              # shared, broadcast in per-member mode
    a.set_pde_params(NU)
    a.set_weights(W)
    b = pinn_native.Ensemble(layers, LB, UB, K)
    b.set_collocation(np.stack([X_f] * K))
    b.set_data(np.stack([s[1] for s in sets]), np.stack([s[2] for s in sets]))
    b.set_pde_params(np.full(K, NU))
    b.set_weights(W)
    la, ga, ta = a.loss_grad()
    lb_, gb, tb = b.loss_grad()
    assert np.array_equal(la, lb_) and np.array_equal(ga, gb) and np.array_equal(ta, tb)
    # and a per-member nu on shared point sets = solo engines at those nus
    c = pinn_native.Ensemble(layers, LB, UB, K)
    c.set_collocation(X_f)
    c.set_data(sets[0][1], sets[0][2])
    c.set_pde_params(np.array([s[3] for s in sets]))
    c.set_weights(W)
    lc, gc, _ = c.loss_grad()
    for k in range(K):
        eng = _solo(layers, "burgers", (X_f, sets[0][1], sets[0][2], sets[k][3]), W[k])
        l, g, _ = eng.loss_grad()
        assert lc[k] == l and np.array_equal(gc[k], g), k
        eng.close()
    for e in (a, b, c):
        e.close()


def test_per_member_nu_matches_oracle():
    from oracle import pde
    K, layers = 3, _layers(8)
    sets = _member_sets(K, "burgers", 4096)
    W = np.stack([_weights(layers, 700 + k, False) for k in range(K)])
    ens = _ensemble(layers, "burgers", sets, W)
    losses, grads, _ = ens.loss_grad()
    for k in range(K):
        X_f, X_u, u, nu = sets[k]
        assert nu != NU or k == 0
        lo, go, _ = pde.burgers_loss_grad(W[k], layers, LB, UB, X_f, X_u, u, nu)
        assert abs(losses[k] - lo) <= 1e-12 * abs(lo), k
        assert np.max(np.abs(grads[k] - go)) <= 1e-11 * np.max(np.abs(go)), k
    ens.close()


class _Recorder(object):
    """Logger stand-in: keeps every entry NeuralNetwork.fit logs"""
    quiet = True

    def __init__(self, frequency=10):
        self.frequency, self.tf, self.nt = frequency, [], []

    def log_train_start(self, model, model_description=False):
        pass

    def log_train_opt(self, name):
        pass

    def log_train_epoch(self, epoch, loss, custom="", is_iter=False):
        (self.nt if is_iter else self.tf).append((int(epoch), float(loss)))

    def log_train_end(self, epoch, custom=""):
        pass

    def get_elapsed(self):
        return ""


def test_ensemble_fit_with_member_sets_nu_and_resampling_equals_solo_fits(burgers_sets, monkeypatch):
    import neuralnetwork
    from ensemble import NeuralNetworkEnsemble
    monkeypatch.setenv("PINN_NO_PLOT", "1")
    monkeypatch.setattr(sys, "argv", ["inf_cont_burgers.py"])     # (the script module reads an hp file from argv)
    import inf_cont_burgers
    X_star, u_star, X_u, u, X_f, ub, lb = burgers_sets(100, 10000)[5:]
    hp = dict(json.load(open(golden("burgers_band.json")))["hp"], dtype="f64", tf_epochs=60, nt_epochs=30,
              resample_every=25)
    K = 4
    members = [{"seed": 20 + k, "nu": NU * (1.0 + 0.25 * k), "resample_seed": 900 + 7 * k} for k in range(K)]
    members[1]["tf_lr"] = 0.01
    pick = [np.random.RandomState(k).choice(X_star.shape[0], 100, replace=False) for k in range(K)]
    X_uk, u_uk = np.stack([X_star[p] for p in pick]), np.stack([u_star[p] for p in pick])
    neuralnetwork.set_seed(1234)
    ens = NeuralNetworkEnsemble(hp, _Recorder(hp["log_frequency"]), ub, lb, members)
    ens.set_collocation(X_f)
    ens.set_pde_params(NU)
    ens.fit(X_uk, u_uk)
    Wf = ens.get_weights()
    for k, m in enumerate(members):
        rec = _Recorder(hp["log_frequency"])
        pinn = inf_cont_burgers.BurgersInformedNN(dict(hp, **m), rec, X_f, ub, lb, nu=m["nu"])
        pinn.fit(X_uk[k], u_uk[k])
        assert np.array_equal(pinn.get_weights(), Wf[k]), k
        assert [l for _, l in rec.tf] == ens.adam_losses[:, k].tolist(), k
        it, ls = ens.nt_log[k]
        assert [i for i, _ in rec.nt] == it.tolist() and [l for _, l in rec.nt] == ls.tolist(), k
        pinn._engine.close()
