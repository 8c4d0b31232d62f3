"""GPU: ensembles (pinn_native.Ensemble / utils/ensemble.py, include/pinn_hip.h pinn_ens_*) against solo engines.  Every
comparison is np.array_equal: member k of an ensemble must be bit-identical to the same member trained alone (same
launch plan, same row order, same per-column arithmetic)."""
import json
import sys

import numpy as np
import pytest

from conftest import ensemble_accepts, golden, same_distribution_p

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


def _setup(eng, pde, n, data):
    X_u, u = data
    if pde == "burgers":
        eng.set_collocation(_points(n, 11))
        eng.set_data(X_u, u)
    else:                                   # identification: the residual lives at the data points
        X = _points(n, 12)
        eng.set_data(X, np.sin(np.pi * X[:, :1]) * np.exp(-X[:, 1:]))
    eng.set_pde_params(NU)


@pytest.fixture(scope="module")
def data():
    X = _points(100, 5)
    return X, -np.sin(np.pi * X[:, :1])


def _solo(layers, pde, n, data, w):
    import pinn_native
    eng = pinn_native.Engine(layers, LB, UB, pde=pde, dtype="f64")
    _setup(eng, pde, n, data)
    eng.set_weights(w)
    assert eng.kernel_path() == 7
    return eng


@pytest.mark.parametrize("n", [10000, 40000])          # one tile per workgroup / tile loop (627 tiles > 256 CUs)
@pytest.mark.parametrize("H", [4, 6, 8])
@pytest.mark.parametrize("pde", ["burgers", "burgers_ide"])
def test_ensemble_loss_grad_equals_solo(data, pde, H, n):
    import pinn_native
    K, layers, ide = 5, _layers(H), pde == "burgers_ide"
    W = np.stack([_weights(layers, 100 + k, ide) for k in range(K)])
    ens = pinn_native.Ensemble(layers, LB, UB, K, pde=pde)
    _setup(ens, pde, n, data)
    ens.set_weights(W)
    assert np.array_equal(ens.get_weights(), W)
    losses, grads, terms = ens.loss_grad()
    for k in range(K):
        eng = _solo(layers, pde, n, data, W[k])
        l, g, t = eng.loss_grad()
        assert losses[k] == l and np.array_equal(grads[k], g) and np.array_equal(terms[k], t), (pde, H, n, k)
        eng.close()
    assert len(set(losses.tolist())) == K                # the members are different networks
    ens.close()


def test_ensemble_adam_equals_solo(data):
    import pinn_native
    K, layers, steps = 5, _layers(8), 100
    lr = np.array([0.03, 0.01, 0.003, 0.02, 0.05])
    W = np.stack([_weights(layers, 200 + k, False) for k in range(K)])
    ens = pinn_native.Ensemble(layers, LB, UB, K)
    _setup(ens, "burgers", 10000, data)
    ens.set_weights(W)
    ens.adam_init(lr, 0.9, 0.999, 1e-7)
    L = np.concatenate([ens.adam_run(37), ens.adam_run(steps - 37)])
    Wf = ens.get_weights()
    assert L.shape == (steps, K)
    for k in range(K):
        eng = _solo(layers, "burgers", 10000, data, W[k])
        eng.adam_init(lr[k], 0.9, 0.999, 1e-7)
        assert np.array_equal(eng.adam_run(steps), L[:, k]), k
        assert np.array_equal(eng.get_weights(), Wf[k]), k
        eng.close()
    n_evals, bad = ens.status()
    assert np.all(n_evals == steps) and np.all(bad == 0)
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


def _default_hp():
    return dict(json.load(open(golden("burgers_band.json")))["hp"], dtype="f64")


def _solo_fit(hp, X_f, X_u, u, ub, lb):
    import inf_cont_burgers
    rec = _Recorder(hp["log_frequency"])
    pinn = inf_cont_burgers.BurgersInformedNN(hp, rec, X_f, ub, lb, nu=NU)
    pinn.fit(X_u, u)
    _, _, done = pinn._engine.lbfgs_run(0)
    return pinn, rec, done


def _ensemble(hp, members, X_f, ub, lb, logger=None):
    from ensemble import NeuralNetworkEnsemble
    ens = NeuralNetworkEnsemble(hp, logger or _Recorder(hp["log_frequency"]), ub, lb, members)
    ens.set_collocation(X_f)
    ens.set_pde_params(NU)
    return ens


@pytest.fixture(scope="module")
def default_sets(burgers_sets):
    r = burgers_sets(100, 10000)
    return r   # x, t, X, T, Exact_u, X_star, u_star, X_u, u, X_f, ub, lb


def test_ensemble_default_schedule_equals_solo_fits(default_sets, monkeypatch):
    import neuralnetwork
    monkeypatch.setenv("PINN_NO_PLOT", "1")
    monkeypatch.setattr(sys, "argv", ["inf_cont_burgers.py"])     # (the script module reads an hp file from argv)
    X_star, u_star, X_u, u, X_f, ub, lb = default_sets[5:]
    hp = _default_hp()
    members = [{"seed": 10 + k} for k in range(8)]
    members[2]["nt_epochs"] = 37                            # members that finish at other iterations
    members[5]["nt_epochs"] = 120
    members[6]["tf_lr"] = 0.01
    neuralnetwork.set_seed(1234)
    ens = _ensemble(hp, members, X_f, ub, lb)
    ens.fit(X_u, u)
    Wf, err = ens.get_weights(), ens.error_l2(X_star, u_star)
    up = ens.predict(X_star)
    assert np.all(ens.nt_done != 0)
    for k, m in enumerate(members):
        pinn, rec, done = _solo_fit(dict(hp, **m), X_f, X_u, u, ub, lb)
        assert np.array_equal(pinn.get_weights(), Wf[k]), k
        assert [l for _, l in rec.tf] == ens.adam_losses[:, k].tolist(), k
        it, ls = ens.nt_log[k]
        assert [i for i, _ in rec.nt] == it.tolist() and [l for _, l in rec.nt] == ls.tolist(), k
        assert done == ens.nt_done[k], (k, done, ens.nt_done[k])
        assert pinn.error_l2(X_star, u_star) == err[k], k
        assert np.array_equal(pinn.predict(X_star)[0], up[k]), k
    assert ens.nt_log[2][0][-1] <= 37 and ens.nt_log[5][0][-1] <= 120


def test_nonfinite_member_is_isolated(data):
    import pinn_native
    K, layers = 4, _layers(8)
    W = np.stack([_weights(layers, 300 + k, False) for k in range(K)])
    W[2, 5] = np.nan
    ens = pinn_native.Ensemble(layers, LB, UB, K)
    _setup(ens, "burgers", 10000, data)
    ens.set_weights(W)
    ens.adam_init(0.01)
    L = ens.adam_run(20)
    ens.lbfgs_begin(30, 0.8, 50, np.finfo(float).eps)
    logs = ens.lbfgs_run(30)
    Wf = ens.get_weights()
    n_evals, bad = ens.status()
    assert bad[2] == 1 and np.all(bad[[0, 1, 3]] == 0), bad
    assert np.all(np.isnan(L[:, 2]))
    for k in (0, 1, 3):
        eng = _solo(layers, "burgers", 10000, data, W[k])
        eng.adam_init(0.01)
        assert np.array_equal(eng.adam_run(20), L[:, k]), k
        eng.lbfgs_begin(30, 0.8, 50, np.finfo(float).eps)
        it, ls, done = eng.lbfgs_collect(eng.lbfgs_enqueue(30))      # (= lbfgs_run(30), log buffer sized by the wrapper)
        assert np.array_equal(it, logs[0][k]) and np.array_equal(ls, logs[1][k]) and done == logs[2][k], k
        assert np.array_equal(eng.get_weights(), Wf[k]), k
        assert eng.status() == (n_evals[k], 0), k
        eng.close()
    ens.close()


def test_band_members_as_one_ensemble(default_sets, monkeypatch, record):
    """the 25 init_scale members of burgers_band.json trained as ONE ensemble: every final error equals the solo engine's
    (the same runs test_gpu_end_to_end.py makes one after another), and the acceptance rules used there pass"""
    import neuralnetwork
    monkeypatch.setenv("PINN_NO_PLOT", "1")
    monkeypatch.setattr(sys, "argv", ["inf_cont_burgers.py"])
    X_star, u_star, X_u, u, X_f, ub, lb = default_sets[5:]
    b = json.load(open(golden("burgers_band.json")))
    hp = dict(b["hp"], dtype="f64")
    members = [{"init_scale": 1.0 + k * b["eps"]} for k in b["k_ulp"]]
    neuralnetwork.set_seed(1234)
    ens = _ensemble(hp, members, X_f, ub, lb)
    ens.fit(X_u, u)
    err = ens.error_l2(X_star, u_star)
    for i, m in enumerate(members):
        neuralnetwork.set_seed(1234)
        pinn, _, _ = _solo_fit(dict(hp, **m), X_f, X_u, u, ub, lb)
        assert pinn.error_l2(X_star, u_star) == err[i], (i, m)
    ref = [b["runs"][str(k)]["final_error"] for k in b["k_ulp"]]
    k0 = list(b["k_ulp"]).index(0)
    ok, lo, hi = ensemble_accepts([v["final_error"] for v in b["runs"].values()], float(err[k0]))
    p = same_distribution_p(err, ref)
    record(members=len(members), err_k0=float(err[k0]), ens_min=lo, ens_max=hi, p_mannwhitney=p)
    assert ok, (err[k0], lo, hi)
    assert p >= 1e-3, (p, sorted(err), sorted(ref))
