"""GPU: ensembles of the adr kind (pinn_native.AdrEnsemble, include/pinn_hip.h pinn_adr_ens_create; k_fused20d<PDE_ADR_ENS>): K members
of one float64 net, each with its own six coefficients, on shared or per-member point sets with periodic pairs.  The
yardstick is a solo Engine(pde="adr", dtype="f64") on kernel path 7 -- existing code, held against the numpy oracle by
tests/test_gpu_adr.py -- and every comparison with it is == / np.array_equal: member k must be bit-identical to an Engine
given member k's weights, coefficients and points with the same calls.  One case is held against the numpy oracle
(tests/helpers/adr_ref.py) directly, with test_gpu_adr.py's float64 tolerances."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import adr_ref  # noqa: E402

pytestmark = pytest.mark.gpu

LB, UB = np.array([-1.0, 0.0]), np.array([1.0, 1.0])
COEFFS = [adr_ref.COEFF_SETS["allen_cahn"], adr_ref.COEFF_SETS["fisher_kpp"], adr_ref.COEFF_SETS["burgers"]]
N_0, N_B = 100, 7
EINVAL, EUNSUPPORTED = -1, -5


def _layers(H):
    return [2] + [20] * H + [1]


def _weights(layers, seed):
    """a glorot draw plus 0.05 * standard_normal: biases non-zero, every member another vector"""
    from oracle import init
    w = init.glorot_flat(layers)
    return w + 0.05 * np.random.RandomState(seed).standard_normal(w.size)


def _set(n_f, n_0, n_b, seed):
    """(X_f, X_u, u, X_lo, X_hi): collocation points, initial data u(x, 0) = x^2 cos(pi x), wall pairs at common times"""
    rs = np.random.RandomState(seed)
    X_f = LB + (UB - LB) * rs.uniform(size=(n_f, 2))
    x0 = rs.uniform(-1, 1, n_0)
    X_u, u = np.column_stack([x0, np.zeros(n_0)]), (x0 * x0 * np.cos(np.pi * x0)).reshape(-1, 1)
    tb = rs.uniform(0, 1, n_b)
    return X_f, X_u, u, np.column_stack([np.full(n_b, -1.0), tb]), np.column_stack([np.full(n_b, 1.0), tb])


def _solo(layers, coeffs, s, w):
    from pinn_native import Engine
    X_f, X_u, u, X_lo, X_hi = s
    eng = Engine(layers, LB, UB, pde="adr", dtype="f64")
    eng.set_pde_params(*coeffs)
    eng.set_collocation(X_f)
    if len(X_u):
        eng.set_data(X_u, u)
    if len(X_lo):
        eng.set_boundary(X_lo, X_hi)
    eng.set_weights(w)
    assert eng.kernel_path() == 7
    return eng


def _ensemble(layers, coeffs, sets, W):
    """sets: one tuple (shared point sets) or a list of K tuples (one set per member)"""
    from pinn_native import AdrEnsemble
    K = len(W)
    ens = AdrEnsemble(layers, LB, UB, K)
    X_f, X_u, u, X_lo, X_hi = sets if isinstance(sets, tuple) else [np.stack(c) for c in zip(*sets)]
    ens.set_collocation(X_f)
    if X_u.shape[-2]:
        ens.set_data(X_u, u)
    if X_lo.shape[-2]:
        ens.set_boundary(X_lo, X_hi)
    ens.set_pde_params(np.asarray(coeffs, dtype=np.float64))
    ens.set_weights(W)
    return ens


def _check_members(ens, layers, coeffs, sets, W, members=None, tag=()):
    """loss, gradient and all three terms of the listed members equal a solo engine's -> (losses, grads, terms)"""
    losses, grads, terms = ens.loss_grad()
    for k in (range(len(W)) if members is None else members):
        s = sets if isinstance(sets, tuple) else sets[k]
        eng = _solo(layers, coeffs[k], s, W[k])
        l, g, t = eng.loss_grad()
        eng.close()
        assert losses[k] == l and np.array_equal(grads[k], g) and np.array_equal(terms[k], t), tag + (k,)
    return losses, grads, terms


# ---- loss, gradient, terms: both launch plans (34 tiles: one per workgroup; 259 tiles > 256 CUs: tile loop) ----------------
@pytest.mark.parametrize("n_f", [2048, 16400])
@pytest.mark.parametrize("H", [4, 6, 8])
def test_shared_sets_member_coefficients_equal_solo(H, n_f):
    K, layers = 3, _layers(H)
    s = _set(n_f, N_0, N_B, 3)
    W = np.stack([_weights(layers, 100 + k) for k in range(K)])
    ens = _ensemble(layers, COEFFS, s, W)
    assert np.array_equal(ens.get_pde_params(), np.asarray(COEFFS))
    losses, _, terms = _check_members(ens, layers, COEFFS, s, W, tag=(H, n_f))
    assert np.all(terms[:, 2] > 0)
    # the rows are really read per member: member 0's weights with member 1's coefficients give another loss
    W2 = W.copy()
    W2[1] = W[0]
    ens.set_weights(W2)
    l2 = ens.loss_grad(want_grad=False)[0]
    assert l2[0] == losses[0] and l2[1] != losses[0]
    ens.close()


@pytest.mark.parametrize("n_f", [2048, 16400])
@pytest.mark.parametrize("H", [4, 6, 8])
def test_per_member_sets_equal_solo(H, n_f):
    K, layers = 3, _layers(H)
    sets = [_set(n_f, N_0, N_B, 10 + k) for k in range(K)]
    W = np.stack([_weights(layers, 200 + k) for k in range(K)])
    ens = _ensemble(layers, COEFFS, sets, W)
    losses, _, terms = _check_members(ens, layers, COEFFS, sets, W, tag=(H, n_f))
    assert np.all(terms[:, 2] > 0)
    # the sets really differ: member 0's weights and coefficients on member 1's set give another loss
    W2 = W.copy()
    W2[1] = W[0]
    ens.set_weights(W2)
    ens.set_pde_params(np.asarray([COEFFS[0], COEFFS[0], COEFFS[2]]))
    l2 = ens.loss_grad(want_grad=False)[0]
    assert l2[0] == losses[0] and l2[1] != losses[0]
    ens.close()


# ---- the pair block ends inside a wave, on a wave boundary (16 points), on a tile boundary (64 points); no pairs and no data --
@pytest.mark.parametrize("per_member", [False, True])
@pytest.mark.parametrize("n_b", [1, 8, 32, 0])
def test_pair_block_edges(n_b, per_member):
    K, layers, n_0 = 3, _layers(4), (N_0 if n_b else 0)
    sets = [_set(2048, n_0, n_b, 20 + k) for k in range(K)]
    W = np.stack([_weights(layers, 300 + k) for k in range(K)])
    ens = _ensemble(layers, COEFFS, sets if per_member else sets[0], W)
    _, _, terms = _check_members(ens, layers, COEFFS, sets if per_member else sets[0], W, tag=(n_b, per_member))
    if n_b:
        assert np.all(terms[:, 2] > 0)
    else:                                             # collocation only
        assert np.all(terms[:, 1] == 0.0) and np.all(terms[:, 2] == 0.0) and np.all(terms[:, 0] > 0)
    ens.close()


# ---- member count: one member, and the last row of the coefficient table ----------------------------------------------------
@pytest.mark.parametrize("K", [1, 64])
def test_member_count(K):
    layers = _layers(4)
    s = _set(256, N_0, N_B, 30)
    rs = np.random.RandomState(31)
    coeffs = [list(np.asarray(COEFFS[k % 3]) * (1.0 + 0.01 * k) + [0.0, 0.0, 0.0, 0.0, 0.001 * k, 0.0]) for k in range(K)]
    W = np.stack([_weights(layers, int(rs.randint(1 << 30))) for k in range(K)])
    ens = _ensemble(layers, coeffs, s, W)
    assert ens.n_members == K
    _check_members(ens, layers, coeffs, s, W, members=sorted({0, K // 2 - 1 if K > 1 else 0, K - 1}), tag=(K,))
    ens.close()


# ---- not only self-consistency: the numpy oracle, test_gpu_adr.py's float64 tolerances ------------------------------------
def test_members_match_the_numpy_oracle():
    K, layers = 3, _layers(8)
    sets = [_set(2048, N_0, N_B, 40 + k) for k in range(K)]
    W = np.stack([_weights(layers, 400 + k) for k in range(K)])
    ens = _ensemble(layers, COEFFS, sets, W)
    losses, grads, terms = ens.loss_grad()
    ens.close()
    for k in range(K):
        X_f, X_u, u, X_lo, X_hi = sets[k]
        lo, go, ex = adr_ref.adr_loss_grad(W[k], layers, LB, UB, X_f, X_u, u, X_lo, X_hi, COEFFS[k])
        d_loss, d_grad = abs(losses[k] - lo) / lo, np.max(np.abs(grads[k] - go)) / np.max(np.abs(go))
        print("adr ensemble member %d: loss %.2e grad %.2e" % (k, d_loss, d_grad))
        assert d_loss < 1e-12 and d_grad < 1e-11, k
        assert abs(terms[k, 2] - ex["mse_b"]) < 1e-11 * lo and terms[k, 2] > 0, k


# ---- training: Adam with a learning rate per member, then L-BFGS; a member that starts from NaN leaves the others alone ---
def _train(ens, lr):
    ens.adam_init(lr, 0.9, 0.999, 1e-7)
    L = ens.adam_run(50)
    ens.lbfgs_begin(30, 0.8, 50, np.finfo(float).eps)
    logs = ens.lbfgs_run(30)
    return L, logs, ens.get_weights()


def test_training_equals_solo_and_a_nan_member_stays_alone():
    K, layers = 3, _layers(4)
    s = _set(2048, N_0, N_B, 50)
    W = np.stack([_weights(layers, 500 + k) for k in range(K)])
    lr = np.array([0.03, 0.01, 0.02])
    ens = _ensemble(layers, COEFFS, s, W)
    L, logs, Wf = _train(ens, lr)
    assert np.all(ens.status()[1] == 0)
    ens.close()
    for k in range(K):
        eng = _solo(layers, COEFFS[k], s, W[k])
        eng.adam_init(lr[k], 0.9, 0.999, 1e-7)
        assert np.array_equal(eng.adam_run(50), L[:, k]), k
        eng.lbfgs_begin(30, 0.8, 50, np.finfo(float).eps)
        it, ls, done = eng.lbfgs_collect(eng.lbfgs_enqueue(30))
        assert np.array_equal(it, logs[0][k]) and np.array_equal(ls, logs[1][k]) and done == logs[2][k], k
        assert np.array_equal(eng.get_weights(), Wf[k]), k
        eng.close()
    W_bad = W.copy()
    W_bad[1] = np.nan
    ens = _ensemble(layers, COEFFS, s, W_bad)
    Lb, logs_b, Wb = _train(ens, lr)
    bad = ens.status()[1]
    ens.close()
    assert bad[1] != 0 and bad[0] == 0 and bad[2] == 0
    for k in (0, 2):
        assert np.array_equal(Lb[:, k], L[:, k]) and np.array_equal(Wb[k], Wf[k]), k
        assert np.array_equal(logs_b[0][k], logs[0][k]) and np.array_equal(logs_b[1][k], logs[1][k]), k


# ---- device LHS with a seed and pairs per member ------------------------------------------------------------------------------
def test_device_lhs_per_member_equals_solo():
    K, layers, n = 3, _layers(4), 2048
    seeds = np.array([11, 2 ** 40 + 3, 977], dtype=np.uint64)
    sets = [_set(n, N_0, N_B, 60 + k) for k in range(K)]
    W = np.stack([_weights(layers, 600 + k) for k in range(K)])
    ens = _ensemble(layers, COEFFS, sets, W)
    for draw in range(2):                              # a first draw (sets rebuilt), then a redraw in place
        sd = seeds + np.uint64(draw)
        ens.lhs_collocation(n, sd)
        losses, grads, terms = ens.loss_grad()
        drawn = []
        for k in range(K):
            eng = _solo(layers, COEFFS[k], sets[k], W[k])
            eng.lhs_collocation(n, int(sd[k]))
            l, g, t = eng.loss_grad()
            drawn.append((eng.get_collocation(),) + sets[k][1:])
            eng.close()
            assert losses[k] == l and np.array_equal(grads[k], g) and np.array_equal(terms[k], t), (draw, k)
        # member k's set is the solo engine's: its points, handed over as arrays, give the same bits
        ref = _ensemble(layers, COEFFS, drawn, W)
        lr_, gr_, _ = ref.loss_grad()
        ref.close()
        assert np.array_equal(lr_, losses) and np.array_equal(gr_, grads), draw
    ens.close()


# ---- the drop-in surface ------------------------------------------------------------------------------------------------------
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


def test_ensemble_fit_equals_solo_neuralnetwork_fits(monkeypatch):
    import neuralnetwork
    from ensemble import NeuralNetworkEnsemble
    monkeypatch.setenv("PINN_NO_PLOT", "1")
    monkeypatch.setattr(sys, "argv", ["inf_cont_allen_cahn.py"])     # (the script module reads an hp file from argv)
    sys.path.insert(0, os.path.join(PKG, "1d-allen-cahn"))
    import inf_cont_allen_cahn
    hp = {"layers": _layers(4), "tf_epochs": 12, "tf_lr": 0.03, "tf_b1": 0.9, "tf_eps": None, "nt_epochs": 8,
          "nt_lr": 0.8, "nt_ncorr": 50, "log_frequency": 5, "dtype": "f64"}
    X_f, X_u, u, X_lo, X_hi = _set(2048, N_0, N_B, 70)
    members = [{"seed": 20, "adr": COEFFS[0]}, {"seed": 21, "adr": COEFFS[1], "tf_lr": 0.01}]
    neuralnetwork.set_seed(1234)
    ens = NeuralNetworkEnsemble(hp, _Recorder(hp["log_frequency"]), UB, LB, members, pde="adr")
    ens.set_collocation(X_f)
    ens._set_boundary(X_lo, X_hi)
    ens.fit(X_u, u)
    Wf = ens.get_weights()
    assert np.array_equal(ens._engine.get_pde_params(), np.asarray(COEFFS[:2]))
    for k, m in enumerate(members):
        rec = _Recorder(hp["log_frequency"])
        mhp = {key: v for key, v in dict(hp, **m).items() if key != "adr"}
        pinn = inf_cont_allen_cahn.AllenCahnInformedNN(mhp, rec, X_f, X_lo, X_hi, UB, LB, coeffs=m["adr"])
        pinn.fit(X_u, u)
        assert np.array_equal(pinn.get_weights(), Wf[k]), k
        assert [l for _, l in rec.tf] == ens.adam_losses[:, k].tolist(), k
        it, ls = ens.nt_log[k]
        assert [i for i, _ in rec.nt] == it.tolist() and [l for _, l in rec.nt] == ls.tolist(), k
        pinn._engine.close()


# ---- refusals leave the ensemble as it was; a Burgers ensemble beside it is untouched ---------------------------------------
def _code(fn, *args):
    from pinn_native import PinnNativeError
    with pytest.raises(PinnNativeError) as e:
        fn(*args)
    return int(re.search(r"\(code (-?\d+)\)", str(e.value)).group(1))


def test_refusals_and_separation():
    import pinn_native
    lib = pinn_native.load()
    K, layers = 3, _layers(4)
    s = _set(2048, N_0, N_B, 80)
    W = np.stack([_weights(layers, 800 + k) for k in range(K)])
    ens = _ensemble(layers, COEFFS, s, W)
    before = ens.loss_grad()

    def unchanged():
        after = ens.loss_grad()
        return all(np.array_equal(a, b) for a, b in zip(before, after)) and np.array_equal(ens.get_pde_params(), COEFFS)

    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))   # noqa: E731
    five, bad6 = np.ones(5), np.array([0.0, 0.0, np.inf, 0.0, 0.0, 0.0])
    rows_bad = np.asarray(COEFFS, dtype=np.float64).copy()
    rows_bad[2, 4] = np.nan
    assert lib.pinn_ens_set_pde_params(ens._h, dp(five), 5) == EINVAL and unchanged()
    assert lib.pinn_ens_set_pde_params(ens._h, dp(bad6), 6) == EINVAL and unchanged()
    assert lib.pinn_adr_ensk_set_params(ens._h, dp(rows_bad), K) == EINVAL and unchanged()
    assert lib.pinn_adr_ensk_set_params(ens._h, dp(np.ones((K + 1, 6))), K + 1) == EINVAL and unchanged()
    assert lib.pinn_adr_ens_get_params(ens._h, dp(np.ones((K + 1, 6))), K + 1) == EINVAL
    assert lib.pinn_ensk_set_pde_params(ens._h, dp(np.full(K, 0.01)), K) == EUNSUPPORTED and unchanged()
    assert _code(ens.set_boundary, np.zeros((K, 3, 2)), np.zeros((K, 3, 2)), 2) == EINVAL and unchanged()   # n_total < n
    # the old constructor keeps refusing the adr kinds, the new one bad counts and shapes
    for pde in ("adr", "adr_ide"):
        with pytest.raises(pinn_native.PinnNativeError, match="ensembles support Burgers"):
            pinn_native.Ensemble(layers, LB, UB, 2, pde=pde)
    assert _code(pinn_native.AdrEnsemble, layers, LB, UB, 65) == EINVAL
    assert _code(pinn_native.AdrEnsemble, [2, 20, 20, 20, 1], LB, UB, 2) == EUNSUPPORTED
    assert unchanged()
    # a Burgers ensemble built in the same process: the adr calls are refused, and it still equals its solo engine
    nu = 0.01 / np.pi
    bur = pinn_native.Ensemble(layers, LB, UB, 2)
    bur.set_collocation(s[0])
    bur.set_data(s[1], s[2])
    bur.set_pde_params(nu)
    bur.set_weights(W[:2])
    x = np.zeros((2, 3, 2))
    assert lib.pinn_adr_ens_set_boundary(bur._h, dp(x), dp(x), 3, 3) == EUNSUPPORTED
    assert lib.pinn_adr_ensk_set_boundary(bur._h, dp(x), dp(x), 3, 3) == EUNSUPPORTED
    assert lib.pinn_adr_ensk_set_params(bur._h, dp(np.ones((2, 6))), 2) == EUNSUPPORTED
    assert lib.pinn_adr_ens_get_params(bur._h, dp(np.ones((2, 6))), 2) == EUNSUPPORTED
    lb_, gb_, _ = bur.loss_grad()
    bur.close()
    for k in range(2):
        eng = pinn_native.Engine(layers, LB, UB, pde="burgers", dtype="f64")
        eng.set_collocation(s[0])
        eng.set_data(s[1], s[2])
        eng.set_pde_params(nu)
        eng.set_weights(W[k])
        l, g, _ = eng.loss_grad()
        eng.close()
        assert lb_[k] == l and np.array_equal(gb_[k], g), k
    assert unchanged()
    ens.close()


# ---- the script, in a fresh process ------------------------------------------------------------------------------------------
def test_ens_cont_allen_cahn_script(tmp_path):
    import json
    hp = {"members": [{"seed": 1}, {"seed": 2, "adr": [0.0, 0.0, 2e-4, -4.0, 0.0, 4.0]}],
          "N_0": 64, "N_b": 16, "N_f": 1024, "layers": _layers(4), "tf_epochs": 6, "nt_epochs": 4, "log_frequency": 3,
          "solver_modes": 512, "solver_substeps": 10}
    path = tmp_path / "hp.json"
    path.write_text(json.dumps(hp))
    env = dict(os.environ, PINN_NO_PLOT="1")
    res = subprocess.run([sys.executable, os.path.join(PKG, "1d-allen-cahn", "ens_cont_allen_cahn.py"), str(path)],
                         cwd=PKG, env=env, capture_output=True, text=True, timeout=240)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    errs = [float(m) for m in re.findall(r"^member +\d+ .*error = ([0-9.eE+-]+)", res.stdout, flags=re.M)]
    assert len(errs) == 2 and np.all(np.isfinite(errs)), res.stdout[-2000:]
