"""GPU: self-adaptive point weights (include/pinn_hip.h pinn_sa_*, the SAW variants of csrc/kernels_fused20d.h) against the
plain kernel and the numpy restatement (tests/helpers/sa_ref.py): unit weights give the plain kernel's bits (loss, gradient,
Adam, L-BFGS), random weights give the restatement's loss and gradient, Adam trajectories of theta and lambda follow the
restatement, nothing but an Adam step moves the weights, set replacement resets them, refusals leave the context usable,
and the Burgers script trains with them reproducibly.  Depths 4, 6 and 8; N_f = 10^4 (one tile per workgroup) and 4 x 10^4
(the tile loop)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import sa_ref  # noqa: E402

pytestmark = pytest.mark.gpu

NU = 0.01 / np.pi
LB, UB = np.array([-1.0, 0.0]), np.array([1.0, 0.99])
DEPTHS = [4, 6, 8]
SIZES = [10000, 40000]


def _layers(H):
    return [2] + [20] * H + [1]


def _sets(n_f, n_u=100, seed=0):
    rs = np.random.RandomState(seed)
    X_f = np.column_stack([rs.uniform(-1, 1, n_f), rs.uniform(0, 0.99, n_f)])
    X_u = np.column_stack([rs.uniform(-1, 1, n_u), rs.uniform(0, 0.99, n_u)])
    u = -np.sin(np.pi * X_u[:, :1]) * (1.0 - X_u[:, 1:2])
    return X_f, X_u, u


def _engine(H, n_f, seed=0, w=None, n_u=100):
    import pinn_native
    from oracle import init
    X_f, X_u, u = _sets(n_f, n_u=n_u, seed=seed)
    eng = pinn_native.Engine(_layers(H), LB, UB, pde="burgers", dtype="f64")
    assert eng.kernel_path() == 7
    eng.set_collocation(X_f)
    eng.set_data(X_u, u)
    eng.set_pde_params(NU)
    eng.set_weights(init.glorot_flat(_layers(H)) if w is None else w)
    eng.adam_init(1e-3, 0.9, 0.999, 1e-7)
    return eng, (X_f, X_u, u)


def _unit(eng):
    eng.sa_set_weights(np.ones(eng.n_u), np.ones(eng.n_f))


@pytest.mark.parametrize("n_f", SIZES)
@pytest.mark.parametrize("H", DEPTHS)
def test_unit_weights_give_the_plain_kernels_bits(H, n_f):
    plain, _ = _engine(H, n_f)
    sa, _ = _engine(H, n_f)
    _unit(sa)
    sa.sa_adam_init(0.0)
    a, b = plain.loss_grad(), sa.loss_grad()
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    la, lb_ = plain.adam_run(20), sa.adam_run(20)
    assert np.array_equal(la, lb_) and np.array_equal(plain.get_weights(), sa.get_weights())
    for e in (plain, sa):
        e.lbfgs_begin(10, 0.8, 50, np.finfo(float).eps)
    ra, rb = plain.lbfgs_run(10), sa.lbfgs_run(10)
    assert np.array_equal(ra[1], rb[1]) and np.array_equal(plain.get_weights(), sa.get_weights())
    lu, lf = sa.sa_get_weights()
    assert np.all(lu == 1.0) and np.all(lf == 1.0)
    plain.close(); sa.close()


@pytest.mark.parametrize("n_f", SIZES)
@pytest.mark.parametrize("H", DEPTHS)
def test_random_weights_match_the_restatement(H, n_f):
    eng, (X_f, X_u, u) = _engine(H, n_f)
    rs = np.random.RandomState(H + n_f)
    lam_u, lam_f = rs.uniform(0.5, 2.0, X_u.shape[0]), rs.uniform(0.5, 2.0, n_f)
    eng.sa_set_weights(lam_u, lam_f)
    loss, grad, terms = eng.loss_grad()
    lo, go, (mf, mu), _, _ = sa_ref.loss_grad(eng.get_weights(), _layers(H), LB, UB, X_f, X_u, u, NU, lam_u, lam_f)
    assert abs(loss - lo) <= 1e-12 * lo
    assert np.max(np.abs(grad - go)) <= 1e-11 * np.max(np.abs(go))
    assert abs(terms[0] - mf) <= 1e-12 * mf and abs(terms[1] - mu) <= 1e-12 * mu
    got_u, got_f = eng.sa_get_weights()
    assert np.array_equal(got_u, lam_u) and np.array_equal(got_f, lam_f)
    eng.close()


@pytest.mark.parametrize("H", DEPTHS)
def test_adam_trajectories_of_theta_and_lambda_follow_the_restatement(H):
    eng, (X_f, X_u, u) = _engine(H, 2000)
    w0 = eng.get_weights()
    rs = np.random.RandomState(H)
    lam_u, lam_f = rs.uniform(0.5, 2.0, X_u.shape[0]), rs.uniform(0.5, 2.0, 2000)
    eng.sa_set_weights(lam_u, lam_f)
    eng.sa_adam_init(0.05)
    losses = eng.adam_run(50)
    w, lu, lf, lr = sa_ref.adam(w0, lam_u, lam_f, 50, _layers(H), LB, UB, X_f, X_u, u, NU, 1e-3, 0.05)
    got_u, got_f = eng.sa_get_weights()
    assert np.max(np.abs(eng.get_weights() - w)) <= 1e-8
    assert np.max(np.abs(got_u - lu)) <= 1e-8 and np.max(np.abs(got_f - lf)) <= 1e-8
    assert np.max(np.abs(losses - lr) / lr) <= 1e-8
    assert np.max(np.abs(got_f - lam_f)) > 1e-4                     # the weights did move (ascent)
    eng.close()


@pytest.mark.parametrize("n_f", SIZES)
def test_only_adam_moves_the_weights_and_disable_restores_plain_bits(n_f):
    H = 8
    eng, (X_f, X_u, u) = _engine(H, n_f)
    plain, _ = _engine(H, n_f)
    rs = np.random.RandomState(7)
    lam_u, lam_f = rs.uniform(0.5, 2.0, X_u.shape[0]), rs.uniform(0.5, 2.0, n_f)
    eng.sa_set_weights(lam_u, lam_f)
    eng.sa_adam_init(0.01)
    eng.loss_grad()
    eng.lbfgs_begin(5, 0.8, 50, np.finfo(float).eps)
    eng.lbfgs_run(5)
    eng.predict(X_f[:100])
    eng.residual()
    got_u, got_f = eng.sa_get_weights()
    assert np.array_equal(got_u, lam_u) and np.array_equal(got_f, lam_f)
    eng.adam_run(3)
    moved_u, moved_f = eng.sa_get_weights()
    assert not np.array_equal(moved_f, lam_f)
    eng.sa_disable()
    plain.set_weights(eng.get_weights())
    a, b = plain.loss_grad(), eng.loss_grad()
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    eng.close(); plain.close()


def test_new_adam_constants_rewrite_the_header_and_keep_weights_and_moments():
    """Two contexts alike (4 x 20, N_u = 5, N_f = 70: two 64-point tiles, the second ragged, one tile per workgroup), ascent on.
    After 3 steps both get pinn_adam_init with the constants they had; the second gets other (beta1, beta2, eps) first, reads
    its weights (which brings the array's header up to date) and then the old constants again, so its header is rewritten twice
    before the next step.  Network weights and all lambdas stay equal bit for bit after every step: lambda, m and v of every
    point survived the rewrites.  One tile per workgroup only: nothing here forces another launch plan.  Last, one step with
    the second context under the other constants: its lambdas must then differ, so the header it wrote is the one the
    kernel reads."""
    k, consts = 3, (1e-3, 0.9, 0.999, 1e-7)
    rs = np.random.RandomState(3)
    lam_u, lam_f = rs.uniform(0.5, 2.0, 5), rs.uniform(0.5, 2.0, 70)
    a, b = _engine(4, 70, n_u=5)[0], _engine(4, 70, n_u=5)[0]
    for e in (a, b):
        e.sa_set_weights(lam_u, lam_f)
        e.sa_adam_init(0.05)

    def step_and_compare():
        for _ in range(k):
            assert np.array_equal(a.adam_run(1), b.adam_run(1))
            assert np.array_equal(a.get_weights(), b.get_weights())
            assert all(np.array_equal(x, y) for x, y in zip(a.sa_get_weights(), b.sa_get_weights()))

    step_and_compare()
    assert not np.array_equal(a.sa_get_weights()[1], lam_f)         # the ascent is on
    a.adam_init(*consts)
    b.adam_init(1e-3, 0.8, 0.99, 1e-5)
    assert all(np.array_equal(x, y) for x, y in zip(a.sa_get_weights(), b.sa_get_weights()))
    b.adam_init(*consts)
    step_and_compare()
    a.adam_init(*consts)
    b.adam_init(1e-3, 0.8, 0.99, 1e-5)
    a.adam_run(1), b.adam_run(1)
    assert not any(np.array_equal(x, y) for x, y in zip(a.sa_get_weights(), b.sa_get_weights()))
    a.close(); b.close()


def test_replacing_a_set_resets_its_class_and_refusals_leave_the_context_usable():
    import pinn_native
    eng, (X_f, X_u, u) = _engine(8, 10000)
    rs = np.random.RandomState(9)
    lam_u, lam_f = rs.uniform(0.5, 2.0, X_u.shape[0]), rs.uniform(0.5, 2.0, 10000)
    eng.sa_set_weights(lam_u, lam_f)
    # refusals: wrong counts, non-finite weights, bad lr, another kernel path -- nothing changes
    for bad in (lambda: eng.sa_set_weights(lam_u[:-1], lam_f), lambda: eng.sa_set_weights(lam_u, np.full(10000, np.nan)),
                lambda: eng.sa_adam_init(-1.0), lambda: eng.sa_adam_init(float("inf")), lambda: eng.set_kernel_path(4)):
        with pytest.raises(pinn_native.PinnNativeError):
            bad()
    assert eng.kernel_path() == 7
    got_u, got_f = eng.sa_get_weights()
    assert np.array_equal(got_u, lam_u) and np.array_equal(got_f, lam_f)
    eng.loss_grad()
    # new data: data weights back to 1, collocation weights kept (and re-placed behind a data set of another size)
    X_u2, u2 = X_u[:60], u[:60]
    eng.set_data(X_u2, u2)
    got_u, got_f = eng.sa_get_weights()
    assert np.all(got_u == 1.0) and got_u.shape == (60,) and np.array_equal(got_f, lam_f)
    lo, _, _, _, _ = sa_ref.loss_grad(eng.get_weights(), _layers(8), LB, UB, X_f, X_u2, u2, NU, np.ones(60), lam_f)
    assert abs(eng.loss_grad()[0] - lo) <= 1e-12 * lo
    # a new collocation set (host, LHS, RAD): collocation weights back to 1, data weights kept
    eng.sa_set_weights(np.full(60, 2.0), lam_f)
    eng.set_collocation(X_f[:5000])
    got_u, got_f = eng.sa_get_weights()
    assert np.all(got_u == 2.0) and np.all(got_f == 1.0) and got_f.shape == (5000,)
    eng.sa_set_weights(np.full(60, 2.0), np.full(5000, 3.0))
    eng.lhs_collocation(5000, 11)                  # same count: an in-place redraw
    assert np.all(eng.sa_get_weights()[1] == 1.0)
    eng.sa_set_weights(np.full(60, 2.0), np.full(5000, 3.0))
    eng.rad_collocation(5000, 12, 20000)
    got_u, got_f = eng.sa_get_weights()
    assert np.all(got_u == 2.0) and np.all(got_f == 1.0)
    eng.close()
    # unsupported models are refused before any device work
    for kw in ({"pde": "burgers", "dtype": "f32"}, {"pde": "burgers_ide", "dtype": "f64"}):
        e = pinn_native.Engine(_layers(8), LB, UB, **kw)
        with pytest.raises(pinn_native.PinnNativeError, match="EUNSUPPORTED|code -5"):
            e.sa_set_weights(np.ones(0), np.ones(0))
        e.close()


_SCRIPT = r"""
import json, os, sys
import numpy as np
sys.argv = [sys.argv[0], sys.argv[1]]
out = sys.argv[1] + ".npz"
sys.path.insert(0, os.path.join(%(pkg)r, "1d-burgers"))
import runpy
g = runpy.run_path(os.path.join(%(pkg)r, "1d-burgers", "inf_cont_burgers.py"), run_name="sa_test")
hp = json.load(open(sys.argv[1]))
pinn = g["run"](hp)
lu, lf = pinn.get_sa_weights()
np.savez(out, w=pinn.get_weights(), lu=lu, lf=lf)
"""


def test_burgers_script_with_sa_is_reproducible(tmp_path):
    hp = {"N_u": 100, "N_f": 2000, "layers": [2, 20, 20, 20, 20, 20, 20, 20, 20, 1],
          "tf_epochs": 40, "tf_lr": 0.001, "tf_b1": 0.9, "tf_eps": None,
          "nt_epochs": 20, "nt_lr": 0.8, "nt_ncorr": 50, "log_frequency": 10, "sa_weights": True, "sa_lr": 0.01}
    runs = []
    for k in range(2):
        p = tmp_path / ("hp%d.json" % k)
        p.write_text(json.dumps(hp))
        env = dict(os.environ, PINN_NO_PLOT="1")
        r = subprocess.run([sys.executable, "-c", _SCRIPT % {"pkg": PKG}, str(p)], cwd=PKG, env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        runs.append((r.stdout, np.load(str(p) + ".npz")))
    (o0, a), (o1, b) = runs
    assert np.array_equal(a["w"], b["w"]) and np.array_equal(a["lu"], b["lu"]) and np.array_equal(a["lf"], b["lf"])
    assert o0.count("SA weights:") == 1 and "SA weights:" in o1
    assert np.all(np.isfinite(a["lf"])) and not np.all(a["lf"] == 1.0)
    end = [t for t in o0.splitlines() if t.startswith("Training finished")]
    assert end and np.isfinite(float(end[-1].split("error = ")[1].split()[0]))
