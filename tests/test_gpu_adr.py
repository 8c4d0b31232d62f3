"""GPU: the advection-diffusion-reaction residual kind (PINN_PDE_ADR, pde="adr") against the numpy oracle
tests/helpers/adr_ref.py (pinned on the CPU by tests/test_adr_host.py).

  f = u_t + (a0 + a1 u) u_x - nu u_xx + r1 u + r2 u^2 + r3 u^3,  loss = mean f^2 + mean (u - u*)^2 + periodic pairs

Float64 on the generic kernels (path 0) and on k_fused20d's six new variants (path 7), float32 on path 0.  The shape-generic
MFMA sweeps (paths 4 to 6) are refused for this kind, as are paths 1, 2, 3 and 8.  Tolerances are those of
tests/test_gpu_parity.py: float64 loss 1e-12, gradient 1e-11, residual 1e-10; float32 1e-5 / 2e-5."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG, golden

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
sys.path.insert(0, os.path.join(PKG, "1d-allen-cahn"))
import adr_ref  # noqa: E402
import rad_ref  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = {"f64": dict(loss=1e-12, grad=1e-11, res=1e-10), "f32": dict(loss=1e-5, grad=2e-5, res=2e-4)}
LB, UB = np.array([-1.0, 0.0]), np.array([1.0, 1.0])
CONFIGS = [("f64", 0), ("f64", 7), ("f32", 0)]        # (dtype, kernel path)


def rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300)


def layers_of(depth, width=20):
    return [2] + [width] * depth + [1]


def weights(layers, seed=7):
    """a glorot draw plus 0.05 * standard_normal: biases non-zero"""
    from oracle import init
    w = init.glorot_flat(layers)
    return w + 0.05 * np.random.RandomState(seed).standard_normal(w.size)


def point_sets(N_f, n_0=512, n_b=50, n_wall=0, seed=3):
    """collocation points, initial data u(x, 0) = x^2 cos(pi x) (+ n_wall Dirichlet wall points), n_b wall pairs"""
    rs = np.random.RandomState(seed)
    X_f = LB + (UB - LB) * rs.uniform(size=(N_f, 2))
    x0 = rs.uniform(-1, 1, n_0)
    X_u = np.column_stack([x0, np.zeros(n_0)])
    u = (x0 * x0 * np.cos(np.pi * x0)).reshape(-1, 1)
    if n_wall:
        tw = rs.uniform(0, 1, n_wall)
        X_u = np.vstack([X_u, np.column_stack([np.where(np.arange(n_wall) % 2, 1.0, -1.0), tw])])
        u = np.vstack([u, -np.ones((n_wall, 1))])
    tb = rs.uniform(0, 1, n_b)
    X_lo, X_hi = np.column_stack([np.full(n_b, -1.0), tb]), np.column_stack([np.full(n_b, 1.0), tb])
    return X_f, X_u, u, X_lo, X_hi


def make(layers, dtype, path, coeffs, X_f, X_u=None, u=None, X_lo=None, X_hi=None, lb=LB, ub=UB):
    from pinn_native import Engine
    eng = Engine(layers, lb, ub, pde="adr", dtype=dtype)
    eng.set_pde_params(*coeffs)
    eng.set_collocation(X_f)
    if X_u is not None and len(X_u):
        eng.set_data(X_u, u)
    if X_lo is not None and len(X_lo):
        eng.set_boundary(X_lo, X_hi)
    eng.set_kernel_path(path)          # no skip: paths 0 and 7 must exist for every cell
    assert eng.kernel_path() == path
    return eng


def check_cell(record, tag, layers, dtype, path, coeffs, X_f, X_u, u, X_lo, X_hi):
    w = weights(layers)
    eng = make(layers, dtype, path, coeffs, X_f, X_u, u, X_lo, X_hi)
    eng.set_weights(w)
    loss, grad, terms = eng.loss_grad()
    f = eng.residual()
    eng.close()
    lo, go, ex = adr_ref.adr_loss_grad(w, layers, LB, UB, X_f, X_u, u, X_lo, X_hi, coeffs)
    tol = TOL[dtype]
    dev = dict(loss=abs(loss - lo) / lo, grad=rel(grad, go), res=rel(f, ex["f"]),
               t_f=abs(terms[0] - ex["mse_f"]) / lo, t_u=abs(terms[1] - ex["mse_u"]) / lo,
               t_b=abs(terms[2] - ex["mse_b"]) / lo)
    print("adr %s %s path %d: %s" % (tag, dtype, path, " ".join("%s %.2e" % kv for kv in sorted(dev.items()))))
    record(tag=tag, dtype=dtype, path=path, **dev)
    assert dev["loss"] < tol["loss"]
    assert dev["grad"] < tol["grad"]
    assert dev["res"] < tol["res"]
    # the three parts, in the order (residual, data, boundary); relative to the loss they add up to
    assert max(dev["t_f"], dev["t_u"], dev["t_b"]) < tol["loss"] * 10
    if X_lo is not None and len(X_lo):
        assert terms[2] > 0
    else:
        assert terms[2] == 0.0


# ---- 1a. kernel variants: depths x set sizes (one tile per workgroup up to 10 000, tile loop at 40 000) ---------------------
@pytest.mark.parametrize("dtype,path", CONFIGS)
@pytest.mark.parametrize("N_f", [2048, 10000, 40000])
@pytest.mark.parametrize("depth", [4, 6, 8])
def test_variants_depths_and_tile_plans(record, depth, N_f, dtype, path):
    X_f, X_u, u, X_lo, X_hi = point_sets(N_f)
    check_cell(record, "a:d%d:Nf%d" % (depth, N_f), layers_of(depth), dtype, path, adr_ref.ALLEN_CAHN, X_f, X_u, u, X_lo, X_hi)


# ---- 1b. equations x set kinds --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,path", CONFIGS)
@pytest.mark.parametrize("kind", ["data", "pairs+initial", "pairs+initial+walls"])
@pytest.mark.parametrize("name", sorted(adr_ref.COEFF_SETS))
def test_equations_and_set_kinds(record, name, kind, dtype, path):
    X_f, X_u, u, X_lo, X_hi = point_sets(10000, n_wall=100 if kind.endswith("walls") else 0)
    if kind == "data":
        X_lo = X_hi = None
    check_cell(record, "b:%s:%s" % (name, kind), layers_of(8), dtype, path, adr_ref.COEFF_SETS[name], X_f, X_u, u, X_lo, X_hi)


# ---- 1c. pair counts: the block ends inside a wave, on a wave boundary, on a tile boundary, several tiles in -----------------
@pytest.mark.parametrize("dtype,path", CONFIGS)
@pytest.mark.parametrize("N_f", [2048, 40000])
@pytest.mark.parametrize("n_b", [1, 7, 8, 50, 200, 1000])
def test_pair_counts(record, n_b, N_f, dtype, path):
    X_f, X_u, u, X_lo, X_hi = point_sets(N_f, n_b=n_b)
    check_cell(record, "c:nb%d:Nf%d" % (n_b, N_f), layers_of(8), dtype, path, adr_ref.ALLEN_CAHN, X_f, X_u, u, X_lo, X_hi)


def test_a_shape_off_the_fast_kernel_runs_on_the_generic_path(record):
    """width 33, depth 3, float64: the default path is 0 (path 7 is refused), pairs and data present"""
    import pinn_native
    layers = [2, 33, 33, 33, 1]
    X_f, X_u, u, X_lo, X_hi = point_sets(3000, n_0=100, n_b=33)
    from pinn_native import Engine
    eng = Engine(layers, LB, UB, pde="adr", dtype="f64")
    assert eng.kernel_path() == 0
    with pytest.raises(pinn_native.PinnNativeError):
        eng.set_kernel_path(7)
    eng.close()
    check_cell(record, "w33", layers, "f64", 0, adr_ref.ALL_NONZERO, X_f, X_u, u, X_lo, X_hi)


def test_default_path_is_the_fast_kernel_for_float64_width_20():
    from pinn_native import Engine
    for depth in (4, 6, 8):
        eng = Engine(layers_of(depth), LB, UB, pde="adr", dtype="f64")
        assert eng.kernel_path() == 7
        eng.close()
    for layers, dtype in ((layers_of(8), "f32"), (layers_of(5), "f64"), (layers_of(3, 100), "f64")):
        eng = Engine(layers, LB, UB, pde="adr", dtype=dtype)
        assert eng.kernel_path() == 0
        eng.close()


# ---- 2. Burgers coefficients against the reference-made fixtures ------------------------------------------------------------
@pytest.mark.parametrize("dtype,path", CONFIGS)
@pytest.mark.parametrize("tag,N_u,N_f", [("_small", 64, 2048), ("", 100, 10000)])
def test_burgers_coefficients_against_the_golden(burgers_sets, record, tag, N_u, N_f, dtype, path):
    g = np.load(golden("burgers_eval%s.npz" % tag))
    r = burgers_sets(N_u, N_f)
    X_u, u, X_f, ub, lb = r[7], r[8], r[9], r[10], r[11]
    eng = make(layers_of(8), dtype, path, adr_ref.BURGERS(float(g["nu"])), X_f, X_u, u, lb=lb, ub=ub)
    eng.set_weights(g["w0"])
    loss, grad, terms = eng.loss_grad()
    eng.close()
    tol = TOL[dtype]
    dl, dg = abs(loss - float(g["loss"])) / float(g["loss"]), rel(grad, g["grad"])
    record(tag=tag, dtype=dtype, path=path, loss=dl, grad=dg)
    assert dl < tol["loss"]
    assert dg < tol["grad"]
    assert abs(terms[1] - float(g["mse_u"])) / float(g["mse_u"]) < tol["loss"] * 10
    assert abs(terms[0] - float(g["mse_f"])) / float(g["mse_f"]) < tol["loss"] * 10
    assert terms[2] == 0.0


# ---- 3. one context, both paths; run-to-run bit equality ---------------------------------------------------------------------
@pytest.mark.parametrize("N_f", [10000, 40000])
def test_paths_share_one_assembly_and_results_are_bit_reproducible(record, N_f):
    layers = layers_of(8)
    X_f, X_u, u, X_lo, X_hi = point_sets(N_f, n_b=200)
    eng = make(layers, "f64", 7, adr_ref.ALLEN_CAHN, X_f, X_u, u, X_lo, X_hi)
    eng.set_weights(weights(layers))
    l7, g7, t7 = eng.loss_grad()
    l7b, g7b, t7b = eng.loss_grad()
    assert l7 == l7b and np.array_equal(g7, g7b) and np.array_equal(t7, t7b)
    eng.set_kernel_path(0)
    l0, g0, t0 = eng.loss_grad()
    l0b, g0b, t0b = eng.loss_grad()
    assert l0 == l0b and np.array_equal(g0, g0b) and np.array_equal(t0, t0b)
    eng.set_kernel_path(7)
    l7c, g7c, _ = eng.loss_grad()
    assert l7c == l7 and np.array_equal(g7c, g7)
    eng.close()
    record(N_f=N_f, loss=abs(l7 - l0) / abs(l0), grad=rel(g7, g0), t_b=abs(t7[2] - t0[2]) / abs(l0))
    assert abs(l7 - l0) / abs(l0) < 1e-12
    assert rel(g7, g0) < 1e-11
    assert t7[2] > 0 and abs(t7[2] - t0[2]) / abs(l0) < 1e-11


# ---- 4. trajectories --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", [0, 7])
def test_adam_and_lbfgs_trajectories(record, path):
    """30 Adam steps (lr 1e-3) and 25 L-BFGS iterations on the Allen-Cahn set (N_f = 2048, 50 pairs) against
    oracle.optim.Adam / oracle.optim.lbfgs driven by adr_ref, float64, at the 1e-8 the README states for trajectories."""
    from oracle import optim
    layers = layers_of(8)
    X_f, X_u, u, X_lo, X_hi = point_sets(2048)
    co = adr_ref.ALLEN_CAHN
    w0 = weights(layers)

    def fg(w):
        l, g, _ = adr_ref.adr_loss_grad(w, layers, LB, UB, X_f, X_u, u, X_lo, X_hi, co)
        return l, g

    # Adam
    eng = make(layers, "f64", path, co, X_f, X_u, u, X_lo, X_hi)
    eng.set_weights(w0)
    eng.adam_init(1e-3, 0.9, 0.999, 1e-7)
    losses = eng.adam_run(30)
    w_dev = eng.get_weights()
    opt, w, ref = optim.Adam(1e-3, 0.9, 0.999, 1e-7), w0.copy(), []
    for _ in range(30):
        l, g = fg(w)
        ref.append(l)
        w = opt.step(w, g)
    da, dw = float(np.max(np.abs(losses - np.array(ref)) / np.array(ref))), rel(w_dev, w)
    # L-BFGS from the same start
    eng.set_weights(w0)
    eng.lbfgs_begin(25, 0.8, 50, np.finfo(float).eps)
    lo_all, done = [], 0
    while not done:
        it, lo, done = eng.lbfgs_run(7)
        lo_all.extend(lo.tolist())
    w_model = eng.get_weights()
    eng.close()
    res = optim.lbfgs(fg, w0, 25, 0.8, 50)
    ref_l = np.array([l for _, l in res["logs"]])
    n = min(len(lo_all), len(ref_l))
    dl = float(np.max(np.abs(np.array(lo_all[:n]) - ref_l[:n]) / ref_l[:n]))
    dm = rel(w_model, res["x_model"])
    print("adr trajectories path %d: adam loss %.2e w %.2e | lbfgs loss %.2e w_model %.2e (%d logged)" % (path, da, dw, dl, dm, n))
    record(path=path, adam_loss=da, adam_w=dw, lbfgs_loss=dl, lbfgs_w_model=dm)
    assert n >= 20 and len(lo_all) == len(ref_l)
    assert da < 1e-8 and dw < 1e-8
    assert dl < 1e-8 and dm < 1e-8


# ---- 5. predict, error_l2, residual_at, adaptive redraws -----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_predict_error_and_residual_at(dtype):
    from oracle import mlp
    layers = layers_of(8)
    X_f, X_u, u, X_lo, X_hi = point_sets(2048)
    w = weights(layers)
    eng = make(layers, dtype, 0, adr_ref.ALLEN_CAHN, X_f, X_u, u, X_lo, X_hi)
    eng.set_weights(w)
    rs = np.random.RandomState(1)
    X = LB + (UB - LB) * rs.uniform(size=(5000, 2))
    want = mlp.forward_value(mlp.unpack(w, layers), X, LB, UB)
    got = eng.predict(X)
    assert np.max(np.abs(got - want)) <= (1e-12 if dtype == "f64" else 3e-6) * max(1.0, np.max(np.abs(want)))
    ref = np.sin(3 * X[:, 0:1]) * np.cos(X[:, 1:2])
    e = eng.error_l2(X, ref)
    e_np = np.linalg.norm(ref - got, 2) / np.linalg.norm(ref, 2)
    assert abs(e - e_np) / e_np < 1e-13
    f = eng.residual_at(X)
    f_ref = adr_ref.residual(w, layers, LB, UB, X, adr_ref.ALLEN_CAHN)
    assert rel(f, f_ref) < TOL[dtype]["res"]
    eng.close()


@pytest.mark.parametrize("kc", [(1, 1.0), (2, 0.0)])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_rad_collocation_draw_is_bit_exact_and_trained_on(dtype, kc):
    """as tests/test_gpu_rad.py checks pde 0: the draw equals the numpy restatement fed with residual_at at the pool, and the
    loss / gradient on the drawn set (a slice of a larger design) equal the oracle's"""
    k, c = kc
    layers = layers_of(8)
    X_f, X_u, u, X_lo, X_hi = point_sets(2000, n_0=100)
    eng = make(layers, dtype, 7 if dtype == "f64" else 0, adr_ref.ALLEN_CAHN, X_f, X_u, u, X_lo, X_hi)
    eng.set_weights(weights(layers))
    eng.adam_init(0.003)
    eng.adam_run(20)
    n_pool, seed = 20000, 0x5EED0000 + 17 * k
    P = rad_ref.pool_points(n_pool, seed, LB, UB, dtype)
    eng.rad_collocation(3000, seed, n_pool, k=k, c=c)
    got = eng.get_collocation()
    want, idx = rad_ref.rad_draw(P, eng.residual_at(P), seed, 0, 3000, k, c)
    assert got.shape == (3000, 2)
    assert np.array_equal(got, want)
    assert len(np.unique(idx)) > 1
    eng.rad_collocation(3000, seed, n_pool, k=k, c=c, first=1000, count=2000)
    Xs = eng.get_collocation()
    assert np.array_equal(Xs, want[1000:])
    loss, grad, _ = eng.loss_grad()
    w = eng.get_weights()
    lo, go, _ = adr_ref.adr_loss_grad(w, layers, LB, UB, Xs, X_u, u, X_lo, X_hi, adr_ref.ALLEN_CAHN, n_f_total=3000)
    eng.close()
    assert abs(loss - lo) <= TOL[dtype]["loss"] * max(1.0, abs(lo))
    assert rel(grad, go) < TOL[dtype]["grad"]


# ---- 6. refusals: the error named, the context usable afterwards ---------------------------------------------------------------
def test_refusals_leave_the_context_usable():
    import pinn_native
    layers = layers_of(8)
    X_f, X_u, u, X_lo, X_hi = point_sets(2048)
    eng = make(layers, "f64", 7, adr_ref.ALLEN_CAHN, X_f, X_u, u, X_lo, X_hi)
    eng.set_weights(weights(layers))
    before = eng.loss_grad()

    def same():
        after = eng.loss_grad()
        assert after[0] == before[0] and np.array_equal(after[1], before[1]) and np.array_equal(after[2], before[2])
        assert eng.kernel_path() == 7

    for path in (1, 2, 3, 4, 5, 6, 8):
        with pytest.raises(pinn_native.PinnNativeError, match="adr kind .*paths 0 and 7 only"):
            eng.set_kernel_path(path)
        same()
    with pytest.raises(pinn_native.PinnNativeError, match="self-adaptive weights are for Burgers"):
        eng.sa_set_weights(np.ones(len(X_u)), np.ones(len(X_f)))
    same()
    for bad in ((1e-4,), (0.0, 0.0, 1e-4, -5.0, 0.0), (0.0, 0.0, 1e-4, -5.0, 0.0, 5.0, 1.0)):
        with pytest.raises(pinn_native.PinnNativeError, match="6 coefficients"):
            eng.set_pde_params(*bad)
        same()
    for bad in ((0.0, 0.0, np.nan, -5.0, 0.0, 5.0), (0.0, np.inf, 1e-4, -5.0, 0.0, 5.0)):
        with pytest.raises(pinn_native.PinnNativeError, match="not finite"):
            eng.set_pde_params(*bad)
        same()
    with pytest.raises(pinn_native.PinnNativeError, match="ensembles support Burgers"):
        pinn_native.Ensemble(layers, LB, UB, 4, pde="adr", dtype="f64")
    same()
    eng.close()
    e32 = make(layers, "f32", 0, adr_ref.ALLEN_CAHN, X_f, X_u, u, X_lo, X_hi)
    for path in (1, 2, 7):
        with pytest.raises(pinn_native.PinnNativeError):
            e32.set_kernel_path(path)
    assert np.isfinite(e32.loss_grad()[0])
    e32.close()


# ---- 7. the script ----------------------------------------------------------------------------------------------------------------
LINE = re.compile(r"^(tf_epoch|nt_epoch) =\s+(\d+)\s+elapsed = \d\d:\d\d \(\+\d\d\.\d\)  loss = (\S+)  ")
END = re.compile(r"^Training finished \(epoch (\d+)\): duration = \d\d:\d\d  error = (\S+)  ")
SHORT_HP = {"N_0": 512, "N_b": 200, "N_f": 20000, "layers": layers_of(8), "seed": 1234,
            "tf_epochs": 20, "tf_lr": 0.003, "tf_b1": 0.9, "tf_eps": None,
            "nt_epochs": 20, "nt_lr": 0.8, "nt_ncorr": 50, "log_frequency": 5}


def test_script_runs_and_its_first_logged_loss_is_the_oracles(tmp_path):
    """inf_cont_allen_cahn.py with a short hp as a child process: Logger lines in the existing format, a finite final error,
    a result folder.  The log prints five significant digits, so the 1e-12 comparison of the first logged loss goes through
    the number behind the line: the same model built in this process from the same hp and seeds (identical point sets and
    initial weights) evaluates its loss at the initial weights, that value agrees with adr_ref to 1e-12, and the child's
    first line prints exactly that value in the log's format."""
    hp_file = tmp_path / "hp.json"
    hp_file.write_text(json.dumps(SHORT_HP))
    env = dict(os.environ, MPLBACKEND="Agg")
    env.pop("PINN_NO_PLOT", None)
    res = subprocess.run([sys.executable, os.path.join(PKG, "1d-allen-cahn", "inf_cont_allen_cahn.py"), str(hp_file)],
                         cwd=PKG, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    out = res.stdout
    assert "-- Starting Adam optimization --" in out and "-- Starting LBFGS optimization --" in out
    rows = [(m.group(1), int(m.group(2)), m.group(3)) for m in map(LINE.match, out.splitlines()) if m]
    assert [r[:2] for r in rows[:4]] == [("tf_epoch", 0), ("tf_epoch", 5), ("tf_epoch", 10), ("tf_epoch", 15)]
    assert any(r[0] == "nt_epoch" for r in rows)
    assert all(np.isfinite(float(r[2])) for r in rows)
    ends = [m for m in map(END.match, out.splitlines()) if m]
    assert len(ends) == 1 and int(ends[0].group(1)) == 40 and np.isfinite(float(ends[0].group(2)))
    m = re.search(r"Saving results to directory\s+(\S+)", out)
    assert m and os.path.isfile(os.path.join(m.group(1), "hp.json")) and os.path.isfile(os.path.join(m.group(1), "weights.npy"))
    assert any(f.startswith("graph") for f in os.listdir(m.group(1)))

    # the number behind the first line
    import allencahnutil as ac
    import neuralnetwork as nn
    from logger import Logger
    np.random.seed(1234)
    (x, t, X, T, Exact_u, X_star, u_star, X_u, u, X_f, X_lb, X_ub, ub, lb) = ac.prep_data(
        SHORT_HP["N_0"], SHORT_HP["N_b"], SHORT_HP["N_f"], cache_dir=os.path.join(PKG, "1d-allen-cahn", "results"))

    class Model(nn.NeuralNetwork):
        pde = "adr"

    pinn = Model(dict(SHORT_HP), Logger(dict(SHORT_HP, log_frequency=10 ** 9)), ub, lb)
    pinn._engine.set_pde_params(*ac.ADR_COEFFS)
    pinn._set_collocation(X_f)
    pinn._set_boundary(X_lb, X_ub)
    pinn._bind(X_u, u)
    assert pinn._engine.kernel_path() == 7
    w0 = pinn.get_weights()
    loss0 = pinn._engine.loss_grad()[0]
    lo, _, _ = adr_ref.adr_loss_grad(np.asarray(w0).ravel(), SHORT_HP["layers"], lb, ub, X_f, X_u, u, X_lb, X_ub, ac.ADR_COEFFS)
    print("first loss: engine %.17g oracle %.17g printed %s" % (loss0, lo, rows[0][2]))
    assert abs(loss0 - lo) / lo < 1e-12
    assert rows[0][2] == "%.4e" % loss0
