"""GPU: Robin points of the adr kind (pinn_set_robin, Engine.set_robin) against the numpy restatement
tests/helpers/adr_robin_ref.py (pinned on the CPU by tests/test_adr_robin_host.py).

  r_j = alpha_j u + beta_j u_x - g_j,   loss = adr loss + (1 / N_w) sum r_j^2,   terms[2] = periodic pairs + Robin part

Float64 on the generic kernels (path 0) and on k_fused20d<PDE_ADR_ROBIN, H, .> (path 7, one tile per workgroup and tile
loop), float32 on path 0.  Float64 bounds are tests/test_gpu_adr.py's TOL (loss 1e-12, gradient 1e-11, residual 1e-10),
float32 1e-5 / 2e-5 / 2e-4.  The Robin block stands behind the collocation block of the assembled set, so the block-edge
cases move its start and end through the 16-point waves and 64-point tiles by the counts in front of it."""
import functools
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
sys.path.insert(0, os.path.join(PKG, "1d-heat"))
import adr_ref  # noqa: E402
import adr_robin_ref  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = {"f64": dict(loss=1e-12, grad=1e-11, res=1e-10), "f32": dict(loss=1e-5, grad=2e-5, res=2e-4)}
LB, UB = np.array([-1.0, 0.0]), np.array([1.0, 1.0])
CONFIGS = [("f64", 0), ("f64", 7), ("f32", 0)]        # (dtype, kernel path)


def rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300)


def layers_of(depth, width=20):
    return [2] + [width] * depth + [1]


@functools.lru_cache(maxsize=None)
def weights(depth, seed=7):
    """a glorot draw plus 0.05 * standard_normal: biases non-zero"""
    from oracle import init
    w = init.glorot_flat(layers_of(depth))
    w = w + 0.05 * np.random.RandomState(seed).standard_normal(w.size)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def point_sets(N_f, n_0=512, n_b=50, seed=3):
    """collocation points, initial data u(x, 0) = x^2 cos(pi x), n_b wall pairs"""
    rs = np.random.RandomState(seed)
    X_f = LB + (UB - LB) * rs.uniform(size=(N_f, 2))
    x0 = rs.uniform(-1, 1, n_0)
    X_u = np.column_stack([x0, np.zeros(n_0)])
    u = (x0 * x0 * np.cos(np.pi * x0)).reshape(-1, 1)
    tb = rs.uniform(0, 1, n_b)
    X_lo, X_hi = np.column_stack([np.full(n_b, -1.0), tb]), np.column_stack([np.full(n_b, 1.0), tb])
    for a in (X_f, X_u, u, X_lo, X_hi):
        a.setflags(write=False)
    return X_f, X_u, u, X_lo, X_hi


@functools.lru_cache(maxsize=None)
def robin_points(n_w, seed=11):
    """x alternating between the walls, random t, alpha, beta in U(-1.5, 1.5) with every fifth alpha and every seventh beta 0
    (never both: such a point is refused), g in U(-1, 1)"""
    rs = np.random.RandomState(seed)
    j = np.arange(n_w)
    X_w = np.column_stack([np.where(j % 2, 1.0, -1.0), rs.uniform(0, 1, n_w)])
    alpha, beta, g = rs.uniform(-1.5, 1.5, n_w), rs.uniform(-1.5, 1.5, n_w), rs.uniform(-1, 1, n_w)
    alpha[j % 5 == 4] = 0.0
    beta[(j % 7 == 6) & (alpha != 0.0)] = 0.0
    for a in (X_w, alpha, beta, g):
        a.setflags(write=False)
    return X_w, alpha, beta, g


@functools.lru_cache(maxsize=None)
def base_ref(depth, name, N_f, n_0, n_b):
    """adr_ref on the sets without Robin points: computed once per (net, equation, sets), shared, never written to"""
    X_f, X_u, u, X_lo, X_hi = point_sets(N_f, n_0, n_b)
    return adr_ref.adr_loss_grad(weights(depth), layers_of(depth), LB, UB, X_f, X_u if n_0 else None, u if n_0 else None,
                                 X_lo if n_b else None, X_hi if n_b else None, adr_ref.COEFF_SETS[name])


def make(layers, dtype, path, coeffs, X_f, X_u=None, u=None, X_lo=None, X_hi=None, robin=None, lb=LB, ub=UB):
    from pinn_native import Engine
    eng = Engine(layers, lb, ub, pde="adr", dtype=dtype)
    eng.set_pde_params(*coeffs)
    eng.set_collocation(X_f)
    if X_u is not None and len(X_u):
        eng.set_data(X_u, u)
    if X_lo is not None and len(X_lo):
        eng.set_boundary(X_lo, X_hi)
    if robin is not None:
        eng.set_robin(*robin)
    eng.set_kernel_path(path)          # no skip: paths 0 and 7 must exist for every cell
    assert eng.kernel_path() == path
    return eng


def check_cell(record, tag, depth, dtype, path, name, N_f, n_0, n_b, n_w):
    layers, w, co = layers_of(depth), weights(depth), adr_ref.COEFF_SETS[name]
    X_f, X_u, u, X_lo, X_hi = point_sets(N_f, n_0, n_b)
    rob = robin_points(n_w)
    eng = make(layers, dtype, path, co, X_f, X_u if n_0 else None, u, X_lo if n_b else None, X_hi, rob)
    eng.set_weights(w)
    loss, grad, terms = eng.loss_grad()
    r = eng.robin_residual()
    f = eng.residual()
    assert eng.n_w == n_w
    eng.close()
    lo, go, ex = adr_robin_ref.robin_loss_grad(w, layers, LB, UB, X_f, X_u, u, X_lo, X_hi, co, *rob,
                                               base=base_ref(depth, name, N_f, n_0, n_b))
    tol = TOL[dtype]
    dev = dict(loss=abs(loss - lo) / lo, grad=rel(grad, go), res=rel(f, ex["f"]), rob=rel(r, ex["r"]),
               t_f=abs(terms[0] - ex["mse_f"]) / lo, t_u=abs(terms[1] - ex["mse_u"]) / lo,
               t_b=abs(terms[2] - (ex["mse_b"] + ex["mse_w"])) / lo)
    print("adr robin %s %s path %d: %s" % (tag, dtype, path, " ".join("%s %.2e" % kv for kv in sorted(dev.items()))))
    record(tag=tag, dtype=dtype, path=path, **dev)
    assert r.shape == (n_w,) and ex["mse_w"] > 0
    assert dev["loss"] < tol["loss"]
    assert dev["grad"] < tol["grad"]
    assert dev["res"] < tol["res"]
    assert dev["rob"] < tol["res"]
    # the three parts, in the order (residual, data, boundary = pairs + Robin); relative to the loss they add up to
    assert max(dev["t_f"], dev["t_u"], dev["t_b"]) < tol["loss"] * 10
    assert terms[2] > 0


# ---- 1. kernel variants: depths x one tile per workgroup (2048) / tile loop (40000: 627 tiles > 256) -----------------------
@pytest.mark.parametrize("dtype,path", CONFIGS)
@pytest.mark.parametrize("N_f", [2048, 40000])
@pytest.mark.parametrize("depth", [4, 6, 8])
def test_variants_depths_and_tile_plans(record, depth, N_f, dtype, path):
    check_cell(record, "a:d%d:Nf%d" % (depth, N_f), depth, dtype, path, "allen_cahn", N_f, 512, 50, 50)


# ---- 2. block edges: the Robin block starts anywhere in a wave, straddles waves and tiles, ends in the padding tile -----------
# 2 n_b + 512 + N_f points stand in front of the block: with 0 and 7 pairs and these N_f it starts at lane 0 and at lane 14 of
# a wave (2048, 40000: offsets 2560 / 2574 and 40512 / 40526); N_f = 2034 with 7 pairs makes the count in front 2560 = 40 x 64,
# a tile of its own for the block.
@pytest.mark.parametrize("dtype,path", CONFIGS)
@pytest.mark.parametrize("n_b", [0, 7])
@pytest.mark.parametrize("N_f", [2048, 40000])
@pytest.mark.parametrize("n_w", [1, 15, 16, 17, 63, 64, 65, 200])
def test_block_edges(record, n_w, N_f, n_b, dtype, path):
    check_cell(record, "b:nw%d:Nf%d:nb%d" % (n_w, N_f, n_b), 8, dtype, path, "allen_cahn", N_f, 512, n_b, n_w)


@pytest.mark.parametrize("dtype,path", CONFIGS)
@pytest.mark.parametrize("n_w", [1, 64, 65])
def test_block_starting_a_tile_of_its_own(record, n_w, dtype, path):
    assert (2 * 7 + 512 + 2034) % 64 == 0
    check_cell(record, "b:own-tile:nw%d" % n_w, 8, dtype, path, "allen_cahn", 2034, 512, 7, n_w)


# ---- 3. set kinds x equations -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,path", CONFIGS)
@pytest.mark.parametrize("kind", ["robin", "robin+data", "robin+pairs"])
@pytest.mark.parametrize("name", sorted(adr_ref.COEFF_SETS))
def test_equations_and_set_kinds(record, name, kind, dtype, path):
    n_0 = 512 if kind == "robin+data" else 0
    n_b = 50 if kind == "robin+pairs" else 0
    check_cell(record, "c:%s:%s" % (name, kind), 8, dtype, path, name, 2048, n_0, n_b, 50)


# ---- 4. Dirichlet rows are data points, on the device ------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,path", [("f64", 0), ("f64", 7)])
def test_dirichlet_rows_equal_data_points_in_a_second_context(record, dtype, path):
    layers, w = layers_of(8), weights(8)
    X_f, _, _, X_lo, X_hi = point_sets(2048)
    X_w, _, _, g = robin_points(50)
    a = make(layers, dtype, path, adr_ref.ALLEN_CAHN, X_f, None, None, None, None, (X_w, 1.0, 0.0, g))
    b = make(layers, dtype, path, adr_ref.ALLEN_CAHN, X_f, X_w, g.reshape(-1, 1))
    a.set_weights(w)
    b.set_weights(w)
    la, ga, ta = a.loss_grad()
    lb_, gb, tb = b.loss_grad()
    a.close()
    b.close()
    d_t, d_g = abs(ta[2] - tb[1]) / tb[1], rel(ga, gb)
    record(path=path, term=d_t, grad=d_g)
    assert ta[1] == 0.0 and tb[2] == 0.0 and tb[1] > 0
    assert d_t < 1e-14
    assert d_g < 1e-12


# ---- 5. bit identity and reproducibility ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("N_f", [10000, 40000])
def test_bit_identity_and_reproducibility(record, N_f):
    layers, w = layers_of(8), weights(8)
    X_f, X_u, u, X_lo, X_hi = point_sets(N_f, 512, 200)
    rob = robin_points(50)
    eng = make(layers, "f64", 7, adr_ref.ALLEN_CAHN, X_f, X_u, u, X_lo, X_hi, rob)
    never = make(layers, "f64", 7, adr_ref.ALLEN_CAHN, X_f, X_u, u, X_lo, X_hi)
    eng.set_weights(w)
    never.set_weights(w)
    # (a) two evaluations are bit-equal, on both paths; (c) switching the path and back gives the first bits again
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
    record(N_f=N_f, loss=abs(l7 - l0) / abs(l0), grad=rel(g7, g0), t_b=abs(t7[2] - t0[2]) / abs(l0))
    assert abs(l7 - l0) / abs(l0) < 1e-12
    assert rel(g7, g0) < 1e-11
    assert abs(t7[2] - t0[2]) / abs(l0) < 1e-11
    # (b) the class removed: every bit is that of a context that never had it, on both paths
    eng.set_robin(np.zeros((0, 2)), 1.0, 0.0, 0.0)
    assert eng.n_w == 0 and eng.robin_residual().shape == (0,)
    for path in (7, 0):
        eng.set_kernel_path(path)
        never.set_kernel_path(path)
        le, ge, te = eng.loss_grad()
        ln, gn, tn = never.loss_grad()
        assert le == ln and np.array_equal(ge, gn) and np.array_equal(te, tn)
        assert le != (l7 if path == 7 else l0)
    eng.close()
    never.close()


# ---- 6. redraws keep the class ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("draw", ["lhs", "rad"])
@pytest.mark.parametrize("dtype,path", CONFIGS)
def test_redraws_keep_the_robin_points(record, draw, dtype, path):
    layers, w, co = layers_of(8), weights(8), adr_ref.ALLEN_CAHN
    X_f, X_u, u, X_lo, X_hi = point_sets(2048)
    rob = robin_points(50)
    eng = make(layers, dtype, path, co, X_f, X_u, u, X_lo, X_hi, rob)
    plain = make(layers, dtype, path, co, X_f, X_u, u, X_lo, X_hi)
    got = []
    for e in (eng, plain):
        e.set_weights(w)
        if draw == "lhs":
            e.lhs_collocation(3000, 0x5EED0001)
        else:
            e.rad_collocation(3000, 0x5EED0002, 20000, k=1, c=1.0)
        got.append(e.get_collocation())
    assert got[0].shape == (3000, 2) and np.array_equal(got[0], got[1])
    loss, grad, terms = eng.loss_grad()
    r = eng.robin_residual()
    eng.close()
    plain.close()
    lo, go, ex = adr_robin_ref.robin_loss_grad(w, layers, LB, UB, got[0], X_u, u, X_lo, X_hi, co, *rob)
    tol = TOL[dtype]
    dev = dict(loss=abs(loss - lo) / lo, grad=rel(grad, go), rob=rel(r, ex["r"]),
               t_b=abs(terms[2] - (ex["mse_b"] + ex["mse_w"])) / lo)
    record(draw=draw, dtype=dtype, path=path, **dev)
    assert dev["loss"] < tol["loss"] and dev["grad"] < tol["grad"] and dev["rob"] < tol["res"] and dev["t_b"] < tol["loss"] * 10


# ---- 7. trajectories ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", [0, 7])
def test_adam_and_lbfgs_trajectories(record, path):
    """30 Adam steps (lr 1e-3) and 25 L-BFGS iterations (N_f = 2048, 50 pairs, 50 Robin points) against oracle.optim driven by
    adr_robin_ref, float64, at the 1e-8 the README states for trajectories"""
    from oracle import optim
    layers = layers_of(8)
    X_f, X_u, u, X_lo, X_hi = point_sets(2048)
    rob = robin_points(50)
    co = adr_ref.ALLEN_CAHN
    w0 = np.array(weights(8))

    def fg(w):
        l, g, _ = adr_robin_ref.robin_loss_grad(w, layers, LB, UB, X_f, X_u, u, X_lo, X_hi, co, *rob)
        return l, g

    eng = make(layers, "f64", path, co, X_f, X_u, u, X_lo, X_hi, rob)
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
    print("adr robin trajectories path %d: adam loss %.2e w %.2e | lbfgs loss %.2e w_model %.2e (%d logged)" % (path, da, dw, dl, dm, n))
    record(path=path, adam_loss=da, adam_w=dw, lbfgs_loss=dl, lbfgs_w_model=dm)
    assert n >= 20 and len(lo_all) == len(ref_l)
    assert da < 1e-8 and dw < 1e-8
    assert dl < 1e-8 and dm < 1e-8


# ---- 8. refusals leave the context usable -----------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable():
    import pinn_native
    layers, w = layers_of(8), weights(8)
    X_f, X_u, u, X_lo, X_hi = point_sets(2048)
    rob = robin_points(50)
    eng = make(layers, "f64", 7, adr_ref.ALLEN_CAHN, X_f, X_u, u, X_lo, X_hi, rob)
    eng.set_weights(w)
    before = eng.loss_grad()

    def same(e=eng, ref=before, path=7):
        after = e.loss_grad()
        assert after[0] == ref[0] and np.array_equal(after[1], ref[1]) and np.array_equal(after[2], ref[2])
        assert e.kernel_path() == path

    with pytest.raises(pinn_native.PinnNativeError, match="pinn_pw_set: point weights do not cover Robin points"):
        eng.pw_set()
    same()
    for path in (1, 2, 3, 4, 5, 6, 8):
        with pytest.raises(pinn_native.PinnNativeError, match="adr kind .*paths 0 and 7 only"):
            eng.set_kernel_path(path)
        same()
    # bad rows through the library itself (Engine.set_robin would stop them first): the stored class stays
    import ctypes
    X2, one, zero = (ctypes.c_double * 4)(0.0, 0.5, 1.0, 0.5), (ctypes.c_double * 2)(1.0, 1.0), (ctypes.c_double * 2)(0.0, 0.0)
    assert eng._lib.pinn_set_robin(eng._h, X2, zero, zero, zero, 2, 2) == -1
    assert eng._lib.pinn_set_robin(eng._h, X2, one, one, zero, 2, 1) == -1
    assert eng._lib.pinn_robin_residual(eng._h, one, 2) == -1                  # another length than the class
    same()
    eng.close()
    # point weights on: set_robin is refused, the weighted results stay
    pw = make(layers, "f64", 7, adr_ref.ALLEN_CAHN, X_f, X_u, u, X_lo, X_hi)
    pw.set_weights(w)
    pw.pw_set(np.full(len(X_u), 2.0), None, None)
    ref = pw.loss_grad()
    with pytest.raises(pinn_native.PinnNativeError, match="pinn_set_robin: point weights do not cover Robin points"):
        pw.set_robin(*rob)
    assert pw.n_w == 0
    same(pw, ref)
    pw.close()
    # the adr_ide kind
    ide = pinn_native.Engine(layers, LB, UB, pde="adr_ide", dtype="f64")
    ide.set_pde_params(*adr_ref.ALLEN_CAHN)
    ide.set_collocation(X_f)
    ide.set_data(X_u, u)
    ide.set_weights(np.concatenate([w, ide.get_weights()[-6:]]))
    ref = ide.loss_grad()
    with pytest.raises(pinn_native.PinnNativeError, match="pinn_set_robin: .*adr kind \\(pde 5\\) only.*adr_ide"):
        ide.set_robin(*rob)
    with pytest.raises(pinn_native.PinnNativeError, match="pinn_robin_residual: .*adr kind"):
        ide._check(ide._lib.pinn_robin_residual(ide._h, None, 0))
    same(ide, ref, ide.kernel_path())
    ide.close()
    # another kind altogether
    bg = pinn_native.Engine(layers, LB, UB, pde="burgers", dtype="f64")
    with pytest.raises(pinn_native.PinnNativeError, match="pinn_set_robin: .*adr kind \\(pde 5\\) only"):
        bg.set_robin(*rob)
    bg.close()


# ---- 9. the script -------------------------------------------------------------------------------------------------------------------
LINE = re.compile(r"^(tf_epoch|nt_epoch) =\s+(\d+)\s+elapsed = \d\d:\d\d \(\+\d\d\.\d\)  loss = (\S+)  ")
END = re.compile(r"^Training finished \(epoch (\d+)\): duration = \d\d:\d\d  error = (\S+)  ")
SHORT_HP = {"nu": 0.1, "h": 1.0, "N_0": 128, "N_w": 64, "N_f": 2048, "layers": layers_of(8), "seed": 1234,
            "tf_epochs": 10, "tf_lr": 0.003, "tf_b1": 0.9, "tf_eps": None,
            "nt_epochs": 10, "nt_lr": 0.8, "nt_ncorr": 50, "log_frequency": 5}


def test_script_runs_and_its_first_logged_loss_is_the_restatements(tmp_path):
    """inf_cont_heat.py with a short hp as a child process: Logger lines in the existing format, a finite final error, the
    wall line, a result folder.  Its first logged loss is the restatement's on the same sets (rebuilt here from the same hp
    and seeds) and initial weights, to the four digits the log prints."""
    hp_file = tmp_path / "hp.json"
    hp_file.write_text(json.dumps(SHORT_HP))
    env = dict(os.environ, MPLBACKEND="Agg")
    env.pop("PINN_NO_PLOT", None)
    res = subprocess.run([sys.executable, os.path.join(PKG, "1d-heat", "inf_cont_heat.py"), str(hp_file)],
                         cwd=PKG, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    out = res.stdout
    assert "-- Starting Adam optimization --" in out and "-- Starting LBFGS optimization --" in out
    rows = [(m.group(1), int(m.group(2)), m.group(3)) for m in map(LINE.match, out.splitlines()) if m]
    assert [r[:2] for r in rows[:2]] == [("tf_epoch", 0), ("tf_epoch", 5)]
    assert any(r[0] == "nt_epoch" for r in rows)
    assert all(np.isfinite(float(r[2])) for r in rows)
    ends = [m for m in map(END.match, out.splitlines()) if m]
    assert len(ends) == 1 and int(ends[0].group(1)) == 20 and np.isfinite(float(ends[0].group(2)))
    wall = re.search(r"^Wall conditions: max \|alpha u \+ beta u_x - g\| = (\S+) over 128 points", out, re.M)
    assert wall and np.isfinite(float(wall.group(1)))
    m = re.search(r"Saving results to directory\s+(\S+)", out)
    assert m and os.path.isfile(os.path.join(m.group(1), "hp.json")) and os.path.isfile(os.path.join(m.group(1), "weights.npy"))
    assert any(f.startswith("graph") for f in os.listdir(m.group(1)))

    # the number behind the first line
    sys.path.insert(0, os.path.join(PKG, "utils"))
    import heatutil as hu
    import neuralnetwork as nn
    from logger import Logger
    np.random.seed(1234)
    (x, t, X, T, Exact_u, X_star, u_star, X_u, u, X_f, X_w, alpha, beta, g, ub, lb) = hu.prep_data(
        SHORT_HP["N_0"], SHORT_HP["N_w"], SHORT_HP["N_f"], nu=SHORT_HP["nu"], h=SHORT_HP["h"])

    class Model(nn.NeuralNetwork):
        pde = "adr"

    pinn = Model(dict(SHORT_HP), Logger(dict(SHORT_HP, log_frequency=10 ** 9)), ub, lb)
    w0 = np.asarray(pinn.get_weights()).ravel()
    pinn._engine.close()
    lo, _, ex = adr_robin_ref.robin_loss_grad(w0, SHORT_HP["layers"], lb, ub, X_f, X_u, u, None, None,
                                              hu.adr_coeffs(SHORT_HP["nu"]), X_w, alpha, beta, g)
    print("first loss: restatement %.17g printed %s" % (lo, rows[0][2]))
    assert ex["mse_w"] > 0
    assert rows[0][2] == "%.4e" % lo
