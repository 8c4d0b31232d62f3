"""GPU: the advection-diffusion-reaction kind with trainable coefficients (PINN_PDE_ADR_IDE, pde="adr_ide") against the numpy
restatement tests/helpers/adr_ide_ref.py (pinned on the CPU by tests/test_adr_ide_host.py).

  theta = [net | a0, a1, log nu, r1, r2, r3];  f and the loss are those of "adr";  a frozen coefficient's gradient entry is 0.0

Float64 on the generic kernels (path 0) and on the six k_fused20d<PDE_ADR_IDE, H, .> variants (path 7), float32 on path 0.  Tolerances on
the loss, the whole-vector gradient and the residual are TOL of tests/test_gpu_adr.py; the six tail entries are judged each
on its own scale A_k = sum |fb df/dp_k| with K of tests/helpers/grad_entries.py."""
import functools
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
import adr_ide_ref as ref  # noqa: E402
import adr_ref  # noqa: E402
import grad_entries as ge  # noqa: E402
import rad_ref  # noqa: E402
from test_gpu_adr import CONFIGS, LB, TOL, UB, layers_of, point_sets, rel, weights  # noqa: E402

pytestmark = pytest.mark.gpu

NU_R1_R3 = ref.mask_of(["nu", "r1", "r3"])
F64_CONFIGS = [("f64", 0), ("f64", 7)]


def make(layers, dtype, path, theta, X_f, X_u=None, u=None, X_lo=None, X_hi=None, mask=ref.ALL, lb=LB, ub=UB):
    from pinn_native import Engine
    eng = Engine(layers, lb, ub, pde="adr_ide", dtype=dtype)
    assert eng.n_params == ref.n_net(layers) + 6
    eng.set_collocation(X_f)
    if X_u is not None and len(X_u):
        eng.set_data(X_u, u)
    if X_lo is not None and len(X_lo):
        eng.set_boundary(X_lo, X_hi)
    eng.set_kernel_path(path)          # no skip: paths 0 and 7 must exist for every cell
    assert eng.kernel_path() == path
    eng.set_pde_trainable(mask)
    eng.set_weights(theta)
    return eng


@functools.lru_cache(maxsize=None)
def case(depth, N_f, n_b=50):
    """one cell's inputs and its float64 oracle values, computed once and shared (never written to)"""
    layers = layers_of(depth)
    S = point_sets(N_f, n_b=n_b)
    theta = ref.pack(weights(layers), adr_ref.ALL_NONZERO)
    lo, go, A, ex = ref.restate(theta, layers, LB, UB, *S)
    for a in (theta, go, A, ex["f"]) + tuple(S):
        a.setflags(write=False)
    return layers, S, theta, float(lo), go, A, ex


WIDE_POINTS = 4000          # an 80-bit run of the 2048-point cells takes a second, once for all paths


@functools.lru_cache(maxsize=None)
def tail_yardstick(depth, N_f, n_b, dtype):
    """-> (wide tail gradient, plain error of the tail in units of A_k): the restatement in the compute dtype against the wider
    one.  float64 sets of more than WIDE_POINTS points (or a host whose longdouble is no wider) have no 80-bit run (13 s at
    40 000 points): the float64 restatement is the reference and its own error is taken as grad_entries.ASSUMED_F64_ULPS."""
    layers, S, theta, _, go, A, _ = case(depth, N_f, n_b)
    dt = ge.DTYPES[dtype]
    n_pts = sum(len(x) for x in (S[0], S[1], S[3], S[4]))
    if dtype == "f64" and (n_pts > WIDE_POINTS or not ge.longdouble_is_wider()):
        return go[-6:].astype(np.longdouble), ge.ASSUMED_F64_ULPS * ge.unit_roundoff(dt)
    _, g, _, _ = ref.restate(theta, layers, LB, UB, *S, dtype=dt)
    _, gw, _, _ = ref.restate(theta, layers, LB, UB, *S, dtype=ge.wider(dt))
    plain = float(np.max(np.abs(g[-6:].astype(np.longdouble) - gw[-6:].astype(np.longdouble)) / A[-6:]))
    return gw[-6:].astype(np.longdouble), plain


# ---- 4., 5., 7., 11a. parity with the restatement, the tail entries on their own scale, run-to-run bit equality ---------------
CELLS = [(4, 2048, 50), (6, 2048, 50), (8, 2048, 50),      # every workgroup has a tile of its own
         (8, 40, 50),                                       # less than one tile of collocation points: padded lanes
         (8, 40000, 50),                                    # the tile loop
         (8, 2048, 1), (8, 2048, 7), (8, 2048, 8)]          # the pair block ends inside a wave / on a wave boundary


@pytest.mark.parametrize("dtype,path", CONFIGS)
@pytest.mark.parametrize("depth,N_f,n_b", CELLS)
def test_parity_with_the_restatement(record, depth, N_f, n_b, dtype, path):
    layers, S, theta, lo, go, A, ex = case(depth, N_f, n_b)
    eng = make(layers, dtype, path, theta, *S)
    loss, grad, terms = eng.loss_grad()
    loss2, grad2, terms2 = eng.loss_grad()
    f = eng.residual()
    eng.close()
    tol = TOL[dtype]
    dev = dict(loss=abs(loss - lo) / lo, grad=rel(grad, go), res=rel(f, ex["f"]), t_f=abs(terms[0] - ex["mse_f"]) / lo,
               t_u=abs(terms[1] - ex["mse_u"]) / lo, t_b=abs(terms[2] - ex["mse_b"]) / lo)
    # the six tail entries, each against its own rounding scale
    g_wide, plain = tail_yardstick(depth, N_f, n_b, dtype)
    u = ge.unit_roundoff(ge.DTYPES[dtype])
    yard = max(plain, ge.FLOOR_ULPS * u)
    tail = np.asarray(np.abs(grad[-6:].astype(np.longdouble) - g_wide) / A[-6:], dtype=np.float64)
    ratio = float(np.max(tail)) / yard
    print("adr_ide d%d Nf%d nb%d %s path %d: %s | tail/yardstick %.3f (entry %s, yardstick %.1f u)" % (
        depth, N_f, n_b, dtype, path, " ".join("%s %.2e" % kv for kv in sorted(dev.items())), ratio,
        ref.NAMES[int(np.argmax(tail))], yard / u))
    record(kind="adr_ide", depth=depth, N_f=N_f, n_b=n_b, dtype=dtype, path=path, tail_ratio=ratio,
           tail_entry=ref.NAMES[int(np.argmax(tail))], **dev)
    assert loss == loss2 and np.array_equal(grad, grad2) and np.array_equal(terms, terms2)      # bit-reproducible
    assert dev["loss"] < tol["loss"]
    assert dev["grad"] < tol["grad"]
    assert dev["res"] < tol["res"]
    assert max(dev["t_f"], dev["t_u"], dev["t_b"]) < tol["loss"] * 10
    assert terms[2] > 0
    assert np.all(A[-6:] > 0) and np.all(grad[-6:] != 0.0)
    assert ratio < ge.K[("w20", dtype)]


# ---- 6. masks ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,path", CONFIGS)
def test_masks_gate_the_store_only(dtype, path):
    """frozen entries are == 0.0, trained ones and every net entry bit for bit those of the all-six run on the same path"""
    layers, S, theta, *_ = case(8, 2048)
    eng = make(layers, dtype, path, theta, *S)
    l_all, g_all, _ = eng.loss_grad()
    for mask in [0] + [1 << k for k in range(6)] + [NU_R1_R3]:
        eng.set_pde_trainable(mask)
        l, g, _ = eng.loss_grad()
        assert l == l_all and np.array_equal(g[:-6], g_all[:-6])
        for k in range(6):
            if (mask >> k) & 1:
                assert g[-6 + k] == g_all[-6 + k] != 0.0
            else:
                assert g[-6 + k] == 0.0
    eng.set_pde_trainable(["nu", "r1", "r3"])          # names
    assert np.array_equal(eng.loss_grad()[1], g)
    eng.close()


# ---- 8. a check that needs no oracle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,path", F64_CONFIGS)
def test_central_differences_in_the_raw_coefficients(record, dtype, path):
    """L is exactly quadratic in a0, a1, r1, r2, r3, so the central difference with h = 2^-10 is the gradient entry up to the
    rounding of the two loss values, 8 u max L / h"""
    layers, S, theta, *_ = case(8, 2048)
    eng = make(layers, dtype, path, theta, *S)
    _, g, _ = eng.loss_grad()
    h, u = 2.0 ** -10, ge.unit_roundoff(np.float64)
    for k in (0, 1, 3, 4, 5):
        L = []
        for sgn in (1.0, -1.0):
            t = np.array(theta)
            t[-6 + k] += sgn * h
            eng.set_weights(t)
            L.append(eng.loss_grad()[0])
        fd, bound = (L[0] - L[1]) / (2 * h), 8 * u * max(L) / h
        record(path=path, entry=ref.NAMES[k], fd_dev=abs(fd - g[-6 + k]), bound=bound)
        assert abs(fd - g[-6 + k]) < bound, (ref.NAMES[k], fd, g[-6 + k], bound)
    eng.close()


# ---- 9. the reference-made identification fixtures --------------------------------------------------------------------------------
IDE_LB, IDE_UB = np.array([-1.0, 0.0]), np.array([1.0, 0.99])


def _ide_theta(w):
    return np.concatenate([w[:-2], [0.0, w[-2], w[-1], 0.0, 0.0, 0.0]])


@pytest.mark.parametrize("dtype,path", CONFIGS)
@pytest.mark.parametrize("tag", ["_small", ""])
def test_burgers_identification_fixture(record, tag, dtype, path):
    """collocation = data = X_u, mask {a1, nu}, tail [0, lambda_1, lambda_2, 0, 0, 0] is the reference's identification model"""
    g = np.load(golden("burgers_ide_eval%s.npz" % tag))
    X_u, u, layers = g["X_u"], g["u"], layers_of(8)
    mask = ref.mask_of(["a1", "nu"])
    theta = _ide_theta(g["w0"])
    eng = make(layers, dtype, path, theta, X_u, X_u, u, mask=mask, lb=IDE_LB, ub=IDE_UB)
    loss, grad, terms = eng.loss_grad()
    tol = TOL[dtype]
    g_ref = _ide_theta(g["grad"])
    # the two trained tail entries on their own scale.  The fixture's values are float64 numbers of another program, so in
    # float64 the yardstick is the rounding grad_entries assumes of a float64 run (ASSUMED_F64_ULPS); in float32 it is the
    # float32 restatement's error against the float64 one, as everywhere
    _, g64, A, _ = ref.restate(theta, layers, IDE_LB, IDE_UB, X_u, X_u, u, None, None, mask=mask)
    un = ge.unit_roundoff(ge.DTYPES[dtype])
    if dtype == "f64":
        plain = ge.ASSUMED_F64_ULPS * un
    else:
        _, g32, _, _ = ref.restate(theta, layers, IDE_LB, IDE_UB, X_u, X_u, u, None, None, mask=mask, dtype=np.float32)
        plain = float(np.max(np.abs(g32[-5:-3].astype(np.float64) - g64[-5:-3]) / A[-5:-3]))
    yard = ge.K[("w20", dtype)] * max(plain, ge.FLOOR_ULPS * un)
    tail = np.abs(grad[-6:] - g_ref[-6:])
    record(tag=tag, dtype=dtype, path=path, loss=abs(loss - float(g["loss"])) / float(g["loss"]), grad=rel(grad, g_ref),
           lam1=tail[1] / A[-5], lam2=tail[2] / A[-4])
    assert abs(loss - float(g["loss"])) / float(g["loss"]) < tol["loss"]
    assert rel(grad, g_ref) < tol["grad"]
    assert tail[1] < yard * A[-5] and tail[2] < yard * A[-4]
    assert grad[-6] == 0.0 and np.all(grad[-3:] == 0.0) and terms[2] == 0.0
    if dtype == "f64":          # the fixture's 10 Adam steps and its 25-iteration L-BFGS trajectory: 1e-8 on the losses
        eng.adam_init(1e-3, 0.9, 0.999, 1e-7)
        losses = eng.adam_run(10)
        da = float(np.max(np.abs(losses - g["adam_losses"]) / g["adam_losses"]))
        dw = rel(eng.get_weights(), _ide_theta(g["adam_w_after_10"]))
        eng.set_weights(theta)
        eng.lbfgs_begin(int(g["lbfgs_max_iter"]), 0.8, int(g["lbfgs_n_corr"]), np.finfo(float).eps)
        it_all, lo_all, done = [], [], 0
        while not done:
            it, lo, done = eng.lbfgs_run(6)
            it_all.extend(it.tolist())
            lo_all.extend(lo.tolist())
        dl = float(np.max(np.abs(np.array(lo_all) - g["lbfgs_log_losses"]) / g["lbfgs_log_losses"]))
        w_end = eng.get_weights()
        record(tag=tag, path=path, adam_loss_dev=da, adam_w=dw, lbfgs_loss_dev=dl)
        assert done == 1 and it_all == g["lbfgs_log_iters"].tolist()
        assert da < 1e-8 and dw < 1e-8
        assert dl < 1e-8
        assert w_end[-6] == 0.0 and np.all(w_end[-3:] == 0.0)          # the frozen four never moved
    eng.close()


# ---- 10. trajectories with a mask ----------------------------------------------------------------------------------------------------
STARTS = {"allen_cahn": adr_ref.ALLEN_CAHN,                          # a0, a1, r2 frozen at 0
          "frozen_not_zero": [0.3, -0.8, 1e-4, -5.0, -0.4, 5.0]}     # the same nu, r1, r3; a0, a1, r2 frozen at other values


@pytest.mark.parametrize("path", [0, 7])
@pytest.mark.parametrize("start", sorted(STARTS))
def test_adam_and_lbfgs_trajectories_with_frozen_coefficients(record, start, path):
    """30 Adam steps (lr 1e-3) and 25 L-BFGS iterations, mask {nu, r1, r3}, Allen-Cahn start values, against oracle.optim
    driven by the restatement at the 1e-8 of tests/test_gpu_adr.py::test_adam_and_lbfgs_trajectories; afterwards the three
    frozen tail entries of get_weights() are bit-identical to their start values"""
    from oracle import optim
    layers = layers_of(8)
    S = point_sets(2048)
    theta0 = ref.pack(weights(layers), STARTS[start])
    frozen = [-6, -5, -2]

    def fg(t):
        l, g, _ = ref.loss_grad(t, layers, LB, UB, *S, mask=NU_R1_R3)
        return l, g

    eng = make(layers, "f64", path, theta0, *S, mask=NU_R1_R3)
    eng.adam_init(1e-3, 0.9, 0.999, 1e-7)
    losses = eng.adam_run(30)
    w_dev = eng.get_weights()
    opt, w, ref_l = optim.Adam(1e-3, 0.9, 0.999, 1e-7), theta0.copy(), []
    for _ in range(30):
        l, g = fg(w)
        ref_l.append(l)
        w = opt.step(w, g)
    da, dw = float(np.max(np.abs(losses - np.array(ref_l)) / np.array(ref_l))), rel(w_dev, w)
    assert all(w_dev[i] == theta0[i] for i in frozen) and all(w_dev[i] != theta0[i] for i in (-4, -3, -1))
    eng.set_weights(theta0)
    eng.lbfgs_begin(25, 0.8, 50, np.finfo(float).eps)
    lo_all, done = [], 0
    while not done:
        it, lo, done = eng.lbfgs_run(7)
        lo_all.extend(lo.tolist())
    w_model = eng.get_weights()
    eng.close()
    res = optim.lbfgs(fg, theta0.copy(), 25, 0.8, 50)
    rl = np.array([l for _, l in res["logs"]])
    n = min(len(lo_all), len(rl))
    dl = float(np.max(np.abs(np.array(lo_all[:n]) - rl[:n]) / rl[:n]))
    dm = rel(w_model, res["x_model"])
    print("adr_ide trajectories path %d: adam loss %.2e w %.2e | lbfgs loss %.2e w_model %.2e (%d logged)" % (path, da, dw, dl, dm, n))
    record(path=path, start=start, adam_loss=da, adam_w=dw, lbfgs_loss=dl, lbfgs_w_model=dm)
    assert n >= 20 and len(lo_all) == len(rl)
    assert da < 1e-8 and dw < 1e-8
    assert dl < 1e-8 and dm < 1e-8
    assert all(w_model[i] == theta0[i] for i in frozen) and all(w_model[i] != theta0[i] for i in (-4, -3, -1))


# ---- 11. default path, refusals, the forward-only entry points ---------------------------------------------------------------------
def test_default_path():
    from pinn_native import Engine
    for depth in (4, 6, 8):
        eng = Engine(layers_of(depth), LB, UB, pde="adr_ide", dtype="f64")
        assert eng.kernel_path() == 7
        eng.close()
    for layers, dtype in ((layers_of(8), "f32"), (layers_of(5), "f64"), (layers_of(3, 100), "f64")):
        eng = Engine(layers, LB, UB, pde="adr_ide", dtype=dtype)
        assert eng.kernel_path() == 0
        eng.close()


def test_a_new_context_holds_burgers_coefficients_all_frozen():
    from pinn_native import Engine
    eng = Engine(layers_of(4), LB, UB, pde="adr_ide", dtype="f64")
    p = eng.get_pde_params()
    assert p[0] == 0.0 and p[1] == 1.0 and abs(p[2] - 0.01 / np.pi) < 1e-17 and np.all(p[3:] == 0.0)
    X_f = point_sets(256)[0]
    eng.set_collocation(X_f)
    eng.set_weights(np.concatenate([weights(layers_of(4)), eng.get_weights()[-6:]]))
    assert np.all(eng.loss_grad()[1][-6:] == 0.0)
    eng.close()


def test_refusals_name_their_reason_and_leave_the_context_usable():
    import pinn_native
    layers, S, theta, *_ = case(8, 2048)
    eng = make(layers, "f64", 7, theta, *S)
    before = eng.loss_grad()

    def same():
        after = eng.loss_grad()
        assert after[0] == before[0] and np.array_equal(after[1], before[1]) and np.array_equal(after[2], before[2])
        assert eng.kernel_path() == 7

    for path in (1, 2, 3, 4, 5, 6, 8):
        with pytest.raises(pinn_native.PinnNativeError, match="adr_ide kind .*paths 0 and 7 only"):
            eng.set_kernel_path(path)
        same()
    with pytest.raises(pinn_native.PinnNativeError, match="self-adaptive weights are for Burgers"):
        eng.sa_set_weights(np.ones(len(S[1])), np.ones(len(S[0])))
    same()
    for bad in (64, -1, 1 << 10):
        with pytest.raises(pinn_native.PinnNativeError, match="outside 0..63"):
            eng.set_pde_trainable(bad)
        same()
    with pytest.raises(ValueError, match="unknown adr coefficient"):
        eng.set_pde_trainable(["nu", "rho"])
    same()
    co = list(adr_ref.ALL_NONZERO)
    for bad_nu in (0.0, -0.02):
        with pytest.raises(pinn_native.PinnNativeError, match="nu must be positive"):
            eng.set_pde_params(*(co[:2] + [bad_nu] + co[3:]))
        same()
    with pytest.raises(pinn_native.PinnNativeError, match="not finite"):
        eng.set_pde_params(*(co[:4] + [np.nan] + co[5:]))
    same()
    with pytest.raises(pinn_native.PinnNativeError, match="6 coefficients"):
        eng.set_pde_params(1e-4)
    same()
    with pytest.raises(pinn_native.PinnNativeError, match="ensembles support Burgers"):
        pinn_native.Ensemble(layers, LB, UB, 4, pde="adr_ide", dtype="f64")
    same()
    assert np.array_equal(eng.get_pde_params(), np.array(adr_ref.ALL_NONZERO)) or \
        rel(eng.get_pde_params(), np.array(adr_ref.ALL_NONZERO)) < 1e-15          # nu goes through log and exp
    eng.close()
    # the other kinds have no trainable coefficients to choose
    other = pinn_native.Engine(layers, LB, UB, pde="adr", dtype="f64")
    with pytest.raises(pinn_native.PinnNativeError, match="only the adr_ide kind"):
        other.set_pde_trainable(1)
    other.close()
    e32 = make(layers, "f32", 0, theta, *S)
    for path in (1, 2, 7):
        with pytest.raises(pinn_native.PinnNativeError):
            e32.set_kernel_path(path)
    assert np.isfinite(e32.loss_grad()[0])
    e32.close()


def test_set_and_get_pde_params_write_and_read_the_tail():
    layers, S, theta, lo, go, *_ = case(8, 2048)
    eng = make(layers, "f64", 7, np.concatenate([theta[:-6], np.zeros(6)]), *S)
    eng.set_pde_params(*adr_ref.ALL_NONZERO)
    w = eng.get_weights()
    keep = [-6, -5, -3, -2, -1]
    assert np.array_equal(w[:-6], theta[:-6]) and np.array_equal(w[keep], theta[keep])
    assert abs(w[-4] - np.log(adr_ref.ALL_NONZERO[2])) <= 4 * np.finfo(float).eps * abs(w[-4])      # log nu in the nu slot
    loss, grad, _ = eng.loss_grad()
    assert abs(loss - lo) / lo < 1e-12 and rel(grad, go) < 1e-11
    eng.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_residual_at_predict_error_and_a_rad_draw(dtype):
    from oracle import mlp
    layers, S, theta, *_ = case(8, 2048)
    X_f, X_u, u, X_lo, X_hi = S
    eng = make(layers, dtype, 7 if dtype == "f64" else 0, theta, *S)
    rs = np.random.RandomState(1)
    X = LB + (UB - LB) * rs.uniform(size=(5000, 2))
    want = mlp.forward_value(mlp.unpack(theta[:-6], layers), X, LB, UB)
    got = eng.predict(X)
    assert np.max(np.abs(got - want)) <= (1e-12 if dtype == "f64" else 3e-6) * max(1.0, np.max(np.abs(want)))
    target = np.sin(3 * X[:, 0:1]) * np.cos(X[:, 1:2])
    e = eng.error_l2(X, target)
    e_np = np.linalg.norm(target - got, 2) / np.linalg.norm(target, 2)
    assert abs(e - e_np) / e_np < 1e-13
    assert rel(eng.residual_at(X), ref.residual(theta, layers, LB, UB, X)) < TOL[dtype]["res"]
    # one residual-adaptive draw with the current coefficients: the restatement fed with residual_at at the pool
    n_pool, seed = 20000, 0x5EED0000 + 17
    P = rad_ref.pool_points(n_pool, seed, LB, UB, dtype)
    eng.rad_collocation(3000, seed, n_pool, k=1, c=1.0)
    got = eng.get_collocation()
    want, idx = rad_ref.rad_draw(P, eng.residual_at(P), seed, 0, 3000, 1, 1.0)
    assert got.shape == (3000, 2) and np.array_equal(got, want) and len(np.unique(idx)) > 1
    loss, grad, _ = eng.loss_grad()
    lo, go, _ = ref.loss_grad(theta, layers, LB, UB, got, X_u, u, X_lo, X_hi)
    eng.close()
    assert abs(loss - lo) <= TOL[dtype]["loss"] * max(1.0, abs(lo))
    assert rel(grad, go) < TOL[dtype]["grad"]


# ---- 12. the script ----------------------------------------------------------------------------------------------------------------
LINE = re.compile(r"^(tf_epoch|nt_epoch) =\s+(\d+)\s+elapsed = \d\d:\d\d \(\+\d\d\.\d\)  loss = (\S+)  (.*)$")
SHORT_HP = {"N_u": 512, "noise": 0.0, "layers": layers_of(8), "seed": 1234,
            "tf_epochs": 10, "tf_lr": 0.003, "tf_b1": 0.9, "tf_eps": None,
            "nt_epochs": 10, "nt_lr": 0.8, "nt_ncorr": 50, "log_frequency": 5,
            "adr_trainable": ["nu", "r1", "r3"], "adr_init": [0.0, 0.0, 1e-3, -1.0, 0.0, 1.0]}


def test_script_runs_logs_its_coefficients_and_a_checkpoint_keeps_the_tail(tmp_path):
    """ide_cont_allen_cahn.py with a short schedule as a child process; the number behind its first logged loss as in
    tests/test_gpu_adr.py: the same model built here from the same hp and seeds evaluates the loss at the initial weights,
    that value agrees with the restatement to 1e-12, and the child's first line prints exactly that value"""
    hp_file = tmp_path / "hp.json"
    hp_file.write_text(json.dumps(SHORT_HP))
    env = dict(os.environ, MPLBACKEND="Agg")
    env.pop("PINN_NO_PLOT", None)
    res = subprocess.run([sys.executable, os.path.join(PKG, "1d-allen-cahn", "ide_cont_allen_cahn.py"), str(hp_file)],
                         cwd=PKG, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    out = res.stdout
    assert "-- Starting Adam optimization --" in out and "-- Starting LBFGS optimization --" in out
    rows = [m.groups() for m in map(LINE.match, out.splitlines()) if m]
    assert [(r[0], int(r[1])) for r in rows[:2]] == [("tf_epoch", 0), ("tf_epoch", 5)]
    assert any(r[0] == "nt_epoch" for r in rows)
    for r in rows:                                   # every progress line carries the three trainable values
        vals = dict(re.findall(r"(\w+) = (\S+)", r[3]))
        assert {"nu", "r1", "r3"} <= set(vals) and not {"a0", "a1", "r2"} & set(vals)
        assert np.isfinite(float(r[2])) and all(np.isfinite(float(vals[n])) for n in ("nu", "r1", "r3")) and float(vals["nu"]) > 0
    final = out[out.index("identified coefficients"):]
    got = {m.group(1): (float(m.group(2)), m.group(3)) for m in
           re.finditer(r"^\s+(a0|a1|nu|r1|r2|r3)\s+=\s+(\S+)\s+\(.*\)\s+(trained|frozen)$", final, re.M)}
    assert sorted(got) == sorted(ref.NAMES)
    assert [n for n in ref.NAMES if got[n][1] == "trained"] == ["nu", "r1", "r3"]
    assert got["a0"][0] == 0.0 and got["a1"][0] == 0.0 and got["r2"][0] == 0.0
    m = re.search(r"Saving results to directory\s+(\S+)", out)
    assert m and os.path.isfile(os.path.join(m.group(1), "hp.json")) and os.path.isfile(os.path.join(m.group(1), "weights.npy"))
    saved = np.load(os.path.join(m.group(1), "weights.npy"))
    assert saved.shape == (ref.n_net(SHORT_HP["layers"]) + 6,)
    assert abs(np.exp(saved[-4]) - got["nu"][0]) <= 1e-8 * got["nu"][0] and saved[-6] == 0.0 and saved[-5] == 0.0 and saved[-2] == 0.0

    # the number behind the first line, and a checkpoint round trip of the tail
    import neuralnetwork as nn
    argv, sys.argv = sys.argv, sys.argv[:1]          # the script reads an hp file from its command line when imported ...
    stream = dict(nn._INIT_STREAM)                   # ... and restarts the initialisers' stream: put back for the tests behind
    try:
        import ide_cont_allen_cahn as script
    finally:
        sys.argv = argv
        nn._INIT_STREAM.update(stream)
    from logger import Logger
    np.random.seed(1234)
    x, t, Exact_u, X_star, u_star, X_u, u, ub, lb = script.prep_data(
        SHORT_HP["N_u"], noise=0.0, cache_dir=os.path.join(PKG, "1d-allen-cahn", "results"))
    pinn = script.AllenCahnIdentificationNN(dict(SHORT_HP), Logger(dict(SHORT_HP, log_frequency=10 ** 9)), X_u, ub, lb)
    pinn._bind(X_u, u)
    assert pinn._engine.kernel_path() == 7
    w0 = np.asarray(pinn.get_weights()).ravel()
    assert np.array_equal(w0[-6:], [0.0, 0.0, np.log(1e-3), -1.0, 0.0, 1.0])
    assert pinn.get_params(numpy=True)[3:] == (-1.0, 0.0, 1.0) and abs(pinn.get_params(numpy=True)[2] - 1e-3) < 1e-18
    loss0 = pinn._engine.loss_grad()[0]
    lo, _, _ = ref.loss_grad(w0, SHORT_HP["layers"], lb, ub, X_u, X_u, u, None, None, mask=NU_R1_R3)
    print("first loss: engine %.17g restatement %.17g printed %s" % (loss0, lo, rows[0][2]))
    assert abs(loss0 - lo) / lo < 1e-12
    assert rows[0][2] == "%.4e" % loss0
    pinn._engine.adam_run(3)
    w3 = np.asarray(pinn.get_weights()).ravel()
    assert w3[-4] != w0[-4] and w3[-6] == 0.0
    ckpt = pinn.save_weights(str(tmp_path / "ckpt.npy"))
    pinn.set_weights(w0)
    pinn.load_weights(ckpt)
    assert np.array_equal(np.asarray(pinn.get_weights()).ravel(), w3)
    assert np.array_equal(pinn._engine.get_pde_params(), ref.raw_coeffs(w3))
