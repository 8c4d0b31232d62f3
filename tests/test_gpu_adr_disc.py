"""GPU: the discrete-time adr kind (pde "adr_disc": the six-coefficient operator and the periodic groups of
csrc/kernels_disc.h) against tests/helpers/adr_disc_oracle.py, itself pinned by tests/test_adr_disc_host.py.
Tolerances are those tests/test_gpu_disc.py holds kinds 3 and 4 to: loss and terms f64 1e-12 / f32 2e-5 of the total loss,
gradient f64 1e-11 / f32 2e-4 of its largest entry, network values f64 1e-12 / f32 5e-6, stage predictions f64 1e-10 /
f32 1e-3.  Every loss_grad is taken twice and must return the same bits."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import adr_disc_oracle as ado  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = {"f64": (1e-12, 1e-11), "f32": (2e-5, 2e-4)}
TOL_VALUE = {"f64": 1e-12, "f32": 5e-6}
TOL_STAGE = {"f64": 1e-10, "f32": 1e-3}
LB, UB = [-1.0], [1.0]
LAYERS, Q = [1, 23, 23, 7], 5


def rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300)


def make_engine(layers, dtype, sets=(None, None), coef=None, pairs=None, order=1, w=None, pde="adr_disc"):
    import pinn_native
    eng = pinn_native.Engine(layers, LB, UB, pde=pde, dtype=dtype)
    for s, st in enumerate(sets):
        if st is not None:
            eng.disc_set_stage(s, *st)
    if coef is not None:
        eng.set_pde_params(*coef)
    if pairs is not None:
        eng.disc_set_periodic(pairs[0], pairs[1], order)
    if w is not None:
        assert eng.n_params == w.size
        eng.set_weights(w)
    return eng


def check(eng, dtype, w, layers, sets, coef, per, tag=""):
    """loss, terms and gradient against the oracle; a second evaluation returns the same bits -> (loss, grad, terms)"""
    loss, grad, terms = eng.loss_grad()
    lo, go, ex = ado.loss_grad(w, layers, LB, UB, sets, coef, per)
    tl, tg = TOL[dtype]
    d_loss, d_grad = abs(loss - lo) / abs(lo), rel(grad, go)
    d_terms = max(abs(terms[k] - ex["terms"][k]) for k in range(3)) / abs(lo)
    print("%s %s: loss %.3e terms %.3e grad %.3e" % (tag, dtype, d_loss, d_terms, d_grad))
    assert d_loss <= tl and d_terms <= tl and d_grad <= tg, (tag, d_loss, d_terms, d_grad)
    loss2, grad2, terms2 = eng.loss_grad()
    assert loss2 == loss and np.array_equal(grad2, grad) and np.array_equal(terms2, terms), tag
    return loss, grad, terms


_COEFS = ado.coefficient_vectors()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("k", range(7))
def test_operator_one_coefficient_at_a_time(k, dtype):
    sets, pairs, w = ado.case(LAYERS, Q, 17, 3, 3, seed=10 + k)
    eng = make_engine(LAYERS, dtype, sets, _COEFS[k], pairs, 1, w)
    try:
        assert np.array_equal(eng.get_pde_params(), np.array(_COEFS[k]))
        check(eng, dtype, w, LAYERS, sets, _COEFS[k], pairs + (1,), "coef%d" % k)
    finally:
        eng.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("n_pairs", [1, 8, 9])
def test_pair_count_edges(n_pairs, order, dtype):
    """1 pair, one full group of 8, a second group holding one pair; next to stage sets of 1, 17 and 33 points"""
    for n0 in (1, 17, 33):
        sets, pairs, w = ado.case(LAYERS, Q, n0, 3, n_pairs, seed=40 + n0 + n_pairs)
        eng = make_engine(LAYERS, dtype, sets, _COEFS[6], pairs, order, w)
        try:
            _, _, terms = check(eng, dtype, w, LAYERS, sets, _COEFS[6], pairs + (order,), "pairs%d-o%d-n%d" % (n_pairs, order, n0))
            assert terms[2] > 0.0
        finally:
            eng.close()


def test_slot_subsets_and_removal():
    sets, pairs, w = ado.case(LAYERS, Q, 17, 3, 3, seed=5)
    coef = _COEFS[6]
    # the periodic set alone (f64 only: a difference of two near-equal wall values has no relative bound in f32)
    eng = make_engine(LAYERS, "f64", (None, None), coef, pairs, 1, w)
    try:
        _, _, terms = check(eng, "f64", w, LAYERS, [None, None], coef, pairs + (1,), "pairs-alone")
        assert terms[0] == 0.0 and terms[1] == 0.0 and terms[2] > 0.0
    finally:
        eng.close()
    for dtype in ("f64", "f32"):
        # stage sets alone, then all three slots, then the pairs removed again: the stage-only value bit for bit
        eng = make_engine(LAYERS, dtype, sets, coef, None, 1, w)
        try:
            loss0, grad0, terms0 = check(eng, dtype, w, LAYERS, sets, coef, None, "stages-alone")
            assert terms0[2] == 0.0
            eng.disc_set_periodic(pairs[0], pairs[1], 1)
            check(eng, dtype, w, LAYERS, sets, coef, pairs + (1,), "all-three")
            eng.disc_set_periodic([], [], 1)
            loss1, grad1, terms1 = eng.loss_grad()
            assert loss1 == loss0 and np.array_equal(grad1, grad0) and np.array_equal(terms1, terms0)
            # one stage set and the pairs
            eng.disc_set_stage(1, np.zeros(0), np.zeros(0), None)
            eng.disc_set_periodic(pairs[0], pairs[1], 0)
            check(eng, dtype, w, LAYERS, [sets[0], None], coef, pairs + (0,), "set0+pairs")
        finally:
            eng.close()
    # none of the three: refused at the evaluation
    import pinn_native
    eng = make_engine(LAYERS, "f64", (None, None), coef, None, 1, w)
    try:
        with pytest.raises(pinn_native.PinnNativeError, match="no stage set"):
            eng.loss_grad()
    finally:
        eng.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("layers,q", [([1, 50, 50, 101], 100), ([1, 50, 50, 71], 70), ([1, 30, 8], 5)],
                         ids=["two-chunks", "table-ends-inside-a-chunk", "n_out-beyond-q+1-H1"])
def test_column_edges(layers, q, dtype):
    sets, pairs, w = ado.case(layers, q, 37, 20, 3, seed=60 + q, wscale=0.9 / np.sqrt(layers[1]))
    eng = make_engine(layers, dtype, sets, _COEFS[6], pairs, 1, w)
    try:
        check(eng, dtype, w, layers, sets, _COEFS[6], pairs + (1,), "cols%d" % layers[-1])
    finally:
        eng.close()


def test_wide_hidden_layers_f32():
    """hidden width 100: the NT = 8 instantiation, float32 only; float64 refuses the width with the existing message"""
    import pinn_native
    layers, q = [1, 100, 100, 13], 12
    sets, pairs, w = ado.case(layers, q, 40, 2, 1, seed=70, wscale=0.3)
    eng = make_engine(layers, "f32", sets, _COEFS[6], pairs, 1, w)
    try:
        check(eng, "f32", w, layers, sets, _COEFS[6], pairs + (1,), "wide")
    finally:
        eng.close()
    with pytest.raises(pinn_native.PinnNativeError, match="hidden width"):
        pinn_native.Engine(layers, LB, UB, pde="adr_disc", dtype="f64")


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_default_coefficients_agree_with_kind_3(dtype):
    """a new adr_disc context holds Burgers' coefficients: same sets, same weights as a burgers_disc engine.  Not bit
    equality -- the expressions differ."""
    sets, _, w = ado.case(LAYERS, Q, 33, 16, 0, seed=80)
    a = make_engine(LAYERS, dtype, sets, None, None, 1, w)
    b = make_engine(LAYERS, dtype, sets, None, None, 1, w, pde="burgers_disc")
    try:
        assert np.array_equal(a.get_pde_params(), np.array(ado.BURGERS))
        b.set_pde_params(ado.BURGERS[2])
        la, ga, ta = a.loss_grad()
        lb_, gb, tb = b.loss_grad()
        tl, tg = TOL[dtype]
        assert abs(la - lb_) <= tl * abs(lb_) and rel(ga, gb) <= tg
        assert max(abs(ta[k] - tb[k]) for k in range(3)) <= tl * abs(lb_)
        assert a.loss_grad()[0] == la and np.array_equal(a.loss_grad()[1], ga)
        xs = np.linspace(-1.0, 1.0, 29)
        Pa, Pb = a.disc_predict(0, xs), b.disc_predict(0, xs)
        assert np.max(np.abs(Pa - Pb)) <= TOL_STAGE[dtype] * max(1.0, np.max(np.abs(Pb)))
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_predict_and_disc_predict(dtype):
    from oracle import mlp
    coef = ado.REACTION_HEAVY
    sets, pairs, w = ado.case(LAYERS, Q, 17, 3, 3, seed=90)
    eng = make_engine(LAYERS, dtype, sets, coef, pairs, 1, w)
    try:
        params = mlp.unpack(w, LAYERS)
        rs = np.random.RandomState(91)
        for n in (37, 1001):
            xs = np.sort(rs.uniform(-1, 1, n))
            U = eng.predict(xs[:, None])
            ref = mlp.forward_value(params, xs[:, None], np.array(LB), np.array(UB))
            d_val = np.max(np.abs(U - ref)) / max(1.0, np.max(np.abs(ref)))
            P = eng.disc_predict(0, xs)
            pred = ado.stage_prediction(params, xs, LB, UB, sets[0][2], coef)
            d_st = np.max(np.abs(P - pred)) / max(1.0, np.max(np.abs(pred)))
            P1 = eng.disc_predict(1, xs)                       # set 1 has no table: U itself
            d_st1 = np.max(np.abs(P1 - ref)) / max(1.0, np.max(np.abs(ref)))
            print("%s n %d: value %.3e stage %.3e stage1 %.3e" % (dtype, n, d_val, d_st, d_st1))
            assert U.shape == ref.shape and d_val <= TOL_VALUE[dtype]
            assert d_st <= TOL_STAGE[dtype] and d_st1 <= TOL_STAGE[dtype]
    finally:
        eng.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_ten_adam_steps_match_the_oracle(dtype):
    """hyper-parameters of tests/test_gpu_disc.py test_adam_trajectory_matches_reference_run (the golden run's hp)"""
    from conftest import golden
    hp = json.loads(str(np.load(golden("burgers_disc_eval_small.npz"))["hp"]))
    coef = ado.REACTION_HEAVY
    sets, pairs, w = ado.case(LAYERS, Q, 17, 3, 3, seed=95)
    ref, _ = ado.adam_losses(w, LAYERS, LB, UB, sets, coef, pairs + (1,), 10, hp["tf_lr"], hp["tf_b1"], 0.999, hp["tf_eps"])
    eng = make_engine(LAYERS, dtype, sets, coef, pairs, 1, w)
    try:
        eng.adam_init(hp["tf_lr"], hp["tf_b1"], 0.999, hp["tf_eps"])
        losses = eng.adam_run(10)
        d = np.max(np.abs(losses - ref) / ref)
        print("%s adam: %.3e" % (dtype, d))
        assert d <= (1e-10 if dtype == "f64" else 1e-4)
    finally:
        eng.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_five_lbfgs_iterations(dtype):
    sets, pairs, w = ado.case(LAYERS, Q, 17, 3, 3, seed=96)
    eng = make_engine(LAYERS, dtype, sets, ado.REACTION_HEAVY, pairs, 1, w)
    try:
        eng.lbfgs_begin(5, 0.8, 50, np.finfo(float).eps)
        it, losses, done = eng.lbfgs_run(5)
        print(dtype, list(it), list(losses), done)
        assert len(losses) >= 2 and np.all(np.isfinite(losses)) and np.all(np.diff(losses) <= 0.0)
        assert eng.status()[1] == 0
    finally:
        eng.close()


def test_errors():
    import pinn_native
    sets, pairs, w = ado.case(LAYERS, Q, 17, 3, 3, seed=97)
    # periodic pairs on a burgers_disc context: refused, the evaluation unchanged
    b = make_engine(LAYERS, "f64", sets, None, None, 1, w, pde="burgers_disc")
    try:
        before = b.loss_grad()
        with pytest.raises(pinn_native.PinnNativeError, match="adr_disc"):
            b.disc_set_periodic(pairs[0], pairs[1], 1)
        after = b.loss_grad()
        assert after[0] == before[0] and np.array_equal(after[1], before[1]) and np.array_equal(after[2], before[2])
    finally:
        b.close()
    eng = make_engine(LAYERS, "f64", sets, _COEFS[6], pairs, 1, w)
    try:
        before = eng.loss_grad()
        with pytest.raises(pinn_native.PinnNativeError, match="order"):
            eng.disc_set_periodic(pairs[0], pairs[1], 2)
        with pytest.raises(pinn_native.PinnNativeError, match="finite"):
            eng.disc_set_periodic([-1.0, np.nan], [1.0, 0.5], 1)
        with pytest.raises(pinn_native.PinnNativeError, match="6 coefficients"):
            eng.set_pde_params(0.1)
        with pytest.raises(pinn_native.PinnNativeError, match="not finite"):
            eng.set_pde_params(0.0, 1.0, np.nan, 0.0, 0.0, 0.0)
        assert np.array_equal(eng.get_pde_params(), np.array(_COEFS[6]))
        after = eng.loss_grad()
        assert after[0] == before[0] and np.array_equal(after[1], before[1])
        # what refuses the discrete-time kinds 3 and 4 refuses this one
        for call in (lambda: eng.set_collocation(np.zeros((4, 2))), lambda: eng.set_data(np.zeros((4, 2)), np.zeros((4, LAYERS[-1]))),
                     lambda: eng.residual()):
            with pytest.raises(pinn_native.PinnNativeError, match="discrete-time"):
                call()
    finally:
        eng.close()


LINE = re.compile(r"^(tf_epoch|nt_epoch) =\s+(\d+)\s+elapsed = \d\d:\d\d \(\+\d\d\.\d\)  loss = (\S+)  ")
END = re.compile(r"^Training finished \(epoch (\d+)\): duration = \d\d:\d\d  error = (\S+)  ")


def test_inf_disc_allen_cahn_script_runs(tmp_path):
    """1d-allen-cahn/inf_disc_allen_cahn.py as a child process (as tests/test_gpu_scripts.py starts scripts) with a small hp
    file: exits 0, prints the log header and both optimiser phases, and the last logged loss is below the first"""
    hp = {"N_n": 50, "q": 8, "layers": [1, 32, 32, 9], "tf_epochs": 20, "tf_lr": 0.001, "tf_b1": 0.9, "tf_eps": 1e-08,
          "nt_epochs": 20, "nt_lr": 0.8, "nt_ncorr": 50, "log_frequency": 10}
    hp_file = tmp_path / "hp.json"
    hp_file.write_text(json.dumps(hp))
    env = dict(os.environ, PINN_NO_PLOT="1", MPLBACKEND="Agg")
    res = subprocess.run([sys.executable, os.path.join(PKG, "1d-allen-cahn", "inf_disc_allen_cahn.py"), str(hp_file)],
                         cwd=PKG, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    out = res.stdout
    assert "Training started" in out and "-- Starting Adam optimization --" in out and "-- Starting LBFGS optimization --" in out
    rows = [(m.group(1), int(m.group(2)), float(m.group(3))) for m in map(LINE.match, out.splitlines()) if m]
    ends = [m for m in map(END.match, out.splitlines()) if m]
    assert any(r[0] == "tf_epoch" for r in rows) and any(r[0] == "nt_epoch" for r in rows)
    assert len(ends) == 1 and int(ends[0].group(1)) == 40 and np.isfinite(float(ends[0].group(2)))
    assert np.isfinite(rows[-1][2]) and rows[-1][2] < rows[0][2], (rows[0], rows[-1])
