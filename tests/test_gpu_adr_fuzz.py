"""GPU: the adr family on fuzzed inputs (tests/helpers/adr_fuzz.py, pinned on the CPU by tests/test_adr_fuzz_host.py): random
shapes, any subset of {pairs, data, Robin points, source, coefficient fields}, drawn coefficients (nu = 0, nu < 0, several
zero columns), nets in the tail of tanh, the launch-plan boundary moved by Robin points alone, reused contexts, ensembles.

Parity.  Every case x eligible config (float64 on paths 0 and 7, float32 on path 0; off-shape nets and float32 on path 0 only)
in a fresh context: loss_grad(), residual() and robin_residual() against the restatement in the wider type.  Every quantity on
its own scale (gradient entries A, f A_f, r A_r, the loss and its terms the loss), bound = grad_entries.K of the path's family
x max(plain error of the restatement in the compute dtype, 32 u).  A float64 set of more than LONGDOUBLE_POINTS points has no
80-bit run: the float64 restatement and ASSUMED_F64_ULPS, as grad_entries.judge.  Ungained cases also keep the whole-vector
bounds TOL of tests/test_gpu_adr.py.  Point-weight cases have a float64 restatement only (adr_pw_ref): TOL.

Reused contexts.  One Engine per (kind, layers, dtype, path) walks its cases (adr_fuzz.walk: sizes shrink and grow across the
n_cu-tile boundary, every feature goes on, off and on); between cases the context is dirtied (3 Adam steps, 2 L-BFGS
iterations, a predict at another point count, a Latin-hypercube draw that the next explicit set replaces).  Loss, gradient,
terms, f and r must be np.array_equal to a fresh context's: a difference is stale device state, not rounding.

Ensembles.  Four AdrEnsemble cases, K = 3, per-member sets: against the restatement by the rule above and bit-equal to a solo
engine.

Measured on an MI355X (256 compute units; profiles/adr_fuzz_measured.jsonl), largest ratio deviation / yardstick per family, dtype
and quantity, with the allowance K it is held to; no quantity needed an allowance of its own:

  family dtype  K    grad                                  f                                   r                       loss
  w20    f64    8    4.02  path 0, edge 8x20 N_f = 1       2.94  paths 0 and 7, adr_ide 4x20   0.51  path 0, 4x20 x 3  0.12
  w20    f32    9    1.44  path 0, edge 8x20 N_f = 1       1.37  path 0, 6x20 fields           1.29  path 0, 4x20 x 3  0.11
  t16    f64    20   0.92  path 0, 3x33 x 3                0.47                                0.66                    0.13
  t16    f32    20   0.41  path 0, 3x33 x 3                0.41                                0.54                    0.12
  ensembles (w20 f64, path 7)  4.97  4x20 N_f = 1, first layer x 12   1.10   -   0.19

Three figures are above K / 3, all are rounding and all stay below K, which does not move:
  * 4.97 (path 7) and 4.02 (path 0), gradients of sets of ONE collocation point and nothing else: no sum over points averages
    the rounding of the single term.  Path 7: plain float64 numpy with tanh in the quotient form of tanh_d
    (grad_entries._tanh "bf") is off by 1749 u of A on that case where the library's tanh gives 344 u: 5.08 x, the kernel
    measures 4.97 x.  The same 8x20 single-point case is at 1.07 on path 7.
  * 2.94, f of the adr_ide draw with every weight x 3 (1506 points: no 80-bit run, the yardstick is the assumed 64 u).  The
    float64 restatement itself is off by 123 u of A_f against longdouble on that case, both paths return the same figure, and
    the gradient of the same case is at 1.11 / 0.94.
Reused contexts: all 30 groups bit-equal at every step (198 steps).  The empty collocation set: accepted, terms[0] == 0.0.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import adr_fuzz as af  # noqa: E402
import grad_entries as ge  # noqa: E402
from test_gpu_adr import TOL  # noqa: E402

pytestmark = pytest.mark.gpu

HOST_CASES = af.cases()                      # ids and configs for collection; the plan-boundary cases are rebuilt for the device
PARITY = [(i, d, p) for i, c in enumerate(HOST_CASES) for d in ("f64", "f32") if d in c["paths"] for p in c["paths"][d]]
GROUPS = sorted(af.config_groups(HOST_CASES))
EPS = float(np.finfo(float).eps)


def n_cu():
    import pinn_native
    return pinn_native.device_info()["compute_units"]


def device_cases():
    return af.cases(n_cu())


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)))
                 / max(float(np.max(np.abs(b))), 1e-300)) if np.size(b) else 0.0


# ---- a case in a context ----------------------------------------------------------------------------------------------------------
def apply(eng, case, state=None):
    """hand `case` to the context `eng`: every set, feature, coefficient and weight, whatever it held before.  state: what the
    walk knows of the context ({"sets": id of the case whose point sets it holds, "pw": bool}); None for a fresh context.
    Point sets that are the context's own already (the bare twin of a case) are not sent again, so that the source and the
    fields are replaced and removed in place."""
    x = af.inputs(case["id"])
    st = state if state is not None else {"sets": None, "pw": False}
    if st["pw"]:
        eng.pw_disable()
        st["pw"] = False
    sets_id = case["id"].replace("-bare", "")
    if case["kind"] != "adr_ide":
        eng.set_pde_params(*case["coeffs"])
    if st["sets"] != sets_id:
        eng.set_collocation(x["X_f"])
        eng.set_data(x["X_u"], x["u"])
        eng.set_boundary(x["X_lo"], x["X_hi"])
        st["sets"] = sets_id
    if case["kind"] == "adr_ide":
        eng.set_pde_params(*case["coeffs"])
        eng.set_pde_trainable(case["mask"])
    else:
        eng.set_source(x["s"])
        eng.set_coef_fields(x["K"])
        if x["robin"] is not None:
            eng.set_robin(*x["robin"])
        elif eng.n_w:
            eng.set_robin(np.zeros((0, 2)), np.zeros(0), np.zeros(0), np.zeros(0))
        assert eng.has_source == case["source"] and eng.has_coef_fields == case["fields"] and eng.n_w == case["n_w"]
    eng.set_weights(x["w"])
    if case["kind"] == "adr_pw":
        lam_u, lam_f, lam_b = x["lam"]
        eng.pw_set(lam_u if case["n_0"] else None, lam_f, lam_b if case["n_b"] else None)
        st["pw"] = True
    return st


def new_engine(case, dtype, path):
    from pinn_native import Engine
    eng = Engine(case["layers"], af.LB, af.UB, pde="adr_ide" if case["kind"] == "adr_ide" else "adr", dtype=dtype)
    eng.set_kernel_path(path)          # no skip: a config that is listed must exist
    assert eng.kernel_path() == path
    return eng


def evaluate(eng, case):
    loss, grad, terms = eng.loss_grad()
    f = eng.residual()
    r = eng.robin_residual() if case["kind"] != "adr_ide" else np.zeros(0)
    assert f.shape == (case["n_f"], 1) and r.shape == (case["n_w"],)
    return {"loss": loss, "grad": grad, "terms": tuple(terms), "f": f, "r": r}


_FRESH = {}


def fresh(case, dtype, path):
    """what a context that has seen nothing else computes for the case (once per case and config)"""
    key = (case["id"], dtype, path)
    if key not in _FRESH:
        eng = new_engine(case, dtype, path)
        apply(eng, case)
        _FRESH[key] = evaluate(eng, case)
        eng.close()
    return _FRESH[key]


def same_bits(a, b):
    return (a["loss"] == b["loss"] and np.array_equal(a["grad"], b["grad"]) and np.array_equal(a["terms"], b["terms"])
            and np.array_equal(a["f"], b["f"]) and np.array_equal(a["r"], b["r"]))


# ---- 1. parity ----------------------------------------------------------------------------------------------------------------------
def judge(record, case, dtype, path, got, tag, ref=None, yard=None):
    """every quantity against the wider restatement on its own scale; -> {quantity: ratio deviation / yardstick}.  ref, yard:
    the restatement and yardsticks of other inputs than the case's own (a block of it, tests/test_gpu_adr_shards.py)"""
    cid = case["id"]
    ref = af.reference(cid, dtype) if ref is None else ref
    dev, yard = af.deviations(got, ref), af.yardsticks(cid, dtype) if yard is None else yard
    k = af.allowance(case, path, dtype)
    u = ge.unit_roundoff(ge.DTYPES[dtype])
    ratio = {q: dev[q] / yard[q] for q in af.QUANTITIES}
    print("%s %s %s path %d: %s (K %g; yardsticks %s u)" % (tag, cid, dtype, path, " ".join("%s %.3f" % (q, ratio[q]) for q in af.QUANTITIES),
                                                           k, " ".join("%.0f" % (yard[q] / u) for q in af.QUANTITIES)))
    record(tag=tag, case=cid, dtype=dtype, path=path, family=ge.family_of(path, case["layers"], dtype), K=k,
           **{"ratio_" + q: ratio[q] for q in af.QUANTITIES}, **{"yard_u_" + q: yard[q] / u for q in af.QUANTITIES})
    for q in af.QUANTITIES:
        assert dev[q] <= k * yard[q], "%s of %s (%s, path %d) is off by %.3e of its scale: %.2f x the yardstick, allowance %g" % (
            q, cid, dtype, path, dev[q], ratio[q], k)
    return ratio


def whole_vector(case, dtype, got):
    """TOL of tests/test_gpu_adr.py: loss and terms as shares of the loss, gradient, f and r by their largest entries"""
    ref = af.reference(case["id"], dtype) if case["kind"] != "adr_pw" else af.restate(case, np.float64)
    lo = float(ref["loss"])
    tol = TOL[dtype]
    assert abs(got["loss"] - lo) / lo < tol["loss"]
    assert max(abs(g - float(t)) for g, t in zip(got["terms"], ref["terms"])) / lo < tol["loss"] * 10
    assert rel(got["grad"], ref["grad"]) < tol["grad"]
    if case["kind"] == "adr_pw":        # adr_pw_ref returns no f: the unweighted residual of the same sets
        x = af.inputs(case["id"])
        f = af.restate_adr(case["layers"], x["w"], case["coeffs"], x["X_f"])["f"]
        assert rel(got["f"], f) < tol["res"]
    else:
        assert rel(got["f"], ref["f"]) < tol["res"] and rel(got["r"], ref["r"]) < tol["res"]


@pytest.mark.parametrize("i,dtype,path", PARITY, ids=["%s-%s-p%d" % (HOST_CASES[i]["id"], d, p) for i, d, p in PARITY])
def test_parity_with_the_restatement(record, i, dtype, path):
    case = device_cases()[i]
    if dtype == "f64" and not ge.longdouble_is_wider():
        pytest.skip("np.longdouble is no wider than float64 here")
    got = fresh(case, dtype, path)
    if case["plan"]:
        cu = n_cu()
        plan = af.plan_of(case, cu)
        print("%s: %d tiles on %d compute units -> %s" % (case["id"], af.n_tiles(case), cu, plan))
        spills = case["n_w"] in (40, 1)
        assert af.n_tiles(case) == cu + spills and plan == ("tile-loop" if spills else "one-tile")
        assert (af.n_points(case) - case["n_w"] + 63) // 64 <= cu        # without the Robin points: one tile per compute unit
    if case["n_f"] == 0:
        assert got["terms"][0] == 0.0                                     # an empty collocation set adds nothing
    if case["kind"] == "adr_pw":
        whole_vector(case, dtype, got)
        return
    judge(record, case, dtype, path, got, "parity")
    if case["cls"] == "ungained":
        whole_vector(case, dtype, got)


@pytest.mark.parametrize("dtype,path", [("f64", 0), ("f64", 7), ("f32", 0)])
def test_empty_collocation_set_contract(dtype, path):
    """a set without collocation points is accepted (the residual term is 0.0, residual() is empty, Robin points
    still count); a context whose only points are Robin points has no training set and is refused with PINN_EINVAL before any
    launch, and works once it is given one"""
    import pinn_native
    case = next(c for c in device_cases() if c["n_f"] == 0)
    x = af.inputs(case["id"])
    eng = new_engine(case, dtype, path)
    eng.set_pde_params(*case["coeffs"])
    eng.set_robin(*x["robin"])
    eng.set_weights(x["w"])
    n_before = eng.status()[0]
    for call in (eng.loss_grad, eng.residual, eng.robin_residual):
        with pytest.raises(pinn_native.PinnNativeError, match=r"no training points set \(code -1\)"):
            call()
    assert eng.status()[0] == n_before                                       # nothing was evaluated
    apply(eng, case)
    got = evaluate(eng, case)
    eng.close()
    assert got["terms"][0] == 0.0 and got["f"].shape == (0, 1) and got["terms"][1] > 0 and got["terms"][2] > 0
    assert same_bits(got, fresh(case, dtype, path))


# ---- 2. reused contexts -------------------------------------------------------------------------------------------------------------
def dirty(eng, case, step, lhs):
    """leave traces in everything a context keeps between evaluations"""
    eng.adam_init(1e-3, 0.9, 0.999, 1e-7)
    eng.adam_run(3)
    eng.lbfgs_begin(2, 0.8, 50, EPS)
    eng.lbfgs_run(2)
    n = (af.n_points(case) * 7 + 13 * step) % 997 + 1
    rs = np.random.RandomState(step)
    eng.predict(np.column_stack([rs.uniform(-1, 1, n), rs.uniform(0, 1, n)]))
    if lhs:
        eng.lhs_collocation(case["n_f"] + 100 + step, 0x5EED0000 + step)


@pytest.mark.parametrize("kind,layers,dtype,path", GROUPS, ids=["%s-%dx%d-%s-p%d" % (k, len(l) - 2, l[1], d, p) for k, l, d, p in GROUPS])
def test_a_reused_context_computes_what_a_fresh_one_does(kind, layers, dtype, path):
    group = af.config_groups(device_cases())[(kind, layers, dtype, path)]
    order = af.walk(group)
    cu = n_cu()
    tiles = [af.n_tiles(c) for c in order]
    if any(c["plan"] for c in group):
        ups = sum(a <= cu < b for a, b in zip(tiles[:-1], tiles[1:]))
        downs = sum(b <= cu < a for a, b in zip(tiles[:-1], tiles[1:]))
        assert ups >= 1 and downs >= 1, tiles
        for name in ("robin", "source", "fields"):
            assert af.on_off_on(order, af.FEATURES[name]), name
    assert any(a > b for a, b in zip(tiles[:-1], tiles[1:])) or len(group) == 1
    eng = new_engine(order[0], dtype, path)
    state, differ = None, []
    for step, case in enumerate(order):
        state = apply(eng, case, state)
        got, want = evaluate(eng, case), fresh(case, dtype, path)
        if not same_bits(got, want):
            differ.append((step, case["id"], [q for q in ("loss", "grad", "terms", "f", "r") if not np.array_equal(got[q], want[q])]))
        nxt = order[step + 1] if step + 1 < len(order) else None
        in_place = nxt is not None and nxt["id"].replace("-bare", "") == case["id"].replace("-bare", "")
        dirty(eng, case, step, lhs=not in_place and case["kind"] != "adr_pw")
        if not in_place:
            state["sets"] = None
        else:
            eng.set_weights(af.inputs(case["id"])["w"])
            eng.loss_grad()                           # the set is assembled and clean: the next setters work in place
    eng.close()
    print("%s %dx%d %s path %d: %d steps, tiles %s" % (kind, len(layers) - 2, layers[1], dtype, path, len(order), tiles))
    assert not differ, differ


# ---- 3. ensembles -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(af.ENSEMBLE_SHAPES)), ids=["b%d-u%d-f%d" % s for s in af.ENSEMBLE_SHAPES])
def test_ensemble_members_against_the_restatement_and_a_solo_engine(record, i):
    from pinn_native import AdrEnsemble
    if not ge.longdouble_is_wider():
        pytest.skip("np.longdouble is no wider than float64 here")
    members = af.ensemble_members(i)
    xs = [af.inputs(c["id"]) for c in members]
    n_b, n_0, n_f = af.ENSEMBLE_SHAPES[i]
    ens = AdrEnsemble(members[0]["layers"], af.LB, af.UB, af.ENSEMBLE_K)
    ens.set_collocation(np.stack([x["X_f"] for x in xs]))
    if n_0:
        ens.set_data(np.stack([x["X_u"] for x in xs]), np.stack([x["u"] for x in xs]))
    if n_b:
        ens.set_boundary(np.stack([x["X_lo"] for x in xs]), np.stack([x["X_hi"] for x in xs]))
    ens.set_pde_params(np.asarray([c["coeffs"] for c in members]))
    ens.set_weights(np.stack([x["w"] for x in xs]))
    losses, grads, terms = ens.loss_grad()
    ens.close()
    for k, case in enumerate(members):
        solo = fresh(case, "f64", 7)
        assert losses[k] == solo["loss"] and np.array_equal(grads[k], solo["grad"]) and np.array_equal(terms[k], solo["terms"]), k
        got = dict(solo, loss=losses[k], grad=grads[k], terms=tuple(terms[k]))      # f and r: the solo engine's (no ensemble call)
        judge(record, case, "f64", 7, got, "ensemble")
