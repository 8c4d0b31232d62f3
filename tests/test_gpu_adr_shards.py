"""GPU: the adr family on SHARDS of its fuzz cases (tests/helpers/adr_shards.py, pinned on the CPU by
tests/test_adr_shards_host.py): every point class cut into the contiguous blocks of a data-parallel run, every pinn_set_* call
given the size of the whole class as n_total, no communicator (the C-ABI contract, as tests/test_gpu_comm.py uses it).  Fresh
contexts on the eligible configurations of tests/test_gpu_adr_fuzz.py: float64 on paths 0 and 7, float32 on path 0, off-shape
nets on path 0.

(a) Each block against its own restatement in the wider type, by test_gpu_adr_fuzz.judge: every quantity on its own scale,
    bound = grad_entries.K of the path's family x max(plain error of the block's restatement, 32 u).  No allowance is added.
    Point-weighted blocks (adr_pw): adr_pw_ref.loss_grad with totals, whole vectors at TOL of tests/test_gpu_adr.py.
    A rank without a collocation block is accepted and its terms[0] == 0.0; a rank without any point is refused ("no training
    points set") and nothing is evaluated.
(b) The ranks' device results summed against the device's full-set result: every gradient entry within the sum of both sides'
    allowed deviations (K x yardstick x A of every block, plus K x yardstick x A of the full set), the loss and its three
    terms the same on the loss scale.  The bound is derived; the adr_ide coefficient entries are asserted on their own.
(c) Identities without a tolerance.  n_total == n is bit-equal to the call without n_total.  All four totals doubled: loss,
    terms and gradient are np.array_equal to 0.5 x the undoubled ones, f and r keep their bits, point-weighted evaluations
    included.  One total doubled: that class's term halves exactly, the other two terms keep their bits (terms[2]: on the
    sets with pairs only and with Robin points only).
    Configurations that satisfy the halving identity: ALL -- float64 path 0, float64 path 7 (one-tile and tile-loop plans,
    pw_set included), float32 path 0, the off-shape nets on path 0, adr_ide on paths 0 and 7.  Every kernel multiplies by
    inv_n = 1 / n_total, formed once on the host (engine.hip ensure_sets, pde_coef) and rounded once to the compute type;
    1 / (2 n) is exactly half of 1 / n in both types.
(d) A reused context walks rank 0 ... W-1 of a case, the full set, then the blocks of another world size, dirtied between steps
    (test_gpu_adr_fuzz.dirty), and is bit-equal to a fresh context at every step; set_collocation and set_robin with the same
    rows and another n_total take effect.
(e) SA-PINN (float64 Burgers, path 7): n_total = 2 n halves exactly, blocks add up, and after one Adam step with an ascent rate
    the weights are those of pinn_hip.h's formula with N = n_total, evaluated in longdouble from the device's own residuals.
(f) Ensembles, K = 3 (Ensemble; AdrEnsemble with shared and per-member sets): with n_total = 2 n and with a ragged block of a
    larger set member k is == / np.array_equal to a solo Engine given the same block and totals, set_boundary's total included.

Measured on an MI355X (256 compute units; profiles/adr_shards_measured.jsonl, written through the `record` fixture).  (a): largest
ratio deviation / yardstick over all blocks per family, dtype and quantity, with the allowance K it is held to; no quantity
needed an allowance of its own:

  family dtype  K    grad                                       f                                r                      loss
  w20    f64    8    5.09  path 7, 4x20 gain0 x 12, rank 1/8    2.65  adr_ide 4x20 x 3, 2/3      0.60  w3 over 8, 0/8   0.74
  w20    f32    9    3.05  path 0, shard-nof rank 7/8           2.73  4x20 x 3, rank 0/3         0.78                   0.38
  t16    f64    20   0.24  path 0, 5x33 gain0 x 12              0.37                             0.37                   0.06
  t16    f32    20   0.30  path 0, 5x33 gain0 x 12              0.29                             0.14                   0.04

Twelve gradient figures are above K / 3, all on blocks of 4 ... 23 points, all rounding, all below K, which does not move:
  * 5.09 (path 7), the block of 18 points of the net whose first layer is x 12: plain float64 numpy with tanh in the quotient
    form of tanh_d (grad_entries._tanh "bf") is off by 6.12 x the same yardstick (408 u of A) on that block, where the
    library's tanh defines the yardstick: the figure of tests/test_gpu_adr_fuzz.py (4.97 on a single point) on a smaller sum.
    Ranks 3 and 7 of the same case: 3.50 and 3.04.
  * 4.63, 4.39, 3.69, 3.25, 3.24 (path 0) and 3.15, 3.06, 2.85 (path 7), float64, and 3.05, float32 path 0: blocks of 4 ... 23
    points of the sets placed for an edge (f45 and f5 over 8, f70 over 3, the b3-u5-f17-w9 edge over 8).  A block of a handful
    of points has no sum over points that averages the rounding of its terms: tests/test_gpu_adr_fuzz.py measures 4.02 on
    path 0 and 4.97 on path 7 for its sets of one point.
(b): the largest share of the derived bound used is 0.009 for a gradient entry (path 7, blocks of 65, 64, 63 points), 0.004
for the loss and its terms, 0.002 for an adr_ide coefficient entry: the device's sums over blocks and over the full set differ
by far less than two independent roundings of K x yardstick would allow.
(c): every configuration satisfies every identity (58 configurations; 52 for the single totals).
(d): all 17 walks bit-equal at every step; both changed totals take effect.
(e): lam after one step: N = n and N = n_total are 2.8e8 u (collocation; smallest 1.2e4 u) and 2.5e11 u (data) of lam apart;
the device is within 0.87 u of the formula with N = n_total.  SA blocks against the full set: loss 1.0e-16, gradient 4.3e-17.

No script of the kind is launched on two ranks: NeuralNetwork refuses a data-parallel launch for "adr" and "adr_ide" by name
before any engine is made (the adr kind; pinned by tests/test_adr_host.py), so the n_total contract of these kinds
is reachable through the engine's own calls only, which is what this file uses.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import adr_fuzz as af  # noqa: E402
import adr_shards as sh  # noqa: E402
import grad_entries as ge  # noqa: E402
import test_gpu_adr_fuzz as fz  # noqa: E402
from test_gpu_adr import TOL  # noqa: E402

pytestmark = pytest.mark.gpu

HOST = [(sh.case_of(b), w) for b, w in sh.SHARDED]                      # ids and configs for collection
CONFIGS = [(i, d, p) for i, (c, _) in enumerate(HOST) for d in ("f64", "f32") if d in c["paths"] for p in c["paths"][d]]
CONFIG_IDS = ["%s-over%d-%s-p%d" % (HOST[i][0]["id"], HOST[i][1], d, p) for i, d, p in CONFIGS]
# (d): one case of every kind of context -- every feature, no collocation block, pairs alone, the plan edge, an off-shape net,
# adr_ide, point weights
WALKED = ("edge-adr-6x20-b3-u5-f17-w9-src-var", "shard-nof-adr-6x20-b9-u11-f5-w10-src-var", "shard-pairs-adr-4x20-b25-u0-f40-w0",
          "plan-robin-spills-adr-4x20-b3-u50-f16298-w40", "rnd-adr-3x7-b39-u81-f517-w78-src-var",
          "rnd-adr_ide-8x20-b23-u17-f449-w0", "rnd-adr_pw-8x20-b15-u62-f309-w0")
WALKS = [(i, d, p) for i, d, p in CONFIGS if sh.SHARDED[i][0] in WALKED]
WALK_IDS = [CONFIG_IDS[CONFIGS.index(k)] for k in WALKS]


def device_case(i):
    base, world = sh.SHARDED[i]
    return sh.case_of(base, fz.n_cu()), world


def need_wide(dtype):
    if dtype == "f64" and not ge.longdouble_is_wider():
        pytest.skip("np.longdouble is no wider than float64 here")


# ---- a block in a context ---------------------------------------------------------------------------------------------------------
def attach(eng, case, x):
    """what hangs on the collocation rows and is reset or made stale when they are replaced: source, fields, point weights"""
    if case["kind"] == "adr_ide":
        return
    if case["kind"] == "adr_pw":                                             # (no source, no fields: not combined with weights)
        eng.pw_set(*(a if len(a) else None for a in x["lam"]))
        return
    eng.set_source(x["s"] if x["s"] is not None and len(x["s"]) else None)
    eng.set_coef_fields(x["K"] if x["K"] is not None and len(x["K"]) else None)


def apply_block(eng, case, x, tot=None):
    """hand the block `x` of `case` to the context with the denominators `tot` (None: the calls without n_total)"""
    t = (lambda k: None) if tot is None else tot.get
    if case["kind"] != "adr_ide":
        eng.set_pde_params(*case["coeffs"])
    eng.set_collocation(x["X_f"], n_total=t("n_f_total"))
    eng.set_data(x["X_u"], x["u"], n_total=t("n_u_total"))
    eng.set_boundary(x["X_lo"], x["X_hi"], n_total=t("n_b_total"))
    if case["kind"] == "adr_ide":
        eng.set_pde_params(*case["coeffs"])
        eng.set_pde_trainable(case["mask"])
    elif x["robin"] is not None:
        eng.set_robin(*x["robin"], n_total=t("n_w_total"))
    elif eng.n_w:
        eng.set_robin(np.zeros((0, 2)), np.zeros(0), np.zeros(0), np.zeros(0))
    eng.set_weights(x["w"])
    attach(eng, case, x)


_RUNS = {}


def run(case, world, rank, dtype, path, scale=None):
    """what a fresh context computes for the block with the global totals (scale: {total: factor}, None: as they are); once
    per block and config.  -> dict of test_gpu_adr_fuzz.evaluate"""
    key = (case["id"], world, rank, dtype, path, None if scale is None else tuple(sorted(scale.items())))
    if key not in _RUNS:
        x, tot = sh.block(case, world, rank)
        tot = {k: v * (scale or {}).get(k, 1) for k, v in tot.items()}
        eng = fz.new_engine(case, dtype, path)
        apply_block(eng, case, x, tot)
        _RUNS[key] = fz.evaluate(eng, sh.local(case, x))
        eng.close()
    return _RUNS[key]


def whole_vector(case, got, x, tot):
    """adr_pw_ref (float64 only, no scale A) with totals: TOL of tests/test_gpu_adr.py, as test_gpu_adr_fuzz.whole_vector"""
    ref = af.restate(case, np.float64, x, **tot)
    lo, tol = float(ref["loss"]), TOL["f64"]
    assert abs(got["loss"] - lo) / lo < tol["loss"]
    assert max(abs(g - float(t)) for g, t in zip(got["terms"], ref["terms"])) / lo < tol["loss"] * 10
    assert fz.rel(got["grad"], ref["grad"]) < tol["grad"]
    if len(x["X_f"]):
        f = af.restate_adr(case["layers"], x["w"], case["coeffs"], x["X_f"])["f"]
        assert fz.rel(got["f"], f) < tol["res"]


# ---- (a) every block against its restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("i,dtype,path", CONFIGS, ids=CONFIG_IDS)
def test_every_block_against_its_restatement(record, i, dtype, path):
    import pinn_native
    need_wide(dtype)
    case, world = device_case(i)
    cu = fz.n_cu()
    if case["plan"]:
        assert af.plan_of(case, cu) == "tile-loop"
    worst = {q: 0.0 for q in af.QUANTITIES}
    for rank in range(world):
        x, tot = sh.block(case, world, rank)
        loc = sh.local(case, x)
        if sh.is_empty(x):                                                   # Robin points alone are no training set
            eng = fz.new_engine(case, dtype, path)
            apply_block(eng, case, x, tot)
            n_before = eng.status()[0]
            with pytest.raises(pinn_native.PinnNativeError, match=r"no training points set \(code -1\)"):
                eng.loss_grad()
            assert eng.status()[0] == n_before
            eng.close()
            continue
        got = run(case, world, rank, dtype, path)
        if case["plan"]:
            assert af.plan_of(loc, cu) == "one-tile" and af.n_tiles(loc) < cu
        if loc["n_f"] == 0:
            assert got["terms"][0] == 0.0 and got["f"].shape == (0, 1)
        if case["n_f"] and case["kind"] == "adr" and loc["n_0"] == 0:
            assert got["terms"][1] == 0.0
        if case["kind"] == "adr_pw":
            whole_vector(case, got, x, tot)
            continue
        ratio = fz.judge(record, case, dtype, path, got, "shard %d/%d" % (rank, world), ref=sh.reference(case["id"], world, rank, dtype),
                         yard=sh.yardsticks(case["id"], world, rank, dtype))
        worst = {q: max(worst[q], ratio[q]) for q in af.QUANTITIES}
    if case["kind"] != "adr_pw":
        record(tag="shards-worst", case=case["id"], world=world, dtype=dtype, path=path, family=ge.family_of(path, case["layers"], dtype),
               K=af.allowance(case, path, dtype), **{"ratio_" + q: worst[q] for q in af.QUANTITIES})


# ---- (b) the blocks add up ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i,dtype,path", CONFIGS, ids=CONFIG_IDS)
def test_blocks_add_up_to_the_full_set(record, i, dtype, path):
    need_wide(dtype)
    case, world = device_case(i)
    parts = [run(case, world, r, dtype, path) for r in range(world) if not sh.is_empty(sh.block(case, world, r)[0])]
    full = run(case, 1, 0, dtype, path)
    assert len(parts) >= 1 and (len(parts) >= 2 or af.n_points(case) < 2 * world)
    if case["kind"] == "adr_pw":
        # no scale A: every side is within TOL of its restatement by its largest entry, so the sum is within the sum of those
        s, tol = sh.summed(parts), TOL["f64"]
        assert abs(float(s["loss"]) - full["loss"]) < tol["loss"] * (sum(p["loss"] for p in parts) + full["loss"])
        assert max(abs(float(a) - b) for a, b in zip(s["terms"], full["terms"])) < 10 * tol["loss"] * (sum(p["loss"] for p in parts) + full["loss"])
        room = tol["grad"] * (sum(np.max(np.abs(p["grad"])) for p in parts) + np.max(np.abs(full["grad"])))
        assert np.max(np.abs(np.asarray(s["grad"], dtype=np.float64) - full["grad"])) < room
        return
    k = af.allowance(case, path, dtype)
    bg, blo = sh.additive_bound(case, world, dtype, k)
    share_g, share_lo, shares = sh.additive_share(parts, full, bg, blo)
    tail = float(np.max(shares[-6:])) if case["kind"] == "adr_ide" else 0.0
    print("%s over %d %s path %d: gradient %.3f of the derived bound, loss and terms %.3f%s" % (
        case["id"], world, dtype, path, share_g, share_lo, ", coefficient entries %.3f" % tail if case["kind"] == "adr_ide" else ""))
    record(tag="shards-add-up", case=case["id"], world=world, dtype=dtype, path=path, K=k, share_grad=share_g, share_loss=share_lo,
           share_tail=tail)
    assert share_g <= 1.0 and share_lo <= 1.0
    if case["kind"] == "adr_ide":                                            # the tail of the gradient adds up too
        trained = np.array([(case["mask"] >> j) & 1 for j in range(6)], dtype=bool)
        assert tail <= 1.0 and np.all(full["grad"][-6:][trained] != 0.0) and np.all(full["grad"][-6:][~trained] == 0.0)
        assert all(np.all(p["grad"][-6:][~trained] == 0.0) for p in parts)


# ---- (c) identities without a tolerance ---------------------------------------------------------------------------------------------
def halved(one, two):
    return (one["loss"] * 0.5 == two["loss"] and np.array_equal(np.asarray(one["terms"]) * 0.5, np.asarray(two["terms"]))
            and np.array_equal(one["grad"] * 0.5, two["grad"]) and np.array_equal(one["f"], two["f"]) and np.array_equal(one["r"], two["r"]))


@pytest.mark.parametrize("i,dtype,path", CONFIGS, ids=CONFIG_IDS)
def test_totals_equal_to_the_counts_and_doubled_totals(i, dtype, path):
    case, world = device_case(i)
    x, tot = sh.full_inputs(case)
    full = run(case, 1, 0, dtype, path)
    eng = fz.new_engine(case, dtype, path)
    apply_block(eng, case, x, None)                                          # the calls without n_total
    plain = fz.evaluate(eng, case)
    eng.close()
    assert fz.same_bits(plain, full)
    twice = {k: 2 for k in sh.TOTALS}
    assert halved(full, run(case, 1, 0, dtype, path, twice)), "the full set"
    rank = 1 if not sh.is_empty(sh.block(case, world, 1)[0]) else 0
    one = run(case, world, rank, dtype, path)
    assert halved(one, run(case, world, rank, dtype, path, twice)), "rank %d of %d" % (rank, world)
    tiny = float(np.finfo(ge.DTYPES[dtype]).tiny)
    for got in (full, one):                                                  # not vacuous: no denormal, something to halve
        g = np.abs(got["grad"])
        assert not np.any((g > 0) & (g < 2 * tiny)) and np.any(g > 0) and got["loss"] > 0


SINGLE = [(i, d, p) for i, d, p in CONFIGS if not HOST[i][0]["plan"]]


@pytest.mark.parametrize("i,dtype,path", SINGLE, ids=[CONFIG_IDS[CONFIGS.index(k)] for k in SINGLE])
def test_one_total_doubled_halves_that_term_alone(i, dtype, path):
    case, world = device_case(i)
    rank = 1 if not sh.is_empty(sh.block(case, world, 1)[0]) else 0
    x, _ = sh.block(case, world, rank)
    loc = sh.local(case, x)
    one = run(case, world, rank, dtype, path)
    term_of = {"n_f_total": 0, "n_u_total": 1, "n_b_total": 2, "n_w_total": 2}
    checked = 0
    for t, j in term_of.items():
        if loc[sh.CLASS_OF_TOTAL[t]] == 0:
            continue
        if j == 2 and loc["n_b"] and loc["n_w"]:
            continue                                                         # terms[2] holds both: the sets with one of them
        two = run(case, world, rank, dtype, path, {t: 2})
        assert one["terms"][j] > 0 and two["terms"][j] == 0.5 * one["terms"][j], t
        assert all(two["terms"][m] == one["terms"][m] for m in range(3) if m != j), t
        assert np.array_equal(one["f"], two["f"]) and np.array_equal(one["r"], two["r"])
        assert not np.array_equal(one["grad"], two["grad"])
        checked += 1
    assert checked >= 1


def test_the_single_total_identity_sees_every_term():
    """terms[2] is checked on a set with pairs only and on a set with Robin points only"""
    cases = [c for c, _ in HOST if not c["plan"]]
    assert any(c["n_b"] and not c["n_w"] for c in cases) and any(c["n_w"] and not c["n_b"] for c in cases)
    assert any(c["n_0"] for c in cases)


# ---- (d) a reused context ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i,dtype,path", WALKS, ids=WALK_IDS)
def test_a_reused_context_walks_the_ranks_the_full_set_and_another_world(i, dtype, path):
    case, world = device_case(i)
    other = 8 if world == 3 else 3
    steps = [(world, r) for r in range(world)] + [(1, 0)] + [(other, r) for r in range(other)] + [(1, 0)]
    steps = [(w, r) for w, r in steps if not sh.is_empty(sh.block(case, w, r)[0])]
    eng = fz.new_engine(case, dtype, path)
    differ = []
    for step, (w, r) in enumerate(steps):
        x, tot = sh.block(case, w, r)
        loc = sh.local(case, x)
        apply_block(eng, case, x, tot)
        got, want = fz.evaluate(eng, loc), run(case, w, r, dtype, path)
        if not fz.same_bits(got, want):
            differ.append((step, w, r, [q for q in ("loss", "grad", "terms", "f", "r") if not np.array_equal(got[q], want[q])]))
        if step + 1 < len(steps):
            fz.dirty(eng, loc, step, lhs=case["kind"] != "adr_pw")
    assert not differ, differ
    # the full set is assembled and clean: the same rows with another total must take effect
    x, tot = sh.full_inputs(case)
    if case["n_f"]:
        eng.set_collocation(x["X_f"], n_total=2 * tot["n_f_total"])
        attach(eng, case, x)
        assert fz.same_bits(fz.evaluate(eng, case), run(case, 1, 0, dtype, path, {"n_f_total": 2}))
    if case["n_w"]:
        eng.set_robin(*x["robin"], n_total=2 * tot["n_w_total"])
        scale = {"n_w_total": 2, "n_f_total": 2} if case["n_f"] else {"n_w_total": 2}
        assert fz.same_bits(fz.evaluate(eng, case), run(case, 1, 0, dtype, path, scale))
    eng.close()


# ---- (e) SA-PINN: float64 Burgers, path 7 -------------------------------------------------------------------------------------------
SA_LAYERS, SA_NU, SA_NF, SA_NU_PTS = [2] + [20] * 6 + [1], 0.01 / np.pi, 333, 41


def _sa_inputs():
    rs = np.random.RandomState(4242)
    w, sets = ge.make_case("burgers", SA_LAYERS, SA_NF, SA_NU_PTS, 0, None, rs)
    return w, sets["X_f"], sets["X_u"], sets["u"], rs.uniform(0.5, 2.0, SA_NU_PTS), rs.uniform(0.5, 2.0, SA_NF)


def _sa_engine(w, X_f, X_u, u, lam_u, lam_f, nf_total, nu_total):
    import pinn_native
    eng = pinn_native.Engine(SA_LAYERS, ge.LB, ge.UB, pde="burgers", dtype="f64")
    assert eng.kernel_path() == 7
    eng.set_collocation(X_f, n_total=nf_total)
    eng.set_data(X_u, u, n_total=nu_total)
    eng.set_pde_params(SA_NU)
    eng.set_weights(w)
    eng.sa_set_weights(lam_u, lam_f)
    return eng


def _sa_eval(*a):
    eng = _sa_engine(*a)
    loss, grad, terms = eng.loss_grad()
    eng.close()
    return {"loss": loss, "grad": grad, "terms": tuple(terms)}


def test_sa_weights_doubled_totals_halve_and_blocks_add_up(record):
    w, X_f, X_u, u, lam_u, lam_f = _sa_inputs()
    full = _sa_eval(w, X_f, X_u, u, lam_u, lam_f, SA_NF, SA_NU_PTS)
    two = _sa_eval(w, X_f, X_u, u, lam_u, lam_f, 2 * SA_NF, 2 * SA_NU_PTS)
    assert two["loss"] == 0.5 * full["loss"] and np.array_equal(np.asarray(two["terms"]), 0.5 * np.asarray(full["terms"]))
    assert np.array_equal(two["grad"], 0.5 * full["grad"]) and full["loss"] > 0
    parts = []
    for r in range(3):
        (f0, f1), (u0, u1) = sh.shard_bounds(SA_NF, 3, r), sh.shard_bounds(SA_NU_PTS, 3, r)
        parts.append(_sa_eval(w, X_f[f0:f1], X_u[u0:u1], u[u0:u1], lam_u[u0:u1], lam_f[f0:f1], SA_NF, SA_NU_PTS))
    # as (b) for point weights: every side within the bounds of tests/test_gpu_sa.py of its restatement (loss 1e-12 of the
    # loss, gradient 1e-11 of its largest entry), so the sum within the sum of those
    s = sh.summed(parts)
    dev_l = abs(float(s["loss"]) - full["loss"]) / (sum(p["loss"] for p in parts) + full["loss"])
    dev_g = float(np.max(np.abs(np.asarray(s["grad"], dtype=np.float64) - full["grad"]))
                  / (sum(np.max(np.abs(p["grad"])) for p in parts) + np.max(np.abs(full["grad"]))))
    record(tag="sa-add-up", loss_dev=dev_l, grad_dev=dev_g)
    assert dev_l <= 1e-12 and dev_g <= 1e-11


SA_RATE, SA_EPS, SA_B1, SA_B2 = 0.05, 1.0, 0.9, 0.999


def sa_first_step(lam, r2, N, rate=SA_RATE, b1=SA_B1, b2=SA_B2, eps=SA_EPS):
    """include/pinn_hip.h: lam += alpha_1 m^ / (sqrt(v^) + eps) from zero moments, dL/dlam = 2 lam r^2 / N, in longdouble"""
    ld = np.longdouble
    lam, r2 = np.asarray(lam, dtype=ld), np.asarray(r2, dtype=ld)
    g = ld(2) * lam * r2 / ld(N)
    m, v = (ld(1) - ld(b1)) * g, (ld(1) - ld(b2)) * g * g
    alpha = ld(rate) * np.sqrt(ld(1) - ld(b2)) / (ld(1) - ld(b1))
    return lam + alpha * m / (np.sqrt(v) + ld(eps))


def test_sa_ascent_divides_by_the_total(record):
    """one Adam step with an ascent rate and n_total = 2 n.  Adam's normalisation m / (sqrt(v) + eps) hides the denominator
    unless eps counts: with eps = 1 against sqrt(v) = sqrt(1 - b2) |g| <= 1e-3 the step is proportional to g, so N = n and
    N = n_total give steps a factor 2 apart.  The device's weights must lie within 1e-3 of that gap (plus the rounding of the
    final sum, 2 u of lam) of the formula with N = n_total: a factor 1000 between what is told apart and what is allowed."""
    w, X_f, X_u, u, lam_u, lam_f = _sa_inputs()
    eng = _sa_engine(w, X_f, X_u, u, lam_u, lam_f, 2 * SA_NF, 2 * SA_NU_PTS)
    f = eng.residual().ravel()
    d = (eng.predict(X_u) - u).ravel()
    eng.adam_init(1e-3, SA_B1, SA_B2, SA_EPS)
    eng.sa_adam_init(SA_RATE)
    eng.adam_run(1)
    got_u, got_f = eng.sa_get_weights()
    eng.close()
    u64 = ge.unit_roundoff(np.float64)
    for name, lam, r, n, got in (("f", lam_f, f, SA_NF, got_f), ("u", lam_u, d, SA_NU_PTS, got_u)):
        right, wrong = sa_first_step(lam, r * r, 2 * n), sa_first_step(lam, r * r, n)
        gap = np.asarray(np.abs(right - wrong), dtype=np.float64)
        off = np.asarray(np.abs(np.asarray(got, dtype=np.longdouble) - right), dtype=np.float64)
        sep_u = float(np.median(gap / (u64 * np.abs(lam))))
        print("lam_%s: N = n and N = n_total are %.3g u apart (median; smallest %.3g u), the device is off by at most %.3g u" % (
            name, sep_u, float(np.min(gap / (u64 * np.abs(lam)))), float(np.max(off / (u64 * np.abs(lam))))))
        record(tag="sa-lambda", cls=name, separation_u_median=sep_u, device_off_u_max=float(np.max(off / (u64 * np.abs(lam)))))
        assert sep_u > 100 and np.mean(gap > 100 * u64 * np.abs(lam)) > 0.9      # the two denominators are told apart
        assert np.all(off <= 1e-3 * gap + 2 * u64 * np.abs(lam))
        assert np.all(got > lam - 2 * u64 * np.abs(lam)) and np.any(got > lam)   # ascent


# ---- (f) ensembles ------------------------------------------------------------------------------------------------------------------
def _solo_adr(case, x, tot):
    eng = fz.new_engine(case, "f64", 7)
    apply_block(eng, case, x, tot)
    out = eng.loss_grad()
    eng.close()
    return out


@pytest.mark.parametrize("shared", [True, False], ids=["shared-sets", "per-member-sets"])
@pytest.mark.parametrize("mode", ["doubled", "ragged"])
def test_adr_ensemble_members_with_totals_equal_solo(mode, shared):
    from pinn_native import AdrEnsemble
    members = af.ensemble_members(2)                                         # (n_b, n_0, N_f) = (9, 61, 65)
    K = len(members)
    own = lambda c: af.make_inputs(c)      # noqa: E731
    xs = [own(members[0] if shared else c) for c in members]
    ws = [own(c)["w"] for c in members]
    if mode == "ragged":                                                     # rank 1 of 4: 2 of 9 pairs, 15 of 61, 16 of 65
        blocks = [sh.shard_inputs(members[0], 4, 1, x)[0] for x in xs]
        tot = sh.totals_of(members[0])
    else:
        blocks = [sh.shard_inputs(members[0], 1, 0, x)[0] for x in xs]
        tot = {k: 2 * v for k, v in sh.totals_of(members[0]).items()}
    ens = AdrEnsemble(members[0]["layers"], af.LB, af.UB, K)
    st = (lambda k: blocks[0][k]) if shared else (lambda k: np.stack([b[k] for b in blocks]))
    ens.set_collocation(st("X_f"), n_total=tot["n_f_total"])
    ens.set_data(st("X_u"), st("u"), n_total=tot["n_u_total"])
    ens.set_boundary(st("X_lo"), st("X_hi"), n_total=tot["n_b_total"])
    ens.set_pde_params(np.asarray([c["coeffs"] for c in members]))
    ens.set_weights(np.stack(ws))
    losses, grads, terms = ens.loss_grad()
    ens.close()
    for k, c in enumerate(members):
        l, g, t = _solo_adr(c, dict(blocks[k], w=ws[k]), tot)
        assert losses[k] == l and np.array_equal(grads[k], g) and np.array_equal(terms[k], t), k
        assert t[2] > 0 and t[1] > 0
    if mode == "doubled":                                                    # and the totals did count
        l1, g1, t1 = _solo_adr(members[0], dict(blocks[0], w=ws[0]), sh.totals_of(members[0]))
        assert losses[0] == 0.5 * l1 and np.array_equal(grads[0], 0.5 * g1) and np.array_equal(terms[0], 0.5 * t1)


@pytest.mark.parametrize("shared", [True, False], ids=["shared-sets", "per-member-sets"])
@pytest.mark.parametrize("mode", ["doubled", "ragged"])
def test_burgers_ensemble_members_with_totals_equal_solo(mode, shared):
    from pinn_native import Engine, Ensemble
    K, layers, n_f, n_u = 3, [2] + [20] * 4 + [1], 130, 23
    draws = [ge.make_case("burgers", layers, n_f, n_u, 0, None, np.random.RandomState(5100 + k)) for k in range(K)]
    sets = [draws[0][1] if shared else s for _, s in draws]
    if mode == "ragged":                                                     # rank 2 of 3: 43 of 130, 7 of 23
        (f0, f1), (u0, u1) = sh.shard_bounds(n_f, 3, 2), sh.shard_bounds(n_u, 3, 2)
        nf_t, nu_t = n_f, n_u
    else:
        (f0, f1), (u0, u1), nf_t, nu_t = (0, n_f), (0, n_u), 2 * n_f, 2 * n_u
    cut = [(s["X_f"][f0:f1], s["X_u"][u0:u1], s["u"][u0:u1]) for s in sets]
    ens = Ensemble(layers, ge.LB, ge.UB, K)
    st = (lambda j: cut[0][j]) if shared else (lambda j: np.stack([c[j] for c in cut]))
    ens.set_collocation(st(0), n_total=nf_t)
    ens.set_data(st(1), st(2), n_total=nu_t)
    ens.set_pde_params(ge.NU)
    ens.set_weights(np.stack([w for w, _ in draws]))
    losses, grads, terms = ens.loss_grad()
    ens.close()
    for k in range(K):
        eng = Engine(layers, ge.LB, ge.UB, pde="burgers", dtype="f64")
        eng.set_collocation(cut[k][0], n_total=nf_t)
        eng.set_data(cut[k][1], cut[k][2], n_total=nu_t)
        eng.set_pde_params(ge.NU)
        eng.set_weights(draws[k][0])
        l, g, t = eng.loss_grad()
        if mode == "doubled" and k == 0:
            eng.set_collocation(cut[k][0])
            eng.set_data(cut[k][1], cut[k][2])
            l1, g1, _ = eng.loss_grad()
            assert l == 0.5 * l1 and np.array_equal(g, 0.5 * g1)
        eng.close()
        assert losses[k] == l and np.array_equal(grads[k], g) and np.array_equal(terms[k], t), k
