"""CPU: the fuzz cases of the adr family (tests/helpers/adr_fuzz.py) are what tests/test_gpu_adr_fuzz.py takes them for.

  * pins: restate(., float64) against adr_var_ref.var_loss_grad on every adr case -- f, r, mse_f and mse_w bit for bit (the
    statements are literally the same), loss and gradient to 1e-13 (adr_var_ref takes the data term through
    oracle.mlp.forward_value, which scales the input as 2 (X - lb) / (ub - lb), not as s (X - lb)) -- and against torch
    autograd in float64 on three cases at the bounds of tests/test_adr_var_host.py (loss 1e-14, gradient and f 1e-13);
  * admission: the search reproduces adr_fuzz.SEEDS, every admitted case meets its conditions;
  * non-vacuity: every mutant of every case stands 10 x above the gradient's entrywise bound in every dtype the case runs in;
  * the refusal shares stay within the caps (below).

The caps.  The rule the fuzz was specified with -- every yardstick at most 256 u, a gained net in the tail of tanh -- refuses
5 of the 50 draws the search makes (ungained 1 of 36, gain0 0 of 3, gain 4 of 11).  Admission here also asks, as
grad_entries' does, that every mutant stand 10 x above the bound; that refuses 6 draws more (ungained 3, gain 3), all in float32
and all on a wall class (a Robin point or a pair dropped): where |u_xx| is in the hundreds (the nets of the gain class; large
drawn coefficients) the collocation term is 1e4 x the wall terms, and one wall point of 30 is below float32 rounding of an
entry's scale (the same mutants are > 1e7 x the float64 bound).  Over ten seeds of each gained spec the two rules refuse 33 %
and 30 % of the gain draws.  Each rule is held to the caps on its own (1/3 overall, 1/2 per class), and no search may give up;
together they refuse 7 of the 11 gain draws of this record, which one cap over both rules would not allow: a single-point wall
mutant and a 256 u yardstick cannot both be had on more than 4 in 10 float32 draws of that class.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import adr_fuzz as af  # noqa: E402
import adr_var_ref  # noqa: E402
import grad_entries as ge  # noqa: E402

CASES = af.cases()
ADR = [c for c in CASES if c["kind"] == "adr"]
IDS = lambda cs: [c["id"] for c in cs]      # noqa: E731
need_longdouble = pytest.mark.skipif(not ge.longdouble_is_wider(), reason="np.longdouble is no wider than float64 here")


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300)) if np.size(b) else 0.0


# ---- the case list ------------------------------------------------------------------------------------------------------------
def test_the_cases_are_the_specified_ones():
    assert 36 <= len(CASES) <= 44 and len(set(IDS(CASES))) == len(CASES)
    assert all(af.n_points(c) <= af.MAX_POINTS for c in CASES)
    counts = [(c["n_b"], c["n_0"], c["n_f"], c["n_w"]) for c in CASES]
    assert counts[:6] == [(0, 0, 1, 0), (1, 1, 1, 1), (3, 5, 17, 9), (0, 0, 63, 1), (0, 0, 64, 1), (2, 30, 0, 5)]
    plan = [c for c in CASES if c["plan"]]
    assert len(plan) == 8 and [c["source"] and c["fields"] for c in plan] == [False] * 4 + [True] * 4
    n_cu = af.HOST_N_CU
    for c, (tiles, n_w) in zip(plan, [(n_cu, 20), (n_cu + 1, 40), (n_cu, 30), (n_cu + 1, 1)] * 2):
        assert (af.n_tiles(c), c["n_w"]) == (tiles, n_w) and c["paths"]["f64"] == (0, 7)
        assert af.plan_of(c, n_cu) == ("one-tile" if tiles == n_cu else "tile-loop")
        # the collocation block alone fits one tile per compute unit: the Robin points decide
        assert (af.n_points(c) - c["n_w"] + 63) // 64 <= n_cu
    assert af.n_points(plan[2]) == 64 * n_cu and af.n_points(plan[3]) == 64 * n_cu + 1
    rnd = [c for c in CASES if c["id"].startswith("rnd-")]
    assert {c["cls"] for c in rnd} == set(af.CLASSES) and 3 * sum(c["cls"] != "ungained" for c in rnd) >= len(rnd) - 4
    assert {c["kind"] for c in rnd} == {"adr", "adr_ide", "adr_pw"}
    assert {(len(c["layers"]) - 2) for c in rnd if c["layers"][1] == 20 and c["kind"] == "adr"} == {4, 6, 8}
    assert {c["layers"][1] for c in rnd} == {1, 7, 20, 33}
    nus = [c["coeffs"][2] for c in CASES if c["kind"] == "adr"]
    assert 0.0 in nus and -0.05 in nus and 1e-4 in nus                       # nu = 0, a negative nu, a small one
    assert any(sum(v == 0.0 for v in c["coeffs"]) >= 3 for c in CASES)      # several zero columns at once
    for feat in ("source", "fields"):
        assert any(c[feat] for c in rnd) and any(not c[feat] for c in rnd)
    assert af.cases() is CASES                                               # deterministic, computed once


# ---- pins ---------------------------------------------------------------------------------------------------------------------
WITH_F = [c for c in ADR if c["n_f"]]       # adr_var_ref divides by N_f; the case without collocation points has the next test


@pytest.mark.parametrize("case", WITH_F, ids=IDS(WITH_F))
def test_float64_restatement_is_adr_var_ref(case):
    x = af.inputs(case["id"])
    mine = af.restate(case, np.float64)
    K = x["K"] if x["K"] is not None else adr_var_ref.constant_rows(case["coeffs"], case["n_f"])
    lo, go, ex = adr_var_ref.var_loss_grad(x["w"], case["layers"], af.LB, af.UB, x["X_f"], x["X_u"], x["u"], x["X_lo"], x["X_hi"],
                                           K, x["s"], *(x["robin"] or ()))
    assert np.array_equal(mine["f"], ex["f"]) and mine["terms"][0] == ex["mse_f"]
    assert np.array_equal(mine["r"], ex["r"]) and mine["mse_w"] == ex["mse_w"] and mine["mse_b"] == ex["mse_b"]
    assert abs(mine["loss"] - lo) <= 1e-13 * abs(lo)
    assert abs(mine["terms"][1] - ex["mse_u"]) <= 1e-13 * abs(lo)
    assert rel(mine["grad"], go) <= 1e-13
    assert np.all(mine["A"] >= np.abs(mine["grad"]) * (1 - 1e-12))           # the scale dominates the entry
    assert mine["f"].shape == (case["n_f"], 1) and mine["r"].shape == (case["n_w"],)
    assert np.all(mine["A_f"] >= np.abs(mine["f"]) * (1 - 1e-12)) and np.all(mine["A_r"] >= np.abs(mine["r"]) * (1 - 1e-12))


def test_a_set_without_collocation_points_has_no_residual_term():
    case = next(c for c in CASES if c["n_f"] == 0)
    x = af.inputs(case["id"])
    got = af.restate(case, np.float64)
    want = af.restate_adr(case["layers"], x["w"], case["coeffs"], x["X_f"], x["X_u"], x["u"], x["X_lo"], x["X_hi"], None)
    assert got["terms"][0] == 0.0 and got["f"].shape == (0, 1) and got["terms"][1] > 0 and got["mse_w"] > 0
    assert got["terms"][1] == want["terms"][1] and got["mse_b"] == want["mse_b"] == want["terms"][2]


def test_restatement_takes_no_wider_type_on_the_way():
    case = next(c for c in CASES if c["source"] and c["fields"] and c["n_w"] and c["n_b"] and c["n_0"])
    for dt in (np.float32, np.float64, np.longdouble):
        out = af.restate(case, dt)
        for k in ("loss", "grad", "f", "r"):
            assert np.asarray(out[k]).dtype == np.dtype(dt), (k, dt)
        assert all(np.asarray(t).dtype == np.dtype(dt) for t in out["terms"])
        assert out["A"].dtype == out["A_f"].dtype == out["A_r"].dtype == np.float64


def _torch_loss_grad(case, x):
    import torch
    torch.set_num_threads(4)
    layers = case["layers"]
    wt = torch.tensor(x["w"], dtype=torch.float64, requires_grad=True)
    lb, ub = torch.tensor(af.LB), torch.tensor(af.UB)

    def channels(X):
        xx = torch.tensor(np.ascontiguousarray(X[:, 0:1]), requires_grad=True)
        tt = torch.tensor(np.ascontiguousarray(X[:, 1:2]), requires_grad=True)
        h = 2.0 * (torch.cat([xx, tt], dim=1) - lb) / (ub - lb) - 1.0
        off = 0
        for i, (fi, fo) in enumerate(zip(layers[:-1], layers[1:])):
            h = h @ wt[off:off + fi * fo].reshape(fi, fo) + wt[off + fi * fo:off + fi * fo + fo]
            off += fi * fo + fo
            if i < len(layers) - 2:
                h = torch.tanh(h)
        ones = torch.ones_like(h)
        u_x, u_t = torch.autograd.grad(h, [xx, tt], ones, create_graph=True)
        u_xx = torch.autograd.grad(u_x, xx, ones, create_graph=True)[0]
        return h, u_x, u_t, u_xx

    col = lambda v: torch.tensor(np.asarray(v, dtype=np.float64).reshape(-1, 1))      # noqa: E731
    K = x["K"] if x["K"] is not None else adr_var_ref.constant_rows(case["coeffs"], case["n_f"])
    a0, a1, nu, r1, r2, r3 = (col(K[:, j]) for j in range(6))
    uu, u_x, u_t, u_xx = channels(x["X_f"])
    f = u_t + (a0 + a1 * uu) * u_x - nu * u_xx + r1 * uu + r2 * uu ** 2 + r3 * uu ** 3
    if x["s"] is not None:
        f = f - col(x["s"])
    loss = torch.mean(f ** 2)
    if case["n_0"]:
        loss = loss + torch.mean((channels(x["X_u"])[0] - torch.tensor(np.asarray(x["u"]))) ** 2)
    if case["n_b"]:
        ul, ul_x, _, _ = channels(x["X_lo"])
        uh, uh_x, _, _ = channels(x["X_hi"])
        loss = loss + torch.mean((ul - uh) ** 2) + torch.mean((ul_x - uh_x) ** 2)
    r = None
    if case["n_w"]:
        X_w, al, be, g = x["robin"]
        uw, uw_x, _, _ = channels(X_w)
        r = col(al) * uw + col(be) * uw_x - col(g)
        loss = loss + torch.mean(r ** 2)
    loss.backward()
    return float(loss.detach()), wt.grad.numpy().copy(), f.detach().numpy(), None if r is None else r.detach().numpy().ravel()


AUTOGRAD = ["edge-adr-6x20-b3-u5-f17-w9-src-var-s11200", "rnd-adr-6x20-b27-u109-f147-w53-var-s12800",
            "rnd-adr-8x20-b26-u119-f547-w18-src-var-s13500"]


@pytest.mark.parametrize("cid", AUTOGRAD)
def test_restatement_against_torch_autograd(cid):
    case = af.CASE_BY_ID[cid]
    x = af.inputs(cid)
    mine = af.restate(case, np.float64)
    lt, gt, ft, rt = _torch_loss_grad(case, x)
    print("%s: loss %.2e grad %.2e f %.2e r %.2e" % (cid, abs(mine["loss"] - lt) / abs(lt), rel(mine["grad"], gt),
                                                     rel(mine["f"], ft), rel(mine["r"], rt)))
    assert abs(mine["loss"] - lt) / abs(lt) < 1e-14
    assert rel(mine["grad"], gt) < 1e-13
    assert rel(mine["f"], ft) < 1e-13 and rel(mine["r"], rt) < 1e-13


# ---- admission ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def searches():
    """{base id: (seed, refused)} of every spec: the search, run once"""
    return {c["id"]: af.first_admitted_seed(c["id"]) for c in af.specs()}


@need_longdouble
def test_the_search_reproduces_the_recorded_seeds(searches):
    found = {base: seed for base, (seed, _) in searches.items()}
    base_seed = {c["id"]: c["seed"] for c in af.specs()}
    moved = {b: s for b, s in found.items() if s != base_seed[b]}
    assert moved == af.SEEDS, "the search finds %s" % moved
    for c in CASES:
        seed, refused = searches[c["base_id"]]
        assert c["seed"] == seed and c["id"] == "%s-s%d" % (c["base_id"], seed)
        assert [s for s, _ in refused] == list(range(base_seed[c["base_id"]], seed)) and all(why for _, why in refused)
    listed = {k for k in af.CASE_BY_ID if not k.endswith("-bare") and not k.startswith("ens")}       # (walk's twins, ensemble members)
    assert listed == set(IDS(CASES))                                      # the refused candidates are gone again


@need_longdouble
@pytest.mark.parametrize("case", CASES, ids=IDS(CASES))
def test_admitted_case_meets_its_conditions(case):
    cid = case["id"]
    assert af.refusal(cid) is None
    if case["kind"] == "adr_pw":
        return
    for d in af.dtypes_judged(case):
        u = ge.unit_roundoff(ge.DTYPES[d])
        y = af.yardsticks(cid, d)
        print("%s %s: yardsticks %s u" % (cid, d, {q: round(v / u) for q, v in y.items()}))
        assert set(y) == set(af.QUANTITIES)
        assert all(ge.FLOOR_ULPS * u <= v <= ge.SAT_YARDSTICK_ULPS * u == 256 * u for v in y.values())
        if case["cls"] != "ungained":
            zmax, share = af.preactivation_stats(cid, d)
            assert zmax >= ge.SAT_MAX_Z == 5.0 and share >= ge.SAT_TAIL_SHARE == 0.01
    # the gains reached the weights: the draws are those of the ungained net
    w = af.inputs(cid)["w"]
    w0 = af.make_inputs(dict(case, gain=None, gain0=None))["w"]
    W, nn = case["layers"][1], af.adr_ide_ref.n_net(case["layers"])
    g_first, g_rest = (case["gain0"] or 1.0) * (case["gain"] or 1.0), case["gain"] or 1.0
    assert np.array_equal(w[:3 * W], g_first * w0[:3 * W]) and np.array_equal(w[3 * W:nn], g_rest * w0[3 * W:nn])


# ---- non-vacuity ----------------------------------------------------------------------------------------------------------------
WANTED = {"colloc": lambda c: c["n_f"] > af.lost_unit(c), "robin": lambda c: c["n_w"] >= 2, "swap": lambda c: c["n_w"] >= 1,
          "pair": lambda c: c["n_b"] >= 2, "row": lambda c: c["fields"] and c["n_f"] > af.lost_unit(c),
          "shift": lambda c: c["fields"] and c["n_f"] > af.lost_unit(c), "source": lambda c: c["source"]}


@need_longdouble
@pytest.mark.parametrize("case", [c for c in CASES if c["kind"] != "adr_pw"], ids=IDS([c for c in CASES if c["kind"] != "adr_pw"]))
def test_every_mutant_is_ten_times_above_the_bound(case):
    """each mutant on every case that has the element it needs, in every dtype the case runs in, against the largest bound of
    the case's paths"""
    found = af.mutants(case)
    if case["kind"] == "adr_ide":
        assert set(found) == {"colloc", "tail"}
    else:
        assert set(found) == {k for k, need in WANTED.items() if need(case)}
    for d in af.dtypes_judged(case):
        margins = af.mutant_margins(case["id"], d)
        print("%s %s: %s" % (case["id"], d, {k: "%.3g" % v for k, v in sorted(margins.items())}))
        assert set(margins) == set(found)
        for name, ratio in margins.items():
            assert ratio >= ge.SAT_MUTANT_MARGIN == 10.0, "%s mutant %s is %.2f x the bound %.3e" % (
                d, name, ratio, af.bound(case["id"], d))


def test_every_mutant_runs_somewhere():
    names = set()
    for c in CASES:
        if c["kind"] == "adr":
            names |= {k for k, need in WANTED.items() if need(c)}
    assert names == set(WANTED) and any(c["kind"] == "adr_ide" for c in CASES)


# ---- the caps -------------------------------------------------------------------------------------------------------------------
@need_longdouble
def test_refusal_shares_stay_within_the_caps(searches):
    """per rule (module docstring): the specified rule (yardsticks, the tail of tanh) and the mutant margin, each at most 1/3
    of the draws overall and 1/2 within a class"""
    cls_of = {c["id"]: c["cls"] for c in af.specs()}
    tried = {k: 0 for k in af.CLASSES}
    refused = {rule: {k: 0 for k in af.CLASSES} for rule in ("specified", "mutant")}
    for base, (seed, ref) in searches.items():
        tried[cls_of[base]] += len(ref) + 1
        for _, why in ref:
            refused["mutant" if "mutant" in why else "specified"][cls_of[base]] += 1
    print("draws %s refused %s" % (tried, refused))
    for rule, by in refused.items():
        assert 3 * sum(by.values()) <= sum(tried.values()), (rule, by, tried)
        for k in af.CLASSES:
            assert tried[k] > 0 and 2 * by[k] <= tried[k], (rule, k, by[k], tried[k])
    for k in af.CLASSES:                                                     # no class is emptied
        assert sum(1 for c in CASES if c["cls"] == k) == sum(1 for c in af.specs() if c["cls"] == k) > 0


# ---- the walk of the reused contexts --------------------------------------------------------------------------------------------
def test_the_walk_shrinks_grows_crosses_the_plan_boundary_and_toggles_every_feature():
    groups = af.config_groups(CASES)
    assert len(groups) == 30 and sum(len(g) for g in groups.values()) == sum(len(p) for c in CASES for p in c["paths"].values())
    n_cu = af.HOST_N_CU
    for (kind, layers, dtype, path), group in groups.items():
        order = af.walk(group)
        assert {c["id"].replace("-bare", "") for c in order} == {c["id"] for c in group} and len(order) >= 2
        tiles = [af.n_tiles(c) for c in order]
        if kind == "adr" and layers[1] == 20:
            assert sum(a <= n_cu < b for a, b in zip(tiles[:-1], tiles[1:])) >= 1      # into the tile loop
            assert sum(b <= n_cu < a for a, b in zip(tiles[:-1], tiles[1:])) >= 1      # and back
            assert any(a > b for a, b in zip(tiles[:-1], tiles[1:])) and any(a < b for a, b in zip(tiles[:-1], tiles[1:]))
            for name in ("robin", "source", "fields"):
                assert af.on_off_on(order, af.FEATURES[name]), (kind, layers, dtype, path, name)
            # the bare twin shares its case's draws: the source and the fields are removed and replaced in place
            full, twin = order[-1], order[-2]
            assert twin["id"] == full["id"] + "-bare" and order[-3] is full
            a, b = af.inputs(full["id"]), af.inputs(twin["id"])
            assert all(np.array_equal(a[k], b[k]) for k in ("w", "X_f", "X_u", "u", "X_lo", "X_hi"))
            assert b["robin"] is None and b["s"] is None and b["K"] is None
    ide = [k for k in groups if k[0] == "adr_ide"]
    assert len(ide) == 9 and {k[3] for k in ide} == {0, 7}
