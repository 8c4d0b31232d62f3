"""CPU: the shards of the adr family's fuzz cases (tests/helpers/adr_shards.py) are what tests/test_gpu_adr_shards.py takes them
for, and the comparator of that file rejects a wrong sharding.

  * partition: the blocks of every class partition it exactly, pairs stay together, source and field rows travel with their
    points, Robin scalars are expanded; the named edges of adr_shards.SHARDED are where its docstring says;
  * exact halving: the restatement with all four totals doubled gives loss, terms and gradient that are 0.5 x the undoubled
    ones bit for bit (float64 and float32) -- every denominator enters as one division of a sum or of 2 r by N, and halving is
    exact short of a denormal;
  * additivity: the blocks' restatements with the global totals sum to the full restatement within the sum of their yardsticks
    (allowance 1: plain arithmetic against itself), every entry on the scale A and the loss and its terms on the loss;
  * mutants: a class divided by its local count (once per class), a pair slice with lo and hi one row apart, source / field
    rows cut where the data block starts, the last Robin row dropped with the total kept: each leaves the derived bound of
    tests/test_gpu_adr_shards.py (both sides' K x yardstick, at the largest K of the case's paths) by SAT_MUTANT_MARGIN = 10 x
    or more, in every dtype the case runs in.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import adr_fuzz as af  # noqa: E402
import adr_shards as sh  # noqa: E402
import grad_entries as ge  # noqa: E402
from pinn_native.parallel import shard_bounds  # noqa: E402

PAIRS = [(sh.case_of(b), w) for b, w in sh.SHARDED]
IDS = ["%s-over%d" % (c["id"], w) for c, w in PAIRS]
JUDGED = [(c, w) for c, w in PAIRS if c["kind"] != "adr_pw"]
JIDS = ["%s-over%d" % (c["id"], w) for c, w in JUDGED]
need_longdouble = pytest.mark.skipif(not ge.longdouble_is_wider(), reason="np.longdouble is no wider than float64 here")
DT = {"f32": np.float32, "f64": np.float64}


# ---- the list -------------------------------------------------------------------------------------------------------------------
def test_the_list_covers_what_it_is_meant_to():
    cases = [c for c, _ in PAIRS]
    assert {w for _, w in PAIRS} == {3, 8} and len(PAIRS) <= 24
    assert {c["kind"] for c in cases} == {"adr", "adr_ide", "adr_pw"}
    feats = lambda c: (c["n_b"] > 0, c["n_0"] > 0, c["n_w"] > 0, c["source"], c["fields"])      # noqa: E731
    seen = {feats(c) for c in cases if c["kind"] == "adr"}
    assert (True,) * 5 in seen                                               # together
    for alone in range(5):                                                   # and each alone
        assert tuple(i == alone for i in range(5)) in seen, alone
    assert any(c["kind"] == "adr_ide" and bin(c["mask"]).count("1") >= 3 for c in cases)
    assert any(c["layers"][1] != 20 and c["paths"] == {"f64": (0,), "f32": (0,)} for c in cases)      # t16 family, path 0
    assert {"gain0", "gain"} <= {c["cls"] for c in cases}
    plan = [(c, w) for c, w in PAIRS if c["plan"]]
    assert plan and all(w == 3 for _, w in plan)
    for c, w in plan:                                                        # the tile loop whole, one tile per workgroup sharded
        assert af.plan_of(c, af.HOST_N_CU) == "tile-loop"
        for r in range(w):
            x, _ = sh.block(c, w, r)
            assert (af.n_points_of(x) + 63) // 64 <= af.HOST_N_CU
    assert max(af.n_points(c) for c in cases if not c["plan"]) < 3000


def _blocks(base, world):
    c = sh.case_of(base)
    return c, [sh.block(c, world, r)[0] for r in range(world)]


def test_the_named_edges_are_there():
    n = lambda xs, k: [len(x[k]) for x in xs]      # noqa: E731
    c, xs = _blocks("edge-adr-6x20-b3-u5-f17-w9-src-var", 8)
    assert n(xs, "X_lo") == [1, 1, 1, 0, 0, 0, 0, 0] and n(xs, "X_u") == [1] * 5 + [0] * 3 and min(n(xs, "X_f")) == 2
    assert [len(x["robin"][0]) for x in xs] == [2] + [1] * 7
    c, xs = _blocks("shard-robin-adr-4x20-b0-u0-f50-w3", 8)
    assert [len(x["robin"][0]) for x in xs] == [1, 1, 1, 0, 0, 0, 0, 0] and all(x["robin"] is not None for x in xs)
    c, xs = _blocks("shard-data-adr-8x20-b0-u7-f130-w0", 8)
    assert n(xs, "X_u") == [1] * 7 + [0]
    c, xs = _blocks("shard-nof-adr-6x20-b9-u11-f5-w10-src-var", 8)
    assert n(xs, "X_f") == [1] * 5 + [0] * 3 and all(not sh.is_empty(x) for x in xs)
    assert all(x["s"].shape == (len(x["X_f"]),) and x["K"].shape == (len(x["X_f"]), 6) for x in xs)
    c, xs = _blocks("edge-adr-4x20-b1-u1-f1-w1", 3)
    assert [sh.is_empty(x) for x in xs] == [False, True, True]
    c, xs = _blocks("shard-pairs-adr-4x20-b25-u0-f40-w0", 3)
    assert [2 * k for k in n(xs, "X_lo")] == [18, 16, 16]                    # inside a wave; a 16-point boundary
    c, xs = _blocks("shard-pairs64-adr-6x20-b97-u0-f100-w0", 3)
    assert [2 * k for k in n(xs, "X_lo")] == [66, 64, 64]                    # a 64-point boundary
    c, xs = _blocks("shard-tile-adr-6x20-b0-u2-f190-w0", 3)
    assert [af.n_points_of(x) for x in xs] == [65, 64, 63]                   # one point either side of a tile


# ---- partition ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,world", PAIRS, ids=IDS)
def test_the_blocks_partition_every_class(case, world):
    x, tot = sh.full_inputs(case)
    assert tot == {"n_f_total": case["n_f"], "n_u_total": case["n_0"], "n_b_total": case["n_b"], "n_w_total": case["n_w"]}
    blocks = [sh.shard_inputs(case, world, r) for r in range(world)]
    assert all(t == tot for _, t in blocks)
    cat = lambda k: np.concatenate([b[k] for b, _ in blocks])      # noqa: E731
    for k in ("X_f", "X_u", "u", "X_lo", "X_hi") + (("s",) if case["source"] else ()) + (("K",) if case["fields"] else ()):
        assert np.array_equal(cat(k), x[k]), k
    for r, (b, _) in enumerate(blocks):
        lo, hi = shard_bounds(case["n_f"], world, r)
        assert len(b["X_f"]) == hi - lo and np.array_equal(b["w"], x["w"])
        assert (b["s"] is None) == (not case["source"]) and (b["K"] is None) == (not case["fields"])
        if case["source"]:
            assert np.array_equal(b["s"], af.cells.source_of(b["X_f"]))        # the rows of the block's own points
        if case["fields"]:
            assert np.array_equal(b["K"], af.fields_of(b["X_f"], case["coeffs"]))
        assert len(b["X_lo"]) == len(b["X_hi"]) and np.array_equal(b["X_lo"][:, 1], b["X_hi"][:, 1])      # pairs stay pairs
        assert len(b["X_u"]) == len(b["u"])
        sizes = [len(b["X_f"]), len(b["X_u"]), len(b["X_lo"])]
        assert all(0 <= case[k] // world <= s <= -(-case[k] // world) for s, k in zip(sizes, ("n_f", "n_0", "n_b")))
    if case["n_w"]:
        for j in range(4):
            assert np.array_equal(np.concatenate([b["robin"][j] for b, _ in blocks]), x["robin"][j])
        assert all(len({len(a) for a in b["robin"]}) == 1 for b, _ in blocks)
    else:
        assert all(b["robin"] is None for b, _ in blocks)
    if case["kind"] == "adr_pw":
        for j, k in enumerate(("X_u", "X_f", "X_lo")):
            assert np.array_equal(np.concatenate([b["lam"][j] for b, _ in blocks]), x["lam"][j])
            assert all(len(b["lam"][j]) == len(b[k]) for b, _ in blocks)


def test_robin_scalars_are_expanded_before_they_are_cut():
    case = sh.case_of("edge-adr-6x20-b3-u5-f17-w9-src-var")
    x = dict(sh.full_inputs(case)[0])
    x["robin"] = (x["robin"][0], 0.5, -1.25, x["robin"][3])
    for r in range(8):
        b, _ = sh.shard_inputs(case, 8, r, x)
        m = len(b["robin"][0])
        assert np.array_equal(b["robin"][1], np.full(m, 0.5)) and np.array_equal(b["robin"][2], np.full(m, -1.25))


# ---- exact halving ------------------------------------------------------------------------------------------------------------------
def _halves(a, b):
    return (np.asarray(a["loss"]) * 0.5 == b["loss"] and all(np.asarray(s) * 0.5 == t for s, t in zip(a["terms"], b["terms"]))
            and np.array_equal(np.asarray(a["grad"]) * a["grad"].dtype.type(0.5), b["grad"]))


@pytest.mark.parametrize("case,world", PAIRS, ids=IDS)
def test_doubled_totals_halve_the_restatement_exactly(case, world):
    for d in case["paths"]:
        for rank in (0, 1):                                                  # the whole set and a block of it
            x, tot = sh.block(case, world if rank else 1, rank)
            if sh.is_empty(x):
                continue
            one = af.restate(case, DT[d], x, **tot)
            two = af.restate(case, DT[d], x, **{k: 2 * v for k, v in tot.items()})
            assert _halves(one, two), (d, rank)
            tiny = np.finfo(DT[d]).tiny
            g = np.abs(np.asarray(one["grad"], dtype=np.float64))
            assert not np.any((g > 0) & (g < 2 * tiny))                      # no denormal entry: the identity is not vacuous


# ---- additivity -----------------------------------------------------------------------------------------------------------------------
def _parts(case, world, dt):
    out = []
    for r in range(world):
        x, tot = sh.block(case, world, r)
        if not sh.is_empty(x):
            out.append(af.restate(case, dt, x, **tot))
    return out


@need_longdouble
@pytest.mark.parametrize("case,world", JUDGED, ids=JIDS)
def test_block_restatements_add_up_within_their_yardsticks(case, world):
    x, tot = sh.full_inputs(case)
    for d in af.dtypes_judged(case):
        u = ge.unit_roundoff(DT[d])
        full = af.restate(case, DT[d], x, **tot)
        bg, blo = sh.additive_bound(case, world, d, 1.0)
        share_g, share_lo, _ = sh.additive_share(_parts(case, world, DT[d]), full, bg, blo)
        ref = sh.reference(case["id"], 1, 0, d)
        s = sh.summed(_parts(case, world, DT[d]))
        dev_u = af._scaled(np.asarray(s["grad"], dtype=np.float64), np.asarray(full["grad"], dtype=np.float64), ref["A"]) / u
        print("%s over %d %s: gradient %.2f of the bound (%.0f u of A), loss %.2f" % (case["id"], world, d, share_g, dev_u, share_lo))
        assert share_g <= 1.0 and share_lo <= 1.0, (d, share_g, share_lo)


def test_point_weighted_blocks_add_up():
    """adr_pw_ref is float64 only and returns no scale A: whole vectors, at the float64 bounds of tests/test_gpu_adr.py"""
    for case, world in [(c, w) for c, w in PAIRS if c["kind"] == "adr_pw"]:
        x, tot = sh.full_inputs(case)
        full = af.restate(case, np.float64, x, **tot)
        assert full["loss"] == af.restate(case, np.float64)["loss"]          # explicit totals of the whole set change nothing
        s = sh.summed(_parts(case, world, np.float64))
        assert abs(float(s["loss"]) - full["loss"]) <= 1e-13 * full["loss"]
        assert max(abs(float(a) - b) for a, b in zip(s["terms"], full["terms"])) <= 1e-13 * full["loss"]
        assert np.max(np.abs(np.asarray(s["grad"], dtype=np.float64) - full["grad"])) <= 1e-13 * np.max(np.abs(full["grad"]))


# ---- mutants ----------------------------------------------------------------------------------------------------------------------------
MUTATED = [(c, w) for c, w in JUDGED if not c["plan"] and af.n_points(c) >= 20]
WANTED = {"local-f": lambda c: c["n_f"] >= 2, "local-u": lambda c: c["n_0"] >= 2, "local-b": lambda c: c["n_b"] >= 2,
          "local-w": lambda c: c["n_w"] >= 2 and c["kind"] == "adr", "pair-shift": lambda c: c["n_b"] >= 2,
          "rows-by-data": lambda c: (c["source"] or c["fields"]) and c["n_0"] > 0 and c["kind"] == "adr",
          "robin-drop": lambda c: c["n_w"] >= 2 and c["kind"] == "adr"}


@need_longdouble
@pytest.mark.parametrize("case,world", MUTATED, ids=["%s-over%d" % (c["id"], w) for c, w in MUTATED])
def test_every_wrong_sharding_is_rejected_with_a_margin(case, world):
    assert set(sh.mutants(case, world)) == {k for k, need in WANTED.items() if need(case)}
    for d in af.dtypes_judged(case):
        margins = sh.mutant_margins(case, world, d)
        print("%s over %d %s: %s" % (case["id"], world, d, {k: "%.3g" % v for k, v in sorted(margins.items())}))
        for name, ratio in margins.items():
            assert ratio >= ge.SAT_MUTANT_MARGIN == 10.0, "%s mutant %s is %.2f x the bound" % (d, name, ratio)


def test_every_mutant_runs_somewhere():
    names = set()
    for c, _ in MUTATED:
        names |= {k for k, need in WANTED.items() if need(c)}
    assert names == set(WANTED)
