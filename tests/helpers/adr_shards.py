"""Shards of the adr family's fuzz cases (test infrastructure, numpy only): what a rank of a data-parallel run holds of a case of
tests/helpers/adr_fuzz.py, and what it has to compute from it.

A rank holds a contiguous block of every point class (pinn_native.parallel.shard_bounds) and divides by the size of the WHOLE
class (the n_total of every pinn_set_* call), so that the ranks' losses and gradients add up to those of the full set.

  shard_inputs(case, world, rank)   -> (inputs, totals): the block of every class -- collocation points with their source values
                                    and coefficient rows, data with its targets, pairs (lo and hi together), Robin rows with
                                    their alpha, beta, g, point weights per class -- and the four denominators
  full_inputs(case)                 -> (inputs, totals) of the whole set (world 1)
  reference, yardsticks             adr_fuzz's, for a block: its own restatement in the wider type (by the block's own point
                                    count) and max(plain error of the block's restatement in the compute dtype, 32 u); cached
  SHARDED                           the fixed list of (case id, world): see the table below
  additive_bound                    what the sum of the ranks' results may differ from the full set's by: the allowed deviation
                                    of every side, K x yardstick on the side's own scale, summed
  mutants(case, world)              wrong shardings a comparator has to reject

SHARDED covers, between its entries: pairs, data, Robin points, source and fields together and each alone; adr_ide with masks
of several coefficients; adr_pw; off-shape nets (path 0); gained nets; worlds 3 and 8; and by name
  b3 over 8, u5 over 8, u7 over 8, w3 over 8, w1 over 3    a class whose local block is empty while its total is not
  shard-nof (f5 over 8)                                    ranks without a collocation block (accepted, terms[0] == 0.0)
  edge b1-u1-f1-w1 over 3                                  ranks 1 and 2 hold no point at all (refused)
  shard-pairs b25 over 3: 9, 8, 8 pairs                    a pair block of 18 points (inside a wave) and of 16
  shard-pairs64 b97 over 3: 33, 32, 32                     a pair block of 66 points and of 64 (a whole tile)
  shard-tile u2-f190 over 3                                blocks of 65, 64 and 63 points: one either side of a tile
  plan-* over 3                                            a full set in the tile loop (more than n_cu tiles) whose blocks take
                                                           one tile per workgroup
"""
import functools
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, _HERE)
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(_HERE)), "pinns-tf2.0_amd"))
import adr_fuzz as af  # noqa: E402
from pinn_native.parallel import shard_bounds  # noqa: E402

TOTALS = ("n_f_total", "n_u_total", "n_b_total", "n_w_total")
CLASS_OF_TOTAL = {"n_f_total": "n_f", "n_u_total": "n_0", "n_b_total": "n_b", "n_w_total": "n_w"}


# ---- cases --------------------------------------------------------------------------------------------------------------------
def _own_cases():
    """cases placed for a sharding edge (no admission, as adr_fuzz.ensemble_members: judged on max(plain error, 32 u) whatever
    that is).  They live here and not in adr_fuzz.CASE_BY_ID, whose content tests/test_adr_fuzz_host.py pins."""
    some = [0.3, -0.8, 0.02, 0.6, -0.4, 1.5]
    L = af.layers_of
    out = [af._spec("shard-pairs", "adr", L(4), 25, 0, 40, 0, 21000, some),
           af._spec("shard-pairs64", "adr", L(6), 97, 0, 100, 0, 21100, some),
           af._spec("shard-data", "adr", L(8), 0, 7, 130, 0, 21200, some),
           af._spec("shard-robin", "adr", L(4), 0, 0, 50, 3, 21300, some),
           af._spec("shard-tile", "adr", L(6), 0, 2, 190, 0, 21400, some),
           af._spec("shard-nof", "adr", L(6), 9, 11, 5, 10, 21500, some, source=True, fields=True),
           af._spec("shard-src", "adr", L(8), 0, 0, 70, 0, 21600, some, source=True),
           af._spec("shard-var", "adr", L(8), 0, 0, 45, 0, 21700, some, fields=True)]
    return {c["id"]: dict(c, base_id=c["id"]) for c in out}


OWN = _own_cases()

# (case id or base id, world)
SHARDED = (
    ("edge-adr-6x20-b3-u5-f17-w9-src-var", 8),                  # every feature; pairs and data blocks empty on the last ranks
    ("edge-adr-4x20-b1-u1-f1-w1", 3),                           # ranks 1, 2: no point at all
    ("edge-adr-4x20-b0-u0-f64-w1-src", 3),                      # the one Robin point is rank 0's
    ("shard-src-adr-8x20-b0-u0-f70-w0-src", 3),                 # source alone
    ("shard-var-adr-8x20-b0-u0-f45-w0-var", 8),                 # fields alone
    ("edge-adr-6x20-b2-u30-f0-w5", 3),                          # no collocation point in the whole set
    ("shard-pairs-adr-4x20-b25-u0-f40-w0", 3),                  # pairs alone
    ("shard-pairs64-adr-6x20-b97-u0-f100-w0", 3),
    ("shard-data-adr-8x20-b0-u7-f130-w0", 8),                   # data alone
    ("shard-robin-adr-4x20-b0-u0-f50-w3", 8),                   # Robin points alone
    ("shard-tile-adr-6x20-b0-u2-f190-w0", 3),
    ("shard-nof-adr-6x20-b9-u11-f5-w10-src-var", 8),
    ("plan-robin-spills-adr-4x20-b3-u50-f16298-w40", 3),        # tile loop -> one tile per workgroup
    ("plan-one-live-lane-adr-4x20-b3-u50-f16328-w1-src-var", 3),
    ("rnd-adr-4x20-b17-u36-f59-w3-src-var-gain0x12", 8),        # gained (first layer x 12); w3 over 8
    ("rnd-adr-4x20-b10-u54-f553-w22-gainx3", 3),                # gained (every layer x 3)
    ("rnd-adr-5x33-b38-u31-f579-w14-src-gain0x12", 3),          # off-shape (t16 family, path 0), gained
    ("rnd-adr-3x7-b39-u81-f517-w78-src-var", 8),                # off-shape
    ("rnd-adr_ide-4x20-b14-u41-f1396-w0-gainx3", 3),            # mask 61: five coefficients trained; gained
    ("rnd-adr_ide-8x20-b23-u17-f449-w0", 8),                    # mask 13: three coefficients
    ("rnd-adr_pw-8x20-b15-u62-f309-w0", 3),
    ("rnd-adr_pw-4x20-b13-u34-f953-w0", 8),
)


def case_of(base_id, n_cu=af.HOST_N_CU):
    """the case of SHARDED by its base id (the plan cases depend on n_cu, and with it their ids)"""
    if base_id in OWN:
        return OWN[base_id]
    if n_cu == af.HOST_N_CU:
        return next(c for c in af.cases(n_cu) if c["base_id"] == base_id)
    host = [c["base_id"] for c in af.cases()]
    return af.cases(n_cu)[host.index(base_id)]        # the same spec on another device: the same place in the list


@functools.lru_cache(maxsize=None)
def _inputs(cid):
    return af.make_inputs(OWN[cid]) if cid in OWN else af.inputs(cid)


def _frozen(x):
    for a in list(x.values()) + list(x["robin"] or ()) + list(x["lam"] or ()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return x


def counts(case, world, rank):
    """-> {class: (lo, hi)} of the rank's block"""
    return {k: shard_bounds(case[k], world, rank) for k in ("n_f", "n_0", "n_b", "n_w")}


def totals_of(case):
    return {t: case[k] for t, k in CLASS_OF_TOTAL.items()}


def shard_inputs(case, world, rank, inp=None):
    """-> (inputs, totals): the rank's block of every class of `case` (inp: other inputs than the case's own), in the form of
    adr_fuzz.make_inputs, and the denominators {n_f_total, n_u_total, n_b_total, n_w_total}.  A case with Robin points keeps the
    class on every rank (a rank without rows: arrays of 0 rows and the total)."""
    x = _inputs(case["id"]) if inp is None else inp
    b = counts(case, world, rank)
    cut = lambda a, k: None if a is None else np.ascontiguousarray(a[b[k][0]:b[k][1]])      # noqa: E731
    out = {"w": x["w"], "X_f": cut(x["X_f"], "n_f"), "s": cut(x["s"], "n_f"), "K": cut(x["K"], "n_f"),
           "X_u": cut(x["X_u"], "n_0"), "u": cut(x["u"], "n_0"),
           "X_lo": cut(x["X_lo"], "n_b"), "X_hi": cut(x["X_hi"], "n_b"), "robin": None, "lam": None}
    if x["robin"] is not None:
        m = len(x["robin"][0])
        cols = [np.broadcast_to(np.asarray(v, dtype=np.float64).reshape(-1), (m,)) for v in x["robin"][1:]]     # scalars expanded
        out["robin"] = tuple(cut(a, "n_w") for a in [x["robin"][0]] + cols)
    if x["lam"] is not None:
        out["lam"] = tuple(cut(a, k) for a, k in zip(x["lam"], ("n_0", "n_f", "n_b")))
    return _frozen(out), totals_of(case)


def full_inputs(case):
    return shard_inputs(case, 1, 0)


def local(case, x):
    """the case with the counts of the block `x` (what a context that holds the block reports)"""
    return dict(case, n_f=len(x["X_f"]), n_0=len(x["X_u"]), n_b=len(x["X_lo"]), n_w=len(x["robin"][0]) if x["robin"] else 0)


def is_empty(x):
    """no training point at all: Robin points alone are no training set"""
    return len(x["X_f"]) + len(x["X_u"]) + len(x["X_lo"]) == 0


# ---- references and yardsticks of a block ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _block(cid, world, rank):
    return shard_inputs(OWN.get(cid) or af.CASE_BY_ID[cid], world, rank)


def block(case, world, rank):
    """shard_inputs, computed once per (case, world, rank); world 1: the whole set with explicit totals"""
    return _block(case["id"], world, rank)


def _case(cid):
    return OWN.get(cid) or af.CASE_BY_ID[cid]


@functools.lru_cache(maxsize=None)
def reference(cid, world, rank, dtype_name):
    x, tot = _block(cid, world, rank)
    return af.reference(_case(cid), dtype_name, x, tot)


@functools.lru_cache(maxsize=None)
def yardsticks(cid, world, rank, dtype_name):
    x, tot = _block(cid, world, rank)
    return af.yardsticks(_case(cid), dtype_name, x, tot, ref=reference(cid, world, rank, dtype_name))


def allowance(case, dtype_name):
    """the largest allowance of the case's paths (what a mutant has to exceed)"""
    return max(af.allowance(case, p, dtype_name) for p in case["paths"][dtype_name])


def additive_bound(case, world, dtype_name, k):
    """-> (bound per gradient entry, bound of the loss and of each term): sum over both sides -- every rank's block and the full
    set -- of k x the side's yardstick x the side's scale (A per entry; the side's loss)"""
    sides = [(r, world) for r in range(world)] + [(0, 1)]
    g, lo = 0.0, 0.0
    for rank, w in sides:
        x, _ = _block(case["id"], w, rank)
        if is_empty(x):
            continue
        ref, y = reference(case["id"], w, rank, dtype_name), yardsticks(case["id"], w, rank, dtype_name)
        g = g + k * y["grad"] * np.asarray(ref["A"], dtype=np.float64)
        lo = lo + k * y["loss"] * float(ref["loss"])
    return g, lo


def summed(parts):
    """sum of the ranks' results {loss, terms, grad}, in longdouble where it is wider (the sum itself then adds no rounding)"""
    wide = np.longdouble
    return {"loss": sum(wide(p["loss"]) for p in parts),
            "terms": tuple(sum(wide(p["terms"][j]) for p in parts) for j in range(3)),
            "grad": sum(np.asarray(p["grad"], dtype=wide) for p in parts)}


def additive_share(parts, full, bound_g, bound_lo):
    """-> (largest share of the bound used by a gradient entry, by the loss or a term); an entry without a bound (no term at
    all on either side) must be equal"""
    s = summed(parts)
    dg = np.asarray(np.abs(s["grad"] - np.asarray(full["grad"], dtype=np.longdouble)), dtype=np.float64)
    bound_g = np.broadcast_to(np.asarray(bound_g, dtype=np.float64), dg.shape)
    share_g = np.where(bound_g > 0, dg / np.where(bound_g > 0, bound_g, 1.0), np.where(dg > 0, np.inf, 0.0))
    dl = [abs(float(s["loss"] - np.longdouble(full["loss"])))] + [abs(float(a - np.longdouble(b))) for a, b in zip(s["terms"], full["terms"])]
    return float(np.max(share_g)), max(dl) / bound_lo, share_g


# ---- mutants ----------------------------------------------------------------------------------------------------------------------
def mutants(case, world):
    """-> {name: per-rank restatements [float64 dicts]} of wrong shardings; the ranks' sum of each has to leave the full
    restatement by more than additive_bound:
      local-f, local-u, local-b, local-w   one class divided by the rank's own count instead of the total (every class of the
                                           case with two rows or more)
      pair-shift                           the hi rows of every block taken one row later than the lo rows
      rows-by-data                         source and field rows taken from where the DATA block of the rank starts
      robin-drop                           the last Robin row of the last non-empty block dropped, the total kept"""
    x = _inputs(case["id"])
    run = lambda inp, tot: af.restate(case, np.float64, inp, **tot)      # noqa: E731
    blocks = [shard_inputs(case, world, r) for r in range(world)]
    out = {}

    def ranks(change):
        res = []
        for r, (inp, tot) in enumerate(blocks):
            inp, tot = change(r, dict(inp), dict(tot))
            if not is_empty(inp):
                res.append(run(inp, tot))
        return res

    for t, k in CLASS_OF_TOTAL.items():
        if case[k] >= 2 and (t != "n_w_total" or case["kind"] == "adr"):
            def change(r, inp, tot, t=t, k=k):
                n = shard_bounds(case[k], world, r)
                tot[t] = max(n[1] - n[0], 1)
                return inp, tot
            out["local-" + k[2:].replace("0", "u")] = ranks(change)
    if case["n_b"] >= 2:
        def change(r, inp, tot):
            lo, hi = shard_bounds(case["n_b"], world, r)
            idx = (np.arange(lo, hi) + 1) % case["n_b"]
            inp["X_hi"] = x["X_hi"][idx]
            return inp, tot
        out["pair-shift"] = ranks(change)
    if (x["s"] is not None or x["K"] is not None) and case["n_0"] and case["kind"] == "adr":
        def change(r, inp, tot):
            lo, _ = shard_bounds(case["n_0"], world, r)
            n = len(inp["X_f"])
            idx = (lo + np.arange(n)) % case["n_f"]                   # (rank 0 is right by accident: both blocks start at 0)
            if x["s"] is not None and n:
                inp["s"] = x["s"][idx]
            if x["K"] is not None and n:
                inp["K"] = x["K"][idx]
            return inp, tot
        out["rows-by-data"] = ranks(change)
    if case["n_w"] >= 2 and case["kind"] == "adr":
        last = max(r for r in range(world) if len(blocks[r][0]["robin"][0]))

        def change(r, inp, tot):
            if r == last:
                inp["robin"] = tuple(a[:-1] for a in inp["robin"])
            return inp, tot
        out["robin-drop"] = ranks(change)
    return out


def mutant_margins(case, world, dtype_name):
    """-> {mutant: largest share of additive_bound (at the case's largest allowance) that the mutant's sum is off by, against
    the full float64 restatement}"""
    x, tot = full_inputs(case)
    full = af.restate(case, np.float64, x, **tot)
    bg, blo = additive_bound(case, world, dtype_name, allowance(case, dtype_name))
    return {name: max(additive_share(parts, full, bg, blo)[:2]) for name, parts in mutants(case, world).items()}
