"""GPU: one context walked through every origin of its collocation block -- handed over, device LHS, an LHS redraw in place,
an adaptive draw in place, a re-assembly that keeps the draw, handed over again, LHS at another count -- and after every
step compared BIT FOR BIT (loss, the three terms, the gradient, get_collocation) with a fresh context put into that state
directly, same weights and seeds.  What a step leaves behind is the next step's starting state: an origin that is not
reset, a count taken from the old origin or a block start that moved shows as a differing bit.  Single transitions are
pinned elsewhere (tests/test_gpu_sampling.py, tests/test_gpu_rad.py, tests/test_gpu_adr_robin.py); the walk is not.

Counts: 5 data points and 70 collocation points (two tiles, 53 padding slots), then 64.  The adr walk carries 3 periodic
pairs and 2 Robin points throughout, so the Robin block stands behind a collocation block of changing origin.  Box B of
tests/helpers/boxes.py (sx != st, lb_t != 0): the device origins take their extents from the host's input map."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import boxes  # noqa: E402

pytestmark = pytest.mark.gpu

LB, UB = boxes.BOXES["B"]
N_U, N_F, N_F2, N_POOL = 5, 70, 64, 500
SETUPS = {                                   # name: (layers, pde, dtype, kernel path, pairs, Robin points)
    "burgers_f64_path7": ([2, 20, 20, 20, 20, 1], "burgers", "f64", 7, 0, 0),
    "burgers_f32_path0": ([2, 8, 8, 1], "burgers", "f32", 0, 0, 0),
    "adr_f64_path7": ([2, 20, 20, 20, 20, 1], "adr", "f64", 7, 3, 2),
}


def _inputs(name):
    layers, pde, dtype, path, n_b, n_w = SETUPS[name]
    rs = np.random.RandomState(11)
    n_params = sum(a * b + b for a, b in zip(layers[:-1], layers[1:]))
    inp = {"w": 0.9 / np.sqrt(layers[1]) * rs.standard_normal(n_params)}
    for tag in ("a", "b"):                   # two data sets and two handed-over collocation sets
        X_u = boxes.points(rs, N_U, LB, UB)
        inp["data_" + tag] = (X_u, np.sin(3.0 * boxes.unit(X_u, LB, UB)[:, 0:1]))
        inp["X_f_" + tag] = boxes.points(rs, N_F, LB, UB)
    inp["pairs"] = boxes.walls(rs, n_b, LB, UB)
    inp["robin"] = (boxes.wall_points(rs, n_w, LB, UB), rs.uniform(0.5, 1.5, n_w), rs.uniform(-1.5, 1.5, n_w),
                    rs.uniform(-1, 1, n_w))
    return inp


def _context(name, inp, data):
    """a context of this set-up with its weights, data set `data`, pairs and Robin points -- and no collocation block yet"""
    import pinn_native
    layers, pde, dtype, path, n_b, n_w = SETUPS[name]
    eng = pinn_native.Engine(layers, LB, UB, pde=pde, dtype=dtype)
    eng.set_kernel_path(path)
    if pde == "adr":
        eng.set_pde_params(*boxes.ADR_COEFFS)
        eng.set_boundary(*inp["pairs"])
        eng.set_robin(*inp["robin"])
    else:
        eng.set_pde_params(0.01 / np.pi)
    eng.set_data(*inp["data_" + data])
    eng.set_weights(inp["w"])
    assert eng.kernel_path() == path
    return eng


def _state(eng):
    loss, grad, terms = eng.loss_grad()
    return {"loss": np.float64(loss), "terms": terms, "grad": grad, "X_f": eng.get_collocation()}


# (step, what the walked context does, data set of the fresh context, how the fresh context gets there directly)
STEPS = [
    ("handed over", lambda e, i: e.set_collocation(i["X_f_a"]), "a", lambda e, i: e.set_collocation(i["X_f_a"])),
    ("device LHS", lambda e, i: e.lhs_collocation(N_F, 0xA1), "a", lambda e, i: e.lhs_collocation(N_F, 0xA1)),
    ("LHS redraw in place", lambda e, i: e.lhs_collocation(N_F, 0xA2), "a", lambda e, i: e.lhs_collocation(N_F, 0xA2)),
    ("adaptive draw in place", lambda e, i: e.rad_collocation(N_F, 0xA3, N_POOL, k=2, c=0.5), "a",
     lambda e, i: e.rad_collocation(N_F, 0xA3, N_POOL, k=2, c=0.5)),
    ("data replaced, draw kept", lambda e, i: e.set_data(*i["data_b"]), "b",
     lambda e, i: e.rad_collocation(N_F, 0xA3, N_POOL, k=2, c=0.5)),
    ("handed over again", lambda e, i: e.set_collocation(i["X_f_b"]), "b", lambda e, i: e.set_collocation(i["X_f_b"])),
    ("LHS at another count", lambda e, i: e.lhs_collocation(N_F2, 0xA4), "b", lambda e, i: e.lhs_collocation(N_F2, 0xA4)),
]


@pytest.mark.parametrize("name", sorted(SETUPS))
def test_walk_through_the_origins_matches_fresh_contexts_bit_for_bit(name):
    inp = _inputs(name)
    walked = _context(name, inp, "a")
    seen = []
    for step, move, data, direct in STEPS:
        move(walked, inp)
        got = _state(walked)                 # (the evaluation also assembles the set: the next step starts from it)
        fresh = _context(name, inp, data)
        direct(fresh, inp)
        want = _state(fresh)
        fresh.close()
        assert got["X_f"].shape == want["X_f"].shape == (N_F2 if step == STEPS[-1][0] else N_F, 2), step
        for key in ("X_f", "loss", "terms", "grad"):
            assert np.array_equal(got[key], want[key]), (name, step, key)
        assert np.isfinite(got["loss"]) and np.all(np.isfinite(got["grad"])) and np.any(got["grad"] != 0.0), (name, step)
        seen.append(got)
    walked.close()
    # the steps are different states, not one state seven times: every step but the re-assembly moved the points, and the
    # re-assembly kept them and moved the data term
    for k in (1, 2, 3, 5):
        assert not np.array_equal(seen[k]["X_f"], seen[k - 1]["X_f"]), STEPS[k][0]
    assert np.array_equal(seen[4]["X_f"], seen[3]["X_f"]) and not np.array_equal(seen[4]["terms"], seen[3]["terms"])
