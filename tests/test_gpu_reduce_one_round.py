"""GPU: both load schedules of the gradient-row reduction (PINN_REDUCE_ONE_ROUND; csrc/kernels_optim.h, reduce_column) give
the same bits.

The product requests the 16 rows a thread owns of every 256 before its first wait (PINN_REDUCE_ONE_ROUND = 1).  The library is
built once more with profiles/build_variant.py:
    loop  -DPINN_REDUCE_ONE_ROUND=0   8 loads per round, then each row of the tail behind a wait of its own
Both must form the same sums: accumulator k of a slice takes rows q + 16 k, q + 16 k + 128, ... from 0.0, an absent row is
not added, ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7)), the slices in index order.  Compared BIT FOR BIT, per case of
tests/helpers/reduce_cases.py (float64 8x20 at 1, 2, 15, 16, 17, 112, 113, 127, 128, 129, 143, 144, 145, 158, 159, 160, 161,
255, 256 rows and one tile-loop set; a depth-4 float64 engine, a float32 engine and a two-member ensemble at 17, 158 and 256
rows): loss, loss terms and gradient of loss_grad(), the weights and losses of 3 Adam steps, the weights and the loss log of
lbfgs_begin + 3 iterations; run-to-run equality over 10 evaluations is asserted for either build.  That the builds really
differ is read off k_reduce_rows<double>: the product has no s_waitcnt vmcnt between the first and the last row load, the
other build has.  No tolerance anywhere: np.array_equal."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG, ROOT

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import reduce_cases  # noqa: E402

pytestmark = pytest.mark.gpu

WORKER = os.path.join(ROOT, "tests", "helpers", "reduce_cases.py")
KERNEL = "k_reduce_rowsIdE"                            # k_reduce_rows<double>
REPEATS = 10
PARTS = ("loss", "terms", "grad", "adam_losses", "adam_w", "lbfgs_iters", "lbfgs_losses", "lbfgs_w")


def _env(**extra):
    e = {k: v for k, v in os.environ.items() if k != "PINN_HIP_LIB"}
    e.update(extra)
    return e


def _row_loads_and_waits(lib):
    """(row loads, s_waitcnt vmcnt between the first and the last of them) of k_reduce_rows<double> of `lib`: the row loads
    are its 8-byte loads (the tile-scratch slots are read 32 bytes at a time), in the order of the code"""
    import isa_lint
    for _, blob in isa_lint.code_objects(lib):
        for name, ins in isa_lint.disassemble(blob).items():
            if KERNEL in name:
                at = [i for i, x in enumerate(ins) if x[1] == "global_load_dwordx2"]
                between = ins[at[0]:at[-1] + 1]
                return len(at), sum(x[1] == "s_waitcnt" and "vmcnt" in x[2] for x in between)
    raise AssertionError("no k_reduce_rows<double> in " + lib)


@pytest.fixture(scope="module")
def builds(tmp_path_factory):
    """{'product' | 'loop': {'lib': path, 'out': arrays of every case}}"""
    import pinn_native
    pinn_native.load()                                                   # the product library exists
    assert not os.environ.get("PINN_HIP_LIB"), "the product library is compared, not a variant"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "profiles", "build_variant.py"), "reduce_loop",
                        "-DPINN_REDUCE_ONE_ROUND=0"], env=_env(), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=1500)
    assert r.returncode == 0, r.stdout
    libs = {"product": pinn_native.LIB_PATH, "loop": r.stdout.strip().splitlines()[-1]}
    assert os.path.exists(libs["loop"]) and os.path.dirname(libs["loop"]) == os.path.join(PKG, "pinn_native", "abl")
    tmp = tmp_path_factory.mktemp("reduce_one_round")
    out = {}
    for tag, lib in libs.items():
        path = str(tmp / (tag + ".npz"))
        r = subprocess.run([sys.executable, WORKER, path, str(REPEATS)], env=_env(PINN_HIP_LIB=lib), capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, "%s build: %s" % (tag, r.stdout + r.stderr)
        out[tag] = dict(lib=lib, out=dict(np.load(path)))
    return out


def test_the_two_builds_run_different_code(builds):
    shape = {tag: _row_loads_and_waits(b["lib"]) for tag, b in builds.items()}
    print(shape)
    assert shape["product"][0] == 16 and shape["product"][1] == 0, shape       # one round: 16 loads, then the first wait
    assert shape["loop"][0] == 15 and shape["loop"][1] > 0, shape              # 8 in the loop + 7 of the tail, waits between


@pytest.mark.parametrize("case", reduce_cases.case_ids())
def test_bit_equal_to_the_loop_build(builds, case):
    new, old = builds["product"]["out"], builds["loop"]["out"]
    for part in PARTS:
        a, b = new["%s/%s" % (case, part)], old["%s/%s" % (case, part)]
        assert np.all(np.isfinite(a)) and a.shape == b.shape and a.size
        print("%s %s: %d of %d values differ" % (case, part, int(np.sum(a != b)), a.size))
        assert np.array_equal(a, b), "%s of %s differs between the product and the loop build" % (part, case)
    assert np.any(new[case + "/grad"] != 0.0)
    assert np.any(new[case + "/adam_w"] != new[case + "/lbfgs_w"])         # both optimisers moved the weights


@pytest.mark.parametrize("build", ["product", "loop"])
def test_run_to_run_bit_equality_over_10_evaluations(builds, build):
    out = builds[build]["out"]
    for case in reduce_cases.case_ids():
        key = case + "/repeats_equal"
        assert key in out and int(out[key]) == REPEATS, (key, out.get(key))
