"""GPU: the settings of the one-tile float64 workgroup sum (PINN_ONETILE_SUM, PINN_ROW_STORE_WT; csrc/kernels_fused20d.h) give
the same bits.

The product parks every lane's unfolded partial block and adds 4 waves x 4 blocks per entry (PINN_ONETILE_SUM = 0), and writes
the gradient row with write-through stores (PINN_ROW_STORE_WT = 1).  The library is built three more times with
profiles/build_variant.py:
    sum1   -DPINN_ONETILE_SUM=1   the four blocks folded in registers (two DPP row rotations) before a shorter per-layer sum
    sum2   -DPINN_ONETILE_SUM=2   the same fold, one sum behind the sweep
    plain  -DPINN_ROW_STORE_WT=0  the parent's plain row stores
The folds must form exactly the association of the sum they replace, (b0 + b1) + (b2 + b3) per wave and ((w0 + w1) + w2) + w3
over the waves -- which of the four blocks ends with that total depends on the direction of the DPP row rotation, and this test
pins it.  Loss, loss terms and gradient of all four builds are compared BIT FOR BIT on
  pde 0 (Burgers inference), 1 (identification) and adr  x  depths 4, 6, 8  x  canonical / perturbed weights,
  and one set per pde whose last tile is partly padding;
run-to-run equality over 20 evaluations is asserted for every build.  That the builds really differ is read off their device
code: the folded kernels hold hundreds of DPP moves and a quarter of the ds_read_b128, the plain build no sc1 store.
No tolerance anywhere: np.array_equal."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG, ROOT

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import onetile_cases  # noqa: E402

pytestmark = pytest.mark.gpu

WORKER = os.path.join(ROOT, "tests", "helpers", "onetile_cases.py")
VARIANTS = {"sum1": ["-DPINN_ONETILE_SUM=1"], "sum2": ["-DPINN_ONETILE_SUM=2"], "plain": ["-DPINN_ROW_STORE_WT=0"]}
HEADLINE = "k_fused20dILi0ELi8ELb1ELb0ELb0ELb0E"         # k_fused20d<0, 8, true, false, false, false>


def _env(**extra):
    e = {k: v for k, v in os.environ.items() if k != "PINN_HIP_LIB"}
    e.update(extra)
    return e


def _shape_of(lib):
    """(DPP moves, ds_read_b128, write-through stores, plain 8-byte stores) of the headline one-tile kernel of `lib`"""
    import isa_lint
    for _, blob in isa_lint.code_objects(lib):
        for name, ins in isa_lint.disassemble(blob).items():
            if HEADLINE in name:
                st = [i for i in ins if i[1] == "global_store_dwordx2"]
                wt = sum("sc1" in i[2] for i in st)
                return (sum(i[1].startswith("v_mov_b32_dpp") or "row_ror" in i[2] for i in ins),
                        sum(i[1] == "ds_read_b128" for i in ins), wt, len(st) - wt)
    raise AssertionError("no headline one-tile kernel in " + lib)


@pytest.fixture(scope="module")
def builds(tmp_path_factory):
    """{'product' | 'sum1' | 'sum2' | 'plain': {'lib': path, 'out': arrays of every case, 'again': 20-evaluation check}}"""
    import pinn_native
    pinn_native.load()                                                   # the product library exists
    assert not os.environ.get("PINN_HIP_LIB"), "the product library is compared, not a variant"
    procs = {tag: subprocess.Popen([sys.executable, os.path.join(ROOT, "profiles", "build_variant.py"), "onetile_" + tag] + flags,
                                   env=_env(), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for tag, flags in VARIANTS.items()}
    libs = {"product": pinn_native.LIB_PATH}
    for tag, p in procs.items():
        log = p.communicate(timeout=1500)[0]
        assert p.returncode == 0, log
        libs[tag] = log.strip().splitlines()[-1]
        assert os.path.exists(libs[tag]) and os.path.dirname(libs[tag]) == os.path.join(PKG, "pinn_native", "abl")
    tmp = tmp_path_factory.mktemp("onetile_fold")
    out = {}
    for tag, lib in libs.items():
        path = str(tmp / (tag + ".npz"))
        r = subprocess.run([sys.executable, WORKER, path, "20"], env=_env(PINN_HIP_LIB=lib), capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, "%s build: %s" % (tag, r.stdout + r.stderr)
        out[tag] = dict(lib=lib, out=dict(np.load(path)))
    return out


def test_the_four_builds_run_different_code(builds):
    shape = {tag: _shape_of(b["lib"]) for tag, b in builds.items()}
    print(shape)
    for tag in ("product", "plain"):                 # unfolded: 16 reads per thread and layer, no fold
        assert shape[tag][0] < 100 and shape[tag][1] >= 100, shape
    for tag in ("sum1", "sum2"):                     # 221 blocks x 4 DPP moves, 4 reads per thread and layer
        assert shape[tag][0] >= 800 and shape[tag][1] <= 40, shape
    assert shape["product"][2] >= 10 and shape["plain"][2] == 0 and shape["plain"][3] > shape["product"][3], shape


@pytest.mark.parametrize("case", onetile_cases.case_ids())
@pytest.mark.parametrize("other", sorted(VARIANTS))
def test_bit_equal_to_the_product(builds, other, case):
    new, old = builds["product"]["out"], builds[other]["out"]
    for part in ("loss", "terms", "grad"):
        a, b = new["%s/%s" % (case, part)], old["%s/%s" % (case, part)]
        assert np.all(np.isfinite(a)) and a.shape == b.shape
        n_diff = int(np.sum(a != b))
        print("%s %s vs %s: %d of %d values differ, max |diff| %.3e" % (case, part, other, n_diff, a.size,
                                                                       float(np.max(np.abs(a - b))) if a.size else 0.0))
        assert np.array_equal(a, b), "%s of %s differs between the product and the %s build" % (part, case, other)
    assert np.any(new[case + "/grad"] != 0.0)


@pytest.mark.parametrize("build", ["product"] + sorted(VARIANTS))
def test_run_to_run_bit_equality_over_20_evaluations(builds, build):
    out = builds[build]["out"]
    for pde in onetile_cases.PDES:
        key = "%s-d8-perturbed-ragged/repeats_equal" % pde
        assert key in out and int(out[key]) == 20, (key, out.get(key))
