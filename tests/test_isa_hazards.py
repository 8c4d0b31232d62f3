"""The built library's device code holds none of the two hazards inline asm can hide from hipcc's hazard recogniser
(tests/helpers/isa_lint.py: matrix-instruction result read by an accvgpr move too early; m0 written right in front of an
LDS-DMA load).  CPU only: reads the gfx950 code objects out of libpinn_hip.so with objcopy + llvm-objdump."""
import os
import shutil
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import isa_lint  # noqa: E402

needs_tools = pytest.mark.skipif(not (os.path.exists(isa_lint.OBJDUMP) and shutil.which(isa_lint.OBJCOPY)),
                                 reason="llvm-objdump / objcopy not here")


def _body(lines):
    return [(4 * i, mn, ops, None) for i, (mn, ops) in enumerate(lines)]


def test_the_lint_sees_the_hazards_it_is_there_for():
    put = ("v_accvgpr_write_b32", "a5, v10")
    dgemm = ("v_mfma_f64_4x4x4_4b_f64", "v[10:11], v[2:3], v[4:5], v[10:11]")
    filler = ("v_add_f64", "v[20:21], v[22:23], v[24:25]")
    # the round-2 bug: the parked word is read straight out of the matrix instruction
    assert len(isa_lint.lint_function("k", _body([dgemm, put]))) == 1
    assert len(isa_lint.lint_function("k", _body([dgemm] + [filler] * 5 + [put]))) == 1
    assert isa_lint.lint_function("k", _body([dgemm] + [filler] * 6 + [put])) == []
    assert isa_lint.lint_function("k", _body([dgemm, ("s_nop", "5"), put])) == []
    assert len(isa_lint.lint_function("k", _body([dgemm, ("s_nop", "4"), put]))) == 1
    # a compiler-visible instruction that overwrites the register ends the hazard; an unrelated register never had one
    assert isa_lint.lint_function("k", _body([dgemm, ("v_mov_b32_e32", "v10, v3"), put])) == []
    assert isa_lint.lint_function("k", _body([dgemm, ("v_accvgpr_write_b32", "a5, v12")])) == []
    # ... and it follows branches: the read sits at the branch target
    body = [(0, "v_mfma_f32_16x16x4_f32", "a[0:3], v1, v2, a[0:3]", None), (8, "s_branch", "2", 20),
            (12, "v_accvgpr_write_b32", "a0, 0", None), (20, "v_accvgpr_read_b32", "v9, a0", None)]
    assert len(isa_lint.lint_function("k", body)) == 1
    body[1] = (8, "s_branch", "0", 12)
    assert isa_lint.lint_function("k", body[:3]) == []
    # m0
    dma = ("global_load_lds_dwordx4", "v[44:45], off")
    assert len(isa_lint.lint_function("k", _body([("s_mov_b32", "m0, s5"), dma]))) == 1
    assert isa_lint.lint_function("k", _body([("s_mov_b32", "m0, s5"), ("s_nop", "0"), dma])) == []


@needs_tools
def test_no_hidden_hazard_in_the_built_library():
    import pinn_native
    pinn_native.load()                      # builds it if it is not there (hipcc cross-compiles without a GPU)
    n, seen, bad = isa_lint.lint_library(pinn_native.LIB_PATH)
    # the walk saw what it is meant to judge: the AGPR stash of the width-20 kernels and the LDS-DMA of the float32 ones
    assert n > 50 and seen["mfma"] > 10000 and seen["v_accvgpr_write_b32"] > 1000 and seen["lds_dma"] > 20, (n, seen)
    assert bad == [], "\n".join(bad[:20])


@needs_tools
def test_no_scratch_in_the_kernels_that_serve_the_baseline_configs_or_the_exchange():
    """Code-object metadata of the built library (llvm-readelf --notes): the loss+gradient kernels of BASELINE configs[1..4],
    the reduction / optimiser kernels behind them and -- since round 6 -- every variant of k_reduce_xgmi (the fallback exchange
    when RCCL fails everywhere; it carried 18 spilled registers until round 5) use no private segment and spill nothing."""
    import re
    import subprocess
    import tempfile
    import pinn_native
    readelf = os.path.join(os.path.dirname(isa_lint.OBJDUMP), "llvm-readelf")
    if not os.path.exists(readelf):
        pytest.skip("llvm-readelf not here")
    pinn_native.build()
    wanted = ("k_reduce_xgmi", "k_fused20dILi0ELi8", "k_fused20dILi1ELi8", "k_fused20mILi0ELi8", "k_fused20mILi1ELi8",
              "k_t16_fusedILi2ELi4", "k_reduce_adam", "k_reduce_rows", "k_lbc_dots", "k_lbc_coef_apply")
    seen = {}
    for _, obj in isa_lint.code_objects(pinn_native.LIB_PATH):
        with tempfile.NamedTemporaryFile(suffix=".o") as fh:
            fh.write(obj)
            fh.flush()
            notes = subprocess.run([readelf, "--notes", fh.name], check=True, capture_output=True, text=True).stdout
        for blk in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk).group(1)
            if any(w in name for w in wanted):
                seen[name] = (int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)),
                              int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)))
    assert sum("k_reduce_xgmi" in n for n in seen) == 4 and any("k_t16_fusedILi2ELi4" in n for n in seen), sorted(seen)
    bad = {n: v for n, v in seen.items() if v != (0, 0)}
    assert not bad, bad


@needs_tools
def test_the_kernel_listing_names_every_kernel_with_its_digest_and_resources():
    """`isa_lint.py --listing`: what two builds are compared by (profiles/refactor_paths_device_code.txt).  Every kernel has
    a line, with metadata from the code object's notes; k_fused20d's variants sit in their own code object, all under that
    one name, and their template arguments are exactly the table below (a new variant adds its row); k_split20d, the same
    text with the two roles compiled in, is the only other name there; the listing of one library is the same twice."""
    import re
    import pinn_native
    if not os.path.exists(isa_lint.READELF):
        pytest.skip("llvm-readelf not here")
    pinn_native.load()
    lines = isa_lint.kernel_listing(pinn_native.LIB_PATH)
    assert len(lines) > 50 and len(set(lines)) == len(lines)
    form = re.compile(r"^\d+ \S+ insns=\d+ sha=[0-9a-f]{16} vgpr=\d+ agpr=\d+ sgpr=\d+ lds=\d+ scratch=\d+$")
    assert all(form.match(l) for l in lines), [l for l in lines if not form.match(l)][:3]
    # PDE -> the (ENS, SETS, SAW) it is built with; each row at H = 4, 6, 8, tile loop and one tile
    variants = {0: [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 0, 1)],        # Burgers inference: solo, ensembles, point weights
                1: [(0, 0, 0), (1, 0, 0), (1, 1, 0)],                   # Burgers identification: solo, ensembles
                3: [(0, 0, 0), (0, 0, 1)],                              # adr, and with point weights
                4: [(0, 0, 0)], 5: [(0, 0, 0)], 6: [(0, 0, 0)], 7: [(0, 0, 0)],   # adr_ide, Robin, source, fields
                8: [(1, 0, 0), (1, 1, 0)]}                              # adr ensembles
    args = re.compile(r"^_ZN4pinn10k_(fused|split)20dILi(\d+)ELi(\d+)ELb([01])ELb([01])ELb([01])ELb([01])EE")

    def built(kind):                      # (PDE, H, ONE_TILE, ENS, SETS, SAW) of every kernel of that name, in listing order
        found = [args.match(l.split()[1]) for l in lines if "k_%s20dI" % kind in l]
        assert all(found), [l for l in lines if "k_%s20dI" % kind in l and not args.match(l.split()[1])][:3]
        return [tuple(int(v) for v in m.groups()[1:]) for m in found if m.group(1) == kind]
    want = {(pde, H, one) + row for pde, rows in variants.items() for row in rows for H in (4, 6, 8) for one in (0, 1)}
    fused, split = built("fused"), built("split")
    assert len(want) == 90 and len(fused) == 90 and set(fused) == want, (sorted(set(fused) - want), sorted(want - set(fused)))
    assert len(split) == 6 and set(split) == {(pde, H, 1, 0, 0, 0) for pde in (0, 1) for H in (4, 6, 8)}, split
    obj = {l.split()[0] for l in lines if "k_fused20dI" in l}
    assert len(obj) == 1
    others = [l for l in lines if l.split()[0] in obj and "k_fused20dI" not in l and "k_split20dI" not in l]
    assert not others, others[:3]
    retired = ("k_robin20d", "k_src20d", "k_var20d", "k_adrens20d", "k_fused20d_")
    assert not [l for l in lines if any(r in l.split()[1] for r in retired)]
    assert lines == isa_lint.kernel_listing(pinn_native.LIB_PATH)
