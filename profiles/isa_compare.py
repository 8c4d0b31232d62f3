"""Per-kernel instruction-stream comparison of two builds of libpinn_hip.so.

    python profiles/isa_compare.py BEFORE.so AFTER.so [substring of the new kernels' names]

Every gfx950 code object of both libraries is unbundled (llvm-objdump --offloading) and disassembled (-d
--no-show-raw-insn); kernels are matched by their demangled name up to the argument list (template arguments included,
argument types not: a parameter whose type became a std::conditional changes the mangled name of every instantiation and
nothing else), and mnemonics + operands are compared line by line with addresses and branch-target comments dropped.
Prints identical / differing / new / removed kernels and, for the new kernels whose name holds the given substring, the
register, scratch and LDS figures of the code-object metadata.
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")


def run(*cmd, cwd=None):
    return subprocess.run(cmd, cwd=cwd, check=True, capture_output=True, text=True).stdout


def kernels_of(lib):
    """-> {short demangled name: [instruction lines]}, {short name: metadata dict}"""
    code, meta = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        local = os.path.join(tmp, "lib.so")
        with open(lib, "rb") as src, open(local, "wb") as dst:
            dst.write(src.read())
        run(os.path.join(LLVM, "llvm-objdump"), "--offloading", "lib.so", cwd=tmp)
        for co in sorted(f for f in os.listdir(tmp) if "amdgcn" in f):
            path = os.path.join(tmp, co)
            dis = run(os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "-C", path)
            cur = None
            for line in dis.splitlines():
                m = re.match(r"^[0-9a-f]+ <(.*)>:$", line)
                if m:
                    name = short(m.group(1))
                    cur = code.setdefault(name, []) if "k_" in name else None
                    continue
                if cur is not None and line[:1] in " \t" and line.strip():
                    ins = line.split("//")[0].strip()
                    ins = re.sub(r"<[^>]*\+0x[0-9a-f]+>", "", ins)
                    if ins and ins != "...":         # ("...": the disassembler's mark for the zero padding behind a kernel)
                        cur.append(ins)
            notes = run(os.path.join(LLVM, "llvm-readelf"), "--notes", path)
            for blk in notes.split("- .agpr_count:")[1:]:
                f = dict(re.findall(r"\.(\w+):\s+(\S+)", ".agpr_count:" + blk.split("\n  - ")[0]))
                if ".name" in blk and "name" in f:
                    dn = run(shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "c++filt", f["name"]).strip()
                    meta[short(dn)] = f
    return code, meta


def short(demangled):
    """'void pinn::k_x<1, 2>(args...) [clone .kd]' -> 'pinn::k_x<1, 2>'"""
    s = re.sub(r"^void ", "", demangled)
    depth, out = 0, []
    for ch in s:
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            break
        out.append(ch)
    return "".join(out).strip()


def main():
    before, after = sys.argv[1], sys.argv[2]
    new_tag = sys.argv[3] if len(sys.argv) > 3 else None
    cb, _ = kernels_of(before)
    ca, ma = kernels_of(after)
    same = [k for k in cb if k in ca and cb[k] == ca[k]]
    diff = [k for k in cb if k in ca and cb[k] != ca[k]]
    new = sorted(k for k in ca if k not in cb)
    gone = sorted(k for k in cb if k not in ca)
    print("kernels before %d, after %d: identical %d, differing %d" % (len(cb), len(ca), len(same), len(diff)))
    for k in diff:
        print("  DIFFERS: %s (%d -> %d instructions)" % (k, len(cb[k]), len(ca[k])))
    print("removed: %s" % gone)
    print("new in after (%d):" % len(new))
    for k in new:
        print("  %s  (%d instructions)" % (k, len(ca[k])))
    if new_tag:
        print("resources of the new kernels matching %r (code-object metadata):" % new_tag)
        for k in new:
            if new_tag in k and k in ma:
                f = ma[k]
                print("  %s: vgpr_count %s (of which agpr %s), sgpr %s, vgpr spills %s, sgpr spills %s, scratch %s B, "
                      "static LDS %s B" % (k, f.get("vgpr_count"), f.get("agpr_count"), f.get("sgpr_count"),
                                          f.get("vgpr_spill_count"), f.get("sgpr_spill_count"),
                                          f.get("private_segment_fixed_size"), f.get("group_segment_fixed_size")))
    return 1 if diff or gone else 0


if __name__ == "__main__":
    sys.exit(main())
