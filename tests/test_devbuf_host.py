"""csrc/devbuf.h on the host: tests/host/devbuf_check.cpp (its own main, malloc/free behind the allocator macros, a switch
that fails the Nth allocation) built with AddressSanitizer + UBSan and run as a child process.  The sanitizer is linked
into that program; nothing is preloaded and nothing is loaded into Python.  No GPU."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "host", "devbuf_check.cpp")
FLAGS = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


# the sanitizer runtimes inside the program where the compiler can do that (gcc links them dynamically by default, and a
# dynamic AddressSanitizer insists on being the first library of the process), else the compiler's default
LINKS = [["-static-libasan", "-static-libubsan"], []]


def _sanitizing_compiler(tmp):
    """the first host compiler that builds AND runs an empty program with FLAGS -> (command, None), or (None, why not)"""
    probe = os.path.join(tmp, "probe.cpp")
    with open(probe, "w") as fh:
        fh.write("int main() { return 0; }\n")
    tried = []
    for cxx in ("g++", "clang++", "c++"):
        path = shutil.which(cxx)
        if not path:
            continue
        for link in LINKS:
            exe = os.path.join(tmp, "probe_%s_%d" % (os.path.basename(path), len(link)))
            res = subprocess.run([path] + FLAGS + link + [probe, "-o", exe], capture_output=True, text=True)
            if res.returncode == 0 and subprocess.run([exe], capture_output=True).returncode == 0:
                return [path] + FLAGS + link, None
            tried.append("%s: %s" % (path, (res.stderr.strip().splitlines() or ["the probe did not run"])[-1]))
    return None, "; ".join(tried) or "no host C++ compiler on PATH"


def test_devbuf_contract_under_sanitizers(tmp_path):
    cxx, why = _sanitizing_compiler(str(tmp_path))
    if cxx is None:
        pytest.skip("no host compiler supports -fsanitize=address,undefined here (%s)" % why)
    exe = str(tmp_path / "devbuf_check")
    res = subprocess.run(cxx + [SRC, "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    # leaks are counted by the program itself (blocks malloc gave against blocks free saw); LeakSanitizer's own pass needs
    # ptrace, which a container may withhold
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("devbuf_check ok"), run.stdout + run.stderr
