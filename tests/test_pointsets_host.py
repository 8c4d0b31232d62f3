"""csrc/pointsets.h on the host: tests/host/pointsets_check.cpp (its own main, that header alone) built with
AddressSanitizer + UBSan and run as a child process -- the SetDesc builder, the block starts, the one set assembler over
pair / data / collocation / Robin counts at the tile edges, K members into adjacent slices between guards, and the input map
on the offset boxes.  The compiler probe and the skip rule are tests/test_devbuf_host.py's.  Nothing is preloaded and nothing
is loaded into Python.  No GPU."""
import os
import subprocess

import pytest

from conftest import ROOT
from test_devbuf_host import _sanitizing_compiler

SRC = os.path.join(ROOT, "tests", "host", "pointsets_check.cpp")


def test_pointsets_under_sanitizers(tmp_path):
    cxx, why = _sanitizing_compiler(str(tmp_path))
    if cxx is None:
        pytest.skip("no host compiler supports -fsanitize=address,undefined here (%s)" % why)
    exe = str(tmp_path / "pointsets_check")
    res = subprocess.run(cxx + ["-Wall", "-Wextra", "-Werror", SRC, "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")      # (LeakSanitizer's pass needs ptrace; the program owns vectors only)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("pointsets_check ok"), run.stdout + run.stderr
