"""csrc/optim_host.h on the host: tests/host/optim_host_check.cpp (its own main, that header alone) built with
AddressSanitizer + UBSan and run as a child process -- the ticket counters across the 31-bit wrap, Adam's step factors for
t = 1 .. 2000 against the written-out expression with ==, the loss ring's layout, and the L-BFGS log window and hand-out
against a model of the device's logging: max_iter 0..12, chunks of 1..6, the host 0..3 chunks behind, every logging pattern
and every break position.  The compiler probe and the skip rule are tests/test_devbuf_host.py's.  Nothing is preloaded and
nothing is loaded into Python.  No GPU."""
import os
import subprocess

import pytest

from conftest import ROOT
from test_devbuf_host import _sanitizing_compiler

SRC = os.path.join(ROOT, "tests", "host", "optim_host_check.cpp")


def test_optim_host_under_sanitizers(tmp_path):
    cxx, why = _sanitizing_compiler(str(tmp_path))
    if cxx is None:
        pytest.skip("no host compiler supports -fsanitize=address,undefined here (%s)" % why)
    exe = str(tmp_path / "optim_host_check")
    res = subprocess.run(cxx + ["-Wall", "-Wextra", "-Werror", SRC, "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")      # (LeakSanitizer's pass needs ptrace; the program owns vectors only)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("optim_host_check ok"), run.stdout + run.stderr
