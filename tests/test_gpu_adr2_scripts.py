"""GPU: the two scripts of the adr2 kind, 1d-wave/inf_cont_wave.py and 2d-helmholtz/inf_helmholtz.py, run as child processes
with a short hp the way tests/test_gpu_scripts.py runs its scripts: the run ends, the logged loss is finite and falls below its
first logged value, and the error line is printed."""
import math
import os

import pytest

from test_gpu_scripts import END, parse, run_script

pytestmark = pytest.mark.gpu

SHORT = {"layers": [2, 20, 20, 20, 20, 1], "tf_epochs": 30, "tf_lr": 0.003, "tf_b1": 0.9, "tf_eps": None,
         "nt_epochs": 30, "nt_lr": 0.8, "nt_ncorr": 50, "log_frequency": 10}


def check(out, n_epochs):
    assert "Training started" in out and "-- Starting Adam optimization --" in out
    rows, end = parse(out)
    assert len(rows) >= 4 and all(math.isfinite(r[2]) for r in rows)
    assert rows[-1][2] < rows[0][2], rows
    assert end is not None and end[0] == n_epochs and math.isfinite(end[1]) and end[1] > 0.0
    assert sum(1 for line in out.splitlines() if END.match(line)) == 1


@pytest.mark.parametrize("equation", ["wave", "telegraph", "klein_gordon"])
def test_inf_cont_wave_runs(tmp_path, equation):
    hp = dict(SHORT, equation=equation, N_0=64, N_w=32, N_f=1024)
    out = run_script(os.path.join("1d-wave", "inf_cont_wave.py"), hp, tmp_path)
    check(out, 60)
    assert "Residual: max |N[u] - s| =" in out and "(%s)" % equation in out


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_inf_helmholtz_runs(tmp_path, dtype):
    hp = dict(SHORT, k=4.0, N_w=32, N_f=1024, dtype=dtype)
    out = run_script(os.path.join("2d-helmholtz", "inf_helmholtz.py"), hp, tmp_path)
    check(out, 60)
    assert "Residual with the source: max |N[u] - s| =" in out
