"""Allen-Cahn continuous-time ensemble: the members of hp["members"] -- seeds and / or coefficient rows of the engine's "adr"
kind -- trained side by side on one point set by one engine ensemble (utils/ensemble.py, pinn_native.AdrEnsemble), then one
line per member: its relative L2 error against allencahnutil's own solver, run once per distinct coefficient set.
    python 1d-allen-cahn/ens_cont_allen_cahn.py [hp.json]          (run from the package root)
hp["members"] is a number K (member k uses hp["seed"] + k, default 1234 + k, and the script's coefficients) or a list of
dicts with the per-member keys of utils/ensemble.py: "seed", "tf_lr", "nt_lr", "nt_epochs", "init_scale" and
    "adr": [a0, a1, nu, r1, r2, r3]     the member's coefficients.  The exact field exists for the Allen-Cahn family
                                        u_t - nu u_xx - rho (u - u^3) = 0, i.e. rows [0, 0, nu, -rho, 0, rho]: an interface-
                                        width sweep is a list of such rows; any other row is refused.
Member k ends bit-identical to inf_cont_allen_cahn.py's model with member k's seed and coefficients trained alone.
hp["solver_modes"] / hp["solver_substeps"] (default: allencahnutil's 4096 / 50) set the reference solver's resolution.
"""
import json
import os
import sys

import numpy as np

np.random.seed(1234)

eqnPath = "1d-allen-cahn"
_root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(os.path.join(_root, eqnPath))
sys.path.append(os.path.join(_root, "utils"))
from logger import Logger  # noqa: E402
from ensemble import NeuralNetworkEnsemble  # noqa: E402
import allencahnutil  # noqa: E402
from allencahnutil import ADR_COEFFS, N_SOLVE, N_T, N_X, SUBSTEPS, exact_field, prep_data, solve_allen_cahn  # noqa: E402

if len(sys.argv) > 1:
    with open(sys.argv[1]) as hpFile:
        hp = json.load(hpFile)
else:
    hp = {"members": 8}
defaults = {"N_0": 512, "N_b": 200, "N_f": 20000, "layers": [2, 20, 20, 20, 20, 20, 20, 20, 20, 1],   # inf_cont_allen_cahn.py
            "tf_epochs": 100, "tf_lr": 0.03, "tf_b1": 0.9, "tf_eps": None,
            "nt_epochs": 200, "nt_lr": 0.8, "nt_ncorr": 50, "log_frequency": 10}
hp = dict(defaults, **hp)
SCRIPT_KEYS = ("members", "seed", "solver_modes", "solver_substeps")


def member_list(hp):
    seed0 = int(hp.get("seed", 1234))
    m = hp["members"]
    if isinstance(m, int):
        return [{"seed": seed0 + k} for k in range(m)]
    return [dict(d) for d in m]


def reference_field(row, n_modes, substeps, cache_dir):
    """the exact field on the comparison grid for one coefficient row of the Allen-Cahn family -> Exact_u [N_T, N_X]"""
    a0, a1, nu, r1, r2, r3 = (float(v) for v in row)
    if a0 != 0.0 or a1 != 0.0 or r2 != 0.0 or r1 != -r3 or nu <= 0.0:
        raise ValueError("no reference solver for the coefficients %r: the exact field exists for rows "
                         "[0, 0, nu, -rho, 0, rho] only" % (list(row),))
    if tuple(row) == tuple(ADR_COEFFS) and (n_modes, substeps) == (N_SOLVE, SUBSTEPS):
        return exact_field(cache_dir)[2]                   # the script family's cached field
    if n_modes % N_X:
        raise ValueError("solver_modes (%d) must be a multiple of %d" % (n_modes, N_X))
    _, _, U = solve_allen_cahn(n_modes, N_T, substeps, nu=nu, rho=r3)
    return np.ascontiguousarray(U[:, ::n_modes // N_X])


def run(hp):
    cache_dir = os.path.join(_root, eqnPath, "results")
    n_modes, substeps = int(hp.get("solver_modes", N_SOLVE)), int(hp.get("solver_substeps", SUBSTEPS))
    members = member_list(hp)
    rows = [tuple(float(v) for v in m.get("adr", ADR_COEFFS)) for m in members]
    fields = {row: reference_field(row, n_modes, substeps, cache_dir) for row in sorted(set(rows))}   # once per distinct set
    x = (-1.0 + 2.0 * np.arange(N_X) / N_X).reshape(-1, 1)
    t = np.linspace(0.0, 1.0, N_T).reshape(-1, 1)
    # the point sets are the first member's equation's: initial data u(x, 0) does not depend on the coefficients
    (x, t, X, T, Exact_u, X_star, u_star, X_u_train, u_train, X_f, X_lb, X_ub, ub, lb) = prep_data(
        hp["N_0"], hp["N_b"], hp["N_f"], field=(x, t, fields[rows[0]]))
    hp_model = {k: v for k, v in hp.items() if k not in SCRIPT_KEYS}
    logger = Logger(hp)
    ens = NeuralNetworkEnsemble(hp_model, logger, ub, lb, members, pde="adr")
    ens.set_collocation(X_f)
    ens._set_boundary(X_lb, X_ub)
    ens.set_pde_params(ADR_COEFFS)                          # (a member's "adr" row wins)
    ens.fit(X_u_train, u_train)
    errs = {row: ens.error_l2(X_star, U.reshape(-1, 1)) for row, U in fields.items()}   # [K] per distinct set
    err = np.array([errs[rows[k]][k] for k in range(len(members))])
    for k, m in enumerate(members):
        print("member %2d  seed %s  nu = %.3e  rho = %.3e  error = %.6e  L-BFGS done %d" % (
            k, m.get("seed", "-"), rows[k][2], rows[k][5], err[k], ens.nt_done[k]))
    return ens, err


if __name__ == "__main__":
    run(hp)
