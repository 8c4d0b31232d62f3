"""Korteweg-de Vries discrete-time identification on the MI355X engine: recover a1 and d3 of

    u_t + a1 u u_x + d3 u_xxx = 0                (truth: a1 = 1, d3 = 0.0025; no diffusion, nu = 0)

from two snapshots of a soliton and nothing in between -- the showcase of the discrete-time method: q implicit Runge-Kutta
stages bridge the large gap between t_0 and t_1.  Same CLI, hp keys and stdout log as 1d-allen-cahn/ide_disc_allen_cahn.py
(`python 1d-kdv/ide_disc_kdv.py [hp.json]` from the package root), with the trained coefficients appended to each progress
line.

The snapshots (x_0, u_0) at t_0 and (x_1, u_1) at t_1 = t_0 + dt constrain the q stage values the network outputs
(n_out = q):
    U_0_model = U + dt N(U) A^T,   U_1_model = U - dt N(U) (b - A)^T,
    N(U) = (a0 + a1 U) U_x - nu U_xx + d3 U_xxx + r1 U + r2 U^2 + r3 U^3
with the Gauss-Legendre table (A, b) of utils/irk.py; the loss is the sum of both squared misfits (the soliton is below 1e-4
at the walls, so there are no periodic pairs).  It is the engine's "adrd_disc" kind (csrc/kernels_disc.h, four Taylor
channels): seven coefficients sit behind the network weights, hp["adr_trainable"] names the ones that are learned (default
a1 and d3; the others stay frozen at their start values, bit for bit, nu at exactly 0) and hp["adr_init"] gives the start
values, away from the truth.  The snapshots are kdvutil.soliton on a uniform grid -- a closed form, no data file.

The kind holds hidden layers up to 64 wide in both dtypes; the default arithmetic is float64.
"""
import json
import os
import sys

import numpy as np

np.random.seed(1234)

eqnPath = "1d-kdv"
_root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(os.path.join(_root, eqnPath))
sys.path.append(os.path.join(_root, "utils"))
from logger import Logger  # noqa: E402
from neuralnetwork import ADRD_NAMES, NeuralNetwork, set_seed  # noqa: E402
from irk import gauss_legendre_butcher  # noqa: E402
from kdvutil import KDV_COEFFS, LB, UB, snapshot  # noqa: E402

set_seed(1234)

if len(sys.argv) > 1:
    with open(sys.argv[1]) as hpFile:
        hp = json.load(hpFile)
else:
    hp = {
        "N_0": 199, "N_1": 201,            # data points on the two snapshots
        "q": 50,                           # Runge-Kutta stages
        "layers": [1, 50, 50, 50, 50, 0],  # the output size (q) is set below
        "tf_epochs": 1000, "tf_lr": 0.001, "tf_b1": 0.9, "tf_eps": 1e-08,    # Adam
        "nt_epochs": 20000, "nt_lr": 0.8, "nt_ncorr": 50,                    # L-BFGS
        "log_frequency": 100,
    }
hp.setdefault("log_frequency", 10)
hp.setdefault("t_0", 0.2)
hp.setdefault("t_1", 0.8)
hp.setdefault("adr_trainable", ["a1", "d3"])
hp.setdefault("adr_init", [0.0, 0.5, 0.0, 0.0, 0.0, 0.0, 0.005])      # a1, d3 start away from the truth [1, 0.0025]; nu = 0 frozen


class KdVDiscreteIdentificationNN(NeuralNetwork):
    pde = "adrd_disc"

    def __init__(self, hp, logger, dt, lb, ub, q, IRK_alpha, IRK_beta):
        super().__init__(hp, logger, ub, lb)
        self.dt = float(dt)
        self.q = max(q, 1)
        self.IRK_alpha = np.asarray(IRK_alpha, dtype=np.float64)      # A [q, q]
        self.IRK_beta = np.asarray(IRK_beta, dtype=np.float64)        # b [1, q]

    def _bind4(self, x_0, u_0, x_1, u_1):
        """Stage set 0 = the t_0 snapshot through dt A, stage set 1 = the t_1 snapshot through -dt (b - A): the construction
        of oracle/disc.py identification_sets"""
        arrs = [np.asarray(a, dtype=np.float64).reshape(-1) for a in (x_0, u_0, x_1, u_1)]
        key = tuple(a.tobytes() for a in arrs)
        if key != self._bound:
            self._engine.disc_set_stage(0, arrs[0], arrs[1], self.dt * self.IRK_alpha)
            self._engine.disc_set_stage(1, arrs[2], arrs[3], -self.dt * (self.IRK_beta - self.IRK_alpha))
            self._bound = key

    def U_0_model(self, x, customDummy=None):
        return self._engine.disc_predict(0, np.asarray(x, dtype=np.float64).reshape(-1))

    def U_1_model(self, x, customDummy=None):
        return self._engine.disc_predict(1, np.asarray(x, dtype=np.float64).reshape(-1))

    def loss(self, x_0, u_0, x_1, u_1):
        self._bind4(x_0, u_0, x_1, u_1)
        return self._engine.loss_grad(want_grad=False)[0]

    def grad(self, x_0, u_0, x_1, u_1):
        self._bind4(x_0, u_0, x_1, u_1)
        loss_value, flat, _ = self._engine.loss_grad()
        return loss_value, self._split(flat)

    def createDummy(self, x):
        return np.ones([np.shape(x)[0], self.q])

    def fit(self, x_0, u_0, x_1, u_1):
        self.logger.log_train_start(self)
        self._bind4(x_0, u_0, x_1, u_1)
        # both optimiser loops are the base class's device-resident ones; _bind() must keep the four-array set
        self._bind = lambda X, u: None
        try:
            self.tf_optimization(x_0, u_0)
            self.nt_optimization(x_0, u_0)
        finally:
            del self._bind
        self.logger.log_train_end(self.tf_epochs, self._log_custom())

    def predict(self, x_star):
        return self.U_0_model(x_star), self.U_1_model(x_star)


def prep_data(N_0, N_1, q, t_0=0.2, t_1=0.8, noise=0.0, n_grid=512):
    """-> x_0 [N_0,1], u_0, x_1 [N_1,1], u_1, x_star, dt, q, IRK_alpha [q,q], IRK_beta [1,q].  Draws the snapshot points
    from numpy's global RNG (t_0 first), then the noise (in units of std(u))."""
    x, U0 = snapshot(t_0, n_grid)
    _, U1 = snapshot(t_1, n_grid)
    p0 = np.random.choice(n_grid, N_0, replace=False)
    x_0, u_0 = x[p0, :], U0[p0, :]
    u_0 = u_0 + noise * np.std(u_0) * np.random.randn(*u_0.shape)
    p1 = np.random.choice(n_grid, N_1, replace=False)
    x_1, u_1 = x[p1, :], U1[p1, :]
    u_1 = u_1 + noise * np.std(u_1) * np.random.randn(*u_1.shape)
    A, b, _ = gauss_legendre_butcher(q)
    return x_0, u_0, x_1, u_1, x, float(t_1) - float(t_0), q, A, b[None, :]


def relative_errors(found, truth=KDV_COEFFS, names=("a1", "d3")):
    return {n: abs(found[ADRD_NAMES.index(n)] - truth[ADRD_NAMES.index(n)]) / abs(truth[ADRD_NAMES.index(n)]) for n in names}


def run(hp):
    lb, ub = np.array([LB]), np.array([UB])
    x_0, u_0, x_1, u_1, x_star, dt, q, IRK_alpha, IRK_beta = prep_data(
        hp["N_0"], hp["N_1"], hp["q"], t_0=float(hp["t_0"]), t_1=float(hp["t_1"]), noise=float(hp.get("noise", 0.0)))
    hp["layers"][-1] = q

    logger = Logger(hp)
    pinn = KdVDiscreteIdentificationNN(hp, logger, dt, lb, ub, q, IRK_alpha, IRK_beta)
    learned = [n for n in hp["adr_trainable"] if KDV_COEFFS[ADRD_NAMES.index(n)] != 0.0]

    def error():          # mean relative error of the learned coefficients whose true value is not 0
        e = relative_errors(pinn.get_params(numpy=True), names=learned)
        return sum(e.values()) / max(len(e), 1)

    logger.set_error_fn(error)
    pinn.fit(x_0, u_0, x_1, u_1)

    found = pinn.get_params(numpy=True)
    if pinn.is_root:                 # under torchrun the discrete-time models are replicas; rank 0 reports
        print("identified coefficients (truth, relative error):")
        for k, n in enumerate(ADRD_NAMES):
            tag = "trained" if n in hp["adr_trainable"] else "frozen"
            rel = "%.3e" % (abs(found[k] - KDV_COEFFS[k]) / abs(KDV_COEFFS[k])) if KDV_COEFFS[k] != 0.0 else "-"
            print("  %-2s = % .8e   (% .8e, %s)  %s" % (n, found[k], KDV_COEFFS[k], rel, tag))
    return pinn


if __name__ == "__main__":
    pinn = run(hp)
