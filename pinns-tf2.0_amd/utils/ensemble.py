"""NeuralNetworkEnsemble: K Burgers PINNs trained side by side on one point set (several seeds, a learning-rate sweep,
repeated identification runs) by one engine ensemble (pinn_native.Ensemble, include/pinn_hip.h pinn_ens_*).

Scope: float64, kernel path 7 -- Burgers inference (pde "burgers") and identification ("burgers_ide"), 2-20-...-20-1 nets
with 4, 6 or 8 hidden layers, one GPU.  The members share the point sets, the PDE parameters and every hyperparameter
except the per-member overrides in `members`:
    seed, init_scale          the initial weights (member k's vector is exactly NeuralNetwork._initial_weights of hp
                              updated with member k's overrides)
    tf_lr, nt_lr, nt_epochs   Adam learning rate, L-BFGS learningRate and maxIter
fit() follows NeuralNetwork.fit's float64 schedule (Adam tf_epochs, then L-BFGS with the same lbfgs_begin arguments) with no
restart guard and no resampling; member k ends bit-identical to a NeuralNetwork of its own hp trained alone.
"""
import os
import sys

import numpy as np

sys.path.append(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from neuralnetwork import NeuralNetwork  # noqa: E402
from pinn_native import Ensemble  # noqa: E402

MEMBER_KEYS = ("seed", "init_scale", "tf_lr", "nt_lr", "nt_epochs")
_LINE = "{tag} = {epoch:6d}  elapsed = {total}  loss min = {lo:.4e}  median = {med:.4e}  max = {hi:.4e}  {custom}"


class NeuralNetworkEnsemble(object):
    engine_class = Ensemble            # (the host tests put a stub here)

    def __init__(self, hp, logger, ub, lb, members, pde="burgers"):
        if not members:
            raise ValueError("an ensemble needs at least one member")
        for m in members:
            bad = set(m) - set(MEMBER_KEYS)
            if bad:
                raise ValueError("per-member overrides are %s; got %s" % (", ".join(MEMBER_KEYS), sorted(bad)))
        if hp.get("dtype", "f64") not in ("f64", "float64"):
            raise ValueError("ensembles are float64 only")
        self.pde = pde
        self.layers = [int(v) for v in hp["layers"]]
        self.ub = np.asarray(ub, dtype=np.float64)
        self.lb = np.asarray(lb, dtype=np.float64)
        self.logger = logger
        self.member_hp = [dict(hp, **m) for m in members]
        self.n_members = len(members)
        self.tf_epochs = int(hp["tf_epochs"])
        self.tf_b1, self.tf_eps = hp["tf_b1"], 1e-7 if hp["tf_eps"] is None else hp["tf_eps"]   # (Keras default)
        self.nt_ncorr = hp["nt_ncorr"]
        self.tol_fun = 1.0 * np.finfo(float).eps                       # NeuralNetwork.nt_config.tolFun
        device = hp.get("device", os.environ.get("PINN_DEVICE", 0))
        self._engine = self.engine_class(self.layers, self.lb, self.ub, self.n_members, pde=pde, dtype="f64",
                                         device=int(device))
        self.initial_weights = self._member_weights()
        self._engine.set_weights(self.initial_weights)
        self.adam_losses = np.zeros((0, self.n_members))
        self.nt_log = [([], []) for _ in range(self.n_members)]       # per member: L-BFGS (iterations, losses)
        self.nt_done = np.zeros(self.n_members, dtype=np.int32)

    # member k's initial vector: NeuralNetwork's own rule for member k's hp.  A member with "seed" draws from its private
    # RandomState; every member without one gets what a NeuralNetwork built at this point would get from the process-wide
    # stream (the stream is rewound for each of them: "init_scale" members are the same draw, scaled), and the stream ends
    # as after one such model.
    def _initial_weights(self, hp):
        return NeuralNetwork._initial_weights(self, hp)

    def _member_weights(self):
        import neuralnetwork
        rs = neuralnetwork._init_stream()
        start = rs.get_state()
        out = []
        for h in self.member_hp:
            if "seed" not in h:
                rs.set_state(start)
            out.append(self._initial_weights(h))
        return np.stack(out)

    def _extra_params(self):
        return np.array([0.0, -6.0]) if self.pde == "burgers_ide" else np.zeros(0)   # ide_cont_burgers.py lambdas

    # ---- point sets -----------------------------------------------------------------------------------
    def set_collocation(self, X_f):
        self._engine.set_collocation(np.asarray(X_f, dtype=np.float64).reshape(-1, 2))

    def set_pde_params(self, nu):
        self._engine.set_pde_params(nu)

    # ---- training ---------------------------------------------------------------------------------------
    def _line(self, tag, epoch, losses, custom=""):
        lg = self.logger
        if lg is None or getattr(lg, "quiet", False):
            return
        losses = np.asarray(losses, dtype=np.float64)
        print(_LINE.format(tag=tag, epoch=int(epoch), total=lg.get_elapsed(), lo=np.min(losses),
                           med=np.median(losses), hi=np.max(losses), custom=custom))

    def fit(self, X_u, u):
        eng, K = self._engine, self.n_members
        freq = max(int(self.logger.frequency if self.logger is not None else 10), 1)
        eng.set_data(np.asarray(X_u, dtype=np.float64).reshape(-1, 2), np.asarray(u, dtype=np.float64).reshape(-1, 1))
        # Adam (NeuralNetwork.tf_optimization)
        eng.adam_init(np.array([h["tf_lr"] for h in self.member_hp], dtype=np.float64), self.tf_b1, 0.999, self.tf_eps)
        chunks, epoch = [], 0
        while epoch < self.tf_epochs:
            stop = min(self.tf_epochs, (epoch + freq - 1) // freq * freq + 1)
            losses = eng.adam_run(stop - epoch)
            chunks.append(losses)
            for i, row in enumerate(losses):
                if (epoch + i) % freq == 0:
                    self._line("tf_epoch", epoch + i, row)
            epoch = stop
        self.adam_losses = np.concatenate(chunks) if chunks else np.zeros((0, K))
        # L-BFGS (NeuralNetwork.nt_optimization with nt_guard = 0): same lbfgs_begin arguments, chunks of log_frequency
        max_iter = np.array([int(h["nt_epochs"]) for h in self.member_hp], dtype=np.int32)
        lr = np.array([h["nt_lr"] or 1 for h in self.member_hp], dtype=np.float64)
        self.nt_log = [([], []) for _ in range(K)]
        if np.any(max_iter > 0):
            eng.lbfgs_begin(max_iter, lr, self.nt_ncorr or 100, self.tol_fun or 1e-5, 1e-19, 0.0)
            done = np.where(max_iter > 0, 0, 1)
            while not np.all(done):
                iters, losses, done = eng.lbfgs_run(freq)
                last = []
                for k in range(K):
                    self.nt_log[k][0].extend(int(i) for i in iters[k])
                    self.nt_log[k][1].extend(float(v) for v in losses[k])
                    if len(losses[k]):
                        last.append(losses[k][-1])
                if last:
                    self._line("nt_epoch", max(max(it) if len(it) else 0 for it in iters), last,
                               "(%d of %d members running)" % (int(np.sum(done == 0)), K))
            self.nt_done = np.asarray(done, dtype=np.int32)
        self.nt_log = [(np.asarray(i, dtype=np.int64), np.asarray(v, dtype=np.float64)) for i, v in self.nt_log]
        bad = self.status()[1]
        for k in np.nonzero(bad)[0]:
            print("warning: member %d: the loss became non-finite at evaluation %d" % (k, bad[k]), file=sys.stderr)

    # ---- results ----------------------------------------------------------------------------------------
    def get_weights(self):
        """[K, P]"""
        return self._engine.get_weights()

    def predict(self, X_star):
        """[K, n, 1]"""
        return self._engine.predict(np.asarray(X_star, dtype=np.float64).reshape(-1, 2))

    def error_l2(self, X_star, reference):
        """[K]: each member's ||reference - model(X_star)||_2 / ||reference||_2, reduced on the device"""
        return self._engine.error_l2(np.asarray(X_star, dtype=np.float64).reshape(-1, 2), reference)

    def get_params(self, numpy=False):
        """identification: (lambda_1 [K], lambda_2 [K]) with lambda_2 = exp of the trained log value; inference: None"""
        if self.pde != "burgers_ide":
            return None
        w = self.get_weights()
        return w[:, -2].copy(), np.exp(w[:, -1])

    def status(self):
        """(evaluations [K], first non-finite evaluation [K], 0 = none)"""
        return self._engine.status()
