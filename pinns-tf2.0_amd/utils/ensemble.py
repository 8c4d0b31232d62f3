"""NeuralNetworkEnsemble: K Burgers PINNs trained side by side (several seeds, a learning-rate or viscosity sweep, bagged
point sets, repeated identification runs) by one engine ensemble (pinn_native.Ensemble, include/pinn_hip.h pinn_ens_* /
pinn_ensk_*), or K PINNs of the "adr" kind, each with its own six coefficients (pinn_native.AdrEnsemble,
pinn_adr_ens_create): Allen-Cahn over interface widths, Fisher-KPP over rho and D.

Scope: float64, kernel path 7 -- Burgers inference (pde "burgers"), identification ("burgers_ide") and the
advection-diffusion-reaction kind with fixed coefficients ("adr"), 2-20-...-20-1 nets with 4, 6 or 8 hidden layers, one GPU.
The members share every hyperparameter except the per-member overrides in `members`:
    seed, init_scale          the initial weights (member k's vector is exactly NeuralNetwork._initial_weights of hp
                              updated with member k's overrides)
    tf_lr, nt_lr, nt_epochs   Adam learning rate, L-BFGS learningRate and maxIter
    nu                        the viscosity (overrides set_pde_params for that member; identification: unused; not "adr")
    adr                       "adr" only: the member's six coefficients a0, a1, nu, r1, r2, r3 (overrides set_pde_params)
    resample_seed             the member's collocation redraws (hp["resample_every"]): seed resample_seed + epoch
The point sets are shared, or one per member: set_collocation(X_f) and fit(X_u, u) take [n, 2] / [n, 1] arrays for
all members or [K, n, 2] / [K, n, 1] arrays, member k's at index k (every member with the same n); so does
_set_boundary(X_lb, X_ub), the periodic pairs of the "adr" kind.
fit() follows NeuralNetwork.fit's float64 schedule (Adam tf_epochs with NeuralNetwork.tf_optimization's chunks and
redraws, then L-BFGS with the same lbfgs_begin arguments) with no restart guard; member k ends bit-identical to a
NeuralNetwork of its own hp trained alone on its own points.
"""
import os
import sys

import numpy as np

sys.path.append(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from neuralnetwork import NeuralNetwork  # noqa: E402
from pinn_native import AdrEnsemble, Ensemble  # noqa: E402

MEMBER_KEYS = ("seed", "init_scale", "tf_lr", "nt_lr", "nt_epochs", "nu", "adr", "resample_seed")
ADR_DEFAULT = (0.0, 1.0, 0.01 / np.pi, 0.0, 0.0, 0.0)      # a new adr context's coefficients (Burgers)
_LINE = "{tag} = {epoch:6d}  elapsed = {total}  loss min = {lo:.4e}  median = {med:.4e}  max = {hi:.4e}  {custom}"


class NeuralNetworkEnsemble(object):
    engine_class = Ensemble            # (the host tests put a stub here; pde "adr" builds adr_engine_class unless one stands here)
    adr_engine_class = AdrEnsemble

    def __init__(self, hp, logger, ub, lb, members, pde="burgers"):
        if not members:
            raise ValueError("an ensemble needs at least one member")
        for m in members:
            bad = set(m) - set(MEMBER_KEYS)
            if bad:
                raise ValueError("per-member overrides are %s; got %s" % (", ".join(MEMBER_KEYS), sorted(bad)))
        for m in members:
            if "nu" in m and pde == "adr":
                raise ValueError('the member key "nu" is the Burgers kinds\'; an "adr" member takes "adr": six coefficients')
            if "adr" in m and pde != "adr":
                raise ValueError('the member key "adr" is for pde "adr"; the %s kind takes "nu"' % pde)
            if "adr" in m and np.asarray(m["adr"], dtype=np.float64).shape != (6,):
                raise ValueError('the member key "adr" takes six numbers (a0, a1, nu, r1, r2, r3), got %r' % (m["adr"],))
        if hp.get("dtype", "f64") not in ("f64", "float64"):
            raise ValueError("ensembles are float64 only")
        if hp.get("resample", "lhs") != "lhs":
            raise ValueError('hp["resample"]: ensembles redraw uniform Latin hypercubes only ("lhs"); per-member adaptive '
                             'sampling ("rad") is not supported')
        if hp.get("sa_weights", False):
            raise ValueError('hp["sa_weights"]: self-adaptive point weights are for single models (NeuralNetwork), not '
                             'ensembles')
        if hp.get("point_weights", False):
            raise ValueError('hp["point_weights"]: point weights are for single "adr" models (NeuralNetwork), not ensembles')
        self.pde = pde
        self.layers = [int(v) for v in hp["layers"]]
        self.ub = np.asarray(ub, dtype=np.float64)
        self.lb = np.asarray(lb, dtype=np.float64)
        self.logger = logger
        self.members = [dict(m) for m in members]
        self.member_hp = [dict(hp, **m) for m in members]
        self.n_members = len(members)
        self.tf_epochs = int(hp["tf_epochs"])
        self.tf_b1, self.tf_eps = hp["tf_b1"], 1e-7 if hp["tf_eps"] is None else hp["tf_eps"]   # (Keras default)
        self.nt_ncorr = hp["nt_ncorr"]
        self.tol_fun = 1.0 * np.finfo(float).eps                       # NeuralNetwork.nt_config.tolFun
        # device-side redraws of the collocation set (NeuralNetwork.tf_optimization): member k's seeds resample_seed_k + epoch
        self.resample_every = int(hp.get("resample_every", 0))
        self.resample_seeds = np.array([int(h.get("resample_seed", 1234)) for h in self.member_hp], dtype=np.int64)
        self._n_design = 0
        device = hp.get("device", os.environ.get("PINN_DEVICE", 0))
        if pde == "adr" and self.engine_class is Ensemble:
            self._engine = self.adr_engine_class(self.layers, self.lb, self.ub, self.n_members, device=int(device))
        else:
            self._engine = self.engine_class(self.layers, self.lb, self.ub, self.n_members, pde=pde, dtype="f64",
                                             device=int(device))
        self.initial_weights = self._member_weights()
        self._engine.set_weights(self.initial_weights)
        if any("nu" in m for m in members):      # per-member viscosities (a later set_pde_params keeps them)
            self.set_pde_params(float(hp.get("nu", 0.0)))
        if any("adr" in m for m in members):     # per-member coefficients (a later set_pde_params keeps them)
            self.set_pde_params(hp.get("adr", ADR_DEFAULT))
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
        """X_f [n, 2] for every member, or [K, n, 2]: member k's own set"""
        X_f = np.asarray(X_f, dtype=np.float64)
        X_f = X_f if X_f.ndim == 3 else X_f.reshape(-1, 2)
        self._engine.set_collocation(X_f)
        self._n_design = X_f.shape[-2]

    def _set_boundary(self, X_lb, X_ub):
        """periodic pairs of the "adr" kind: X_lb, X_ub [n, 2] for every member, or [K, n, 2]: member k's own pairs"""
        if self.pde != "adr":
            raise ValueError('_set_boundary: periodic pairs are for pde "adr"; the %s ensemble has none' % self.pde)
        X_lb, X_ub = np.asarray(X_lb, dtype=np.float64), np.asarray(X_ub, dtype=np.float64)
        if X_lb.ndim != 3:
            X_lb, X_ub = X_lb.reshape(-1, 2), X_ub.reshape(-1, 2)
        self._engine.set_boundary(X_lb, X_ub)

    def set_pde_params(self, nu):
        """nu for every member (a member's "nu" override wins), or nu [K]; pde "adr": six coefficients for every member (a
        member's "adr" override wins), or [K, 6]"""
        if self.pde == "adr":
            p = np.asarray(nu, dtype=np.float64)
            if p.shape != (6,) and p.shape != (self.n_members, 6):
                raise ValueError("set_pde_params: six coefficients or [K=%d, 6], got %s" % (self.n_members, p.shape))
            rows = np.broadcast_to(p, (self.n_members, 6)).copy()
            for k, m in enumerate(self.members):
                if "adr" in m:
                    rows[k] = np.asarray(m["adr"], dtype=np.float64)
            if p.ndim == 1 and not any("adr" in m for m in self.members):
                self._engine.set_pde_params(p.copy())
            else:
                self._engine.set_pde_params(rows)
            return
        nu_k = np.broadcast_to(np.asarray(nu, dtype=np.float64), (self.n_members,)).copy()
        for k, m in enumerate(self.members):
            if "nu" in m:
                nu_k[k] = m["nu"]
        if np.ndim(nu) == 0 and not any("nu" in m for m in self.members):
            self._engine.set_pde_params(float(nu))
        else:
            self._engine.set_pde_params(nu_k)

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
        X_u, u = np.asarray(X_u, dtype=np.float64), np.asarray(u, dtype=np.float64)
        if X_u.ndim == 3:                                              # one data set per member
            eng.set_data(X_u, u.reshape(K, X_u.shape[1], 1))
        else:
            eng.set_data(X_u.reshape(-1, 2), u.reshape(-1, 1))
        # Adam (NeuralNetwork.tf_optimization): the same chunks and redraws, all members' redraws in one launch
        eng.adam_init(np.array([h["tf_lr"] for h in self.member_hp], dtype=np.float64), self.tf_b1, 0.999, self.tf_eps)
        chunks, epoch = [], 0
        every = self.resample_every if self._n_design > 0 else 0
        while epoch < self.tf_epochs:
            if every and epoch > 0 and epoch % every == 0:
                eng.lhs_collocation(self._n_design, self.resample_seeds + epoch)
            stop = min(self.tf_epochs, (epoch + freq - 1) // freq * freq + 1)
            if every:
                stop = min(stop, (epoch // every + 1) * every)
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
