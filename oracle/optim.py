"""Oracle (test infrastructure): optimisers, numpy float64.

Reference being restated:
  Adam    utils/neuralnetwork.py:19-22 (hyper-parameters; epsilon=None -> Keras 1e-7),
          :105-116 (full-batch loop).  Update = TF-2.0 ResourceApplyAdam:
          alpha = lr*sqrt(1-b2^t)/(1-b1^t); m += (1-b1)(g-m); v += (1-b2)(g^2-v);
          theta -= alpha*m/(sqrt(v)+eps)        [SURVEY.md Appendix A.4]
  L-BFGS  utils/custom_lbfgs.py:39-236, statement by statement, including
          - first step t = min(1, 1/sum|g|), later t = learningRate (:159-163)
          - curvature pair accepted only if y.s > 1e-10 (:102)
          - no re-evaluation on the last iteration (:176), so the "model" ends at the last
            *evaluated* point while the returned x is one step further
          - log_fn is called after the break tests (:217-218)
"""
import numpy as np


class Adam(object):
    def __init__(self, lr, b1=0.9, b2=0.999, eps=None):
        self.lr, self.b1, self.b2 = lr, b1, b2
        self.eps = 1e-7 if eps is None else eps
        self.t = 0
        self.m = None
        self.v = None

    def step(self, w, g):
        if self.m is None:
            self.m = np.zeros_like(w)
            self.v = np.zeros_like(w)
        self.t += 1
        alpha = self.lr * np.sqrt(1.0 - self.b2 ** self.t) / (1.0 - self.b1 ** self.t)
        self.m += (1.0 - self.b1) * (g - self.m)
        self.v += (1.0 - self.b2) * (g * g - self.v)
        return w - alpha * self.m / (np.sqrt(self.v) + self.eps)


def lbfgs(opfunc, x, max_iter, lr, n_corr, tol_fun=np.finfo(float).eps, tol_x=1e-19,
          max_eval=None, log_fn=None, trace=None):
    """Returns dict(x=returned x, x_model=last evaluated x, f_hist, n_eval, logs, final_loss).

    trace: optional dict, filled in place with what decided the run (the return value does not change):
      reason  why it ended, in the engine's LbfgsState::done codes: 1 nIter == maxIter, 2 gtd > -tolX,
              3 maxEval, 4 tolFun, 5 step < tolX, 6 |f - f_old| < tolX, 7 initial tolFun (0: max_iter == 0)
      g0_abs  sum|g| at the start
      iters   one dict per iteration: n_iter; ys and kept (the curvature pair, None on iteration 1); gtd;
              g_abs = sum|g|, s_abs = sum|d t|, df = |f - f_old| after the evaluation (None where the
              iteration ended before that test)
      n_eval  evaluations, the initial one included
    """
    if trace is not None:
        trace.update(reason=0, g0_abs=None, iters=[], n_eval=0)
    if max_iter == 0:
        return None                                            # :43-44
    max_eval = max_eval or max_iter * 1.25                     # :50
    x = np.array(x, dtype=np.float64)
    f, g = opfunc(x)                                           # :65
    x_model = x.copy()
    f_hist = [f]
    n_eval = 1
    logs = []
    final_loss = None
    if trace is not None:
        trace.update(g0_abs=float(np.sum(np.abs(g))), n_eval=1)
    if np.sum(np.abs(g)) <= tol_fun:                           # :72-76
        if trace is not None:
            trace["reason"] = 7
        return dict(x=x, x_model=x_model, f_hist=f_hist, n_eval=n_eval, logs=logs,
                    final_loss=final_loss)
    n_iter = 0
    S, Y = [], []                                              # old_dirs (s), old_stps (y)
    Hdiag = 1.0
    d = t = g_old = f_old = None
    reason = 0
    while n_iter < max_iter:                                   # :81
        n_iter += 1
        rec = dict(n_iter=n_iter, ys=None, kept=None, gtd=None, g_abs=None, s_abs=None, df=None)
        if trace is not None:
            trace["iters"].append(rec)
        if n_iter == 1:                                        # :90-95
            d = -g
            S, Y = [], []
            Hdiag = 1.0
        else:
            y = g - g_old                                      # :98-100
            s = d * t
            ys = np.sum(y * s)
            rec.update(ys=float(ys), kept=bool(ys > 1e-10))
            if ys > 1e-10:                                     # :102-114
                if len(S) == n_corr:
                    del S[0]
                    del Y[0]
                S.append(s)
                Y.append(y)
                Hdiag = ys / np.sum(y * y)
            k = len(S)
            ro = [1.0 / np.sum(Y[i] * S[i]) for i in range(k)]  # :121-123
            al = [0.0] * k
            q = -g
            for i in range(k - 1, -1, -1):                     # :130-133
                al[i] = np.sum(S[i] * q) * ro[i]
                q = q - al[i] * Y[i]
            r = q * Hdiag                                      # :136
            for i in range(k):                                 # :137-139
                be_i = np.sum(Y[i] * r) * ro[i]
                r = r + (al[i] - be_i) * S[i]
            d = r
        g_old = g
        f_old = f
        gtd = np.sum(g * d)                                    # :151
        rec["gtd"] = float(gtd)
        if gtd > -tol_x:                                       # :154-156
            reason = 2
            break
        if n_iter == 1:                                        # :159-163
            t = min(1.0, 1.0 / np.sum(np.abs(g)))
        else:
            t = lr
        x = x + t * d                                          # :174
        ls_eval = 0
        if n_iter != max_iter:                                 # :176-182
            f, g = opfunc(x)
            x_model = x.copy()
            ls_eval = 1
            f_hist.append(f)
        n_eval += ls_eval
        if n_iter == max_iter:                                 # :192
            reason = 1
            break
        if n_eval >= max_eval:                                 # :195
            reason = 3
            break
        rec["g_abs"] = float(np.sum(np.abs(g)))
        if np.sum(np.abs(g)) <= tol_fun:                       # :200-203
            reason = 4
            break
        rec["s_abs"] = float(np.sum(np.abs(d * t)))
        if np.sum(np.abs(d * t)) <= tol_x:                     # :206-209
            reason = 5
            break
        rec["df"] = float(abs(f - f_old))
        if abs(f - f_old) < tol_x:                             # :212-215
            reason = 6
            break
        logs.append((n_iter, f))                               # :217-218
        if log_fn is not None:
            log_fn(n_iter, f, True)
        if n_iter == max_iter - 1:                             # :223-224
            final_loss = f
    if trace is not None:
        trace.update(reason=reason, n_eval=n_eval)
    return dict(x=x, x_model=x_model, f_hist=f_hist, n_eval=n_eval, logs=logs,
                final_loss=final_loss)
