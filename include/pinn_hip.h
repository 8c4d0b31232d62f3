/*
 * pinn_hip.h -- C ABI of libpinn_hip.so, the MI355X (gfx950) PINN training engine.
 *
 * The reference (pierremtb/PINNs-TF2.0) has no FFI/plugin boundary: its hot path is
 * Python calling TensorFlow eager ops.  This ABI therefore sits *under* the reference's
 * Python surface; each entry point below replaces the TensorFlow work done by the cited
 * reference method, and `pinns-tf2.0_amd/utils/neuralnetwork.py` (same class/method
 * names as the reference) is its only caller.  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *   - every function returns 0 on success, a negative PINN_E* code on failure;
 *     pinn_last_error() returns a thread-local message for the last failure.
 *   - host pointers are borrowed for the duration of the call only; host interchange
 *     dtype is always float64 (the reference's dtype, utils/neuralnetwork.py:24-26),
 *     whatever the kernel compute dtype.
 *   - the flat weight vector uses the reference layout (utils/neuralnetwork.py:68-89):
 *     per Dense layer W.ravel() (row-major [fan_in, fan_out]) then b; the identification
 *     problem appends lambda_1, lambda_2 (1d-burgers/ide_cont_burgers.py:98-107).
 *   - a pinn_ctx is bound to one device and one stream and is not thread-safe.
 *   - no torch / Python types anywhere in the signatures.
 */
#ifndef PINN_HIP_H
#define PINN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pinn_ctx pinn_ctx;

enum {
  PINN_PDE_BURGERS = 0,     /* 1d-burgers/inf_cont_burgers.py:65-90   f = u_t + u u_x - nu u_xx            */
  PINN_PDE_BURGERS_IDE = 1, /* 1d-burgers/ide_cont_burgers.py:56-85   f = u_t + l1 u u_x - exp(l2) u_xx    */
  PINN_PDE_SCHRODINGER = 2, /* 1dcomplex-schrodinger/inf_cont_schrodinger.py:79-129                        */
  /* discrete-time (implicit Runge-Kutta) models: 1 input (x), q or q+1 outputs, see pinn_disc_set_stage */
  PINN_PDE_BURGERS_DISC = 3,     /* 1d-burgers/inf_disc_burgers.py:57-95   N = U U_x - nu U_xx             */
  PINN_PDE_BURGERS_DISC_IDE = 4, /* 1d-burgers/ide_disc_burgers.py:81-115  N = l1 U U_x - exp(l2) U_xx     */
  /* advection-diffusion-reaction, one output u(x, t), six fixed coefficients p = [a0, a1, nu, r1, r2, r3]
   * (pinn_set_pde_params):  f = u_t + (a0 + a1 u) u_x - nu u_xx + r1 u + r2 u^2 + r3 u^3.
   * Burgers [0, 1, nu, 0, 0, 0], Allen-Cahn [0, 0, 1e-4, -5, 0, 5], Fisher-KPP [0, 0, D, -rho, rho, 0].
   * loss = mean_f f^2 + mean_u (u - u*)^2 + mean_b [(u(lo) - u(hi))^2 + (u_x(lo) - u_x(hi))^2]; any set but the
   * collocation set may be empty.  Kernel paths 0 (any shape, float32 / float64) and 7 (float64, width 20, 4 / 6 / 8
   * hidden layers: the default there); PINN_EUNSUPPORTED for the other paths, self-adaptive weights and ensembles.
   * (Additive: one enum value, no new entry point; the ABI version stays 6.) */
  PINN_PDE_ADR = 5,
  /* the same equation and loss with TRAINABLE coefficients (identification from data).  The weight vector is
   * [net | a0, a1, log nu, r1, r2, r3] (pinn_num_params = net + 6, always all six, in this order; nu = exp(log nu) stays
   * positive); pinn_get_weights / pinn_set_weights carry the tail as PINN_PDE_BURGERS_IDE carries its two lambdas.
   * pinn_set_pde_params takes the six RAW values (nu > 0) and writes the tail, pinn_get_pde_params returns them;
   * pinn_set_pde_trainable chooses which are trained (default: none).  The gradient entry of a frozen coefficient is
   * exactly 0.0, so Adam and L-BFGS leave its value bit-identical.  The residual is taken on the collocation set (hand the
   * data points over as collocation points for the usual identification loss).  Kernel paths 0 and 7 as PINN_PDE_ADR;
   * PINN_EUNSUPPORTED for the other paths, self-adaptive weights, ensembles and communicators.
   * (Additive: one enum value, two entry points; the ABI version stays 6.) */
  PINN_PDE_ADR_IDE = 6,
  /* the discrete-time model of the adr operator: everything PINN_PDE_BURGERS_DISC is (layers[0] == 1, stage sets 0 and 1
   * through pinn_disc_set_stage, a SUM of squares, pinn_predict / pinn_disc_predict, both optimisers), with
   *     N(U) = (a0 + a1 U) U_x - nu U_xx + r1 U + r2 U^2 + r3 U^3
   * on the first q outputs.  The six coefficients are those of PINN_PDE_ADR, set and read the same way
   * (pinn_set_pde_params with n = 6; a new context holds Burgers', [0, 1, 0.01 / pi, 0, 0, 0]); they are fixed, not
   * trained.  The one kind with periodic pairs, pinn_disc_set_periodic.  Every call that refuses the discrete-time kinds
   * 3 and 4 refuses this one with the same code.  (Additive: one enum value, one entry point; the ABI version stays 6.) */
  PINN_PDE_ADR_DISC = 7,
  /* PINN_PDE_ADR_DISC with the six coefficients trained alongside the net (two snapshots joined by one Runge-Kutta step,
   * the discrete-time identification of 1d-burgers/ide_disc_burgers.py for the whole family): the weight vector is
   *     [net weights | a0, a1, log nu, r1, r2, r3]        n_theta = n_net + 6, nu = exp(log nu)
   * with PINN_PDE_ADR_IDE's semantics: pinn_set_pde_trainable chooses the trained subset (a new context trains none and
   * holds Burgers'), a frozen coefficient's gradient entry is exactly 0.0 and its value survives both optimisers bit for
   * bit; pinn_set_pde_params (n = 6, raw, nu > 0) writes the tail, pinn_get_pde_params reads it.  Either stage set may carry
   * a table, periodic pairs are allowed (pinn_disc_set_periodic); pairs and sets without a table add nothing to the six
   * gradient entries.  Every call that refuses kinds 3, 4 and 7 refuses this one with the same code.  (Additive: one enum
   * value, no entry point; the ABI version stays 6.) */
  PINN_PDE_ADR_DISC_IDE = 8,
  /* PINN_PDE_ADR_DISC_IDE with a dispersion term (Korteweg-de Vries u_t + a1 u u_x + d3 u_xxx = 0, the linear dispersive
   * equation, KdV-Burgers):
   *     N(U) = (a0 + a1 U) U_x - nu U_xx + d3 U_xxx + r1 U + r2 U^2 + r3 U^3
   * on the first q outputs; the weight vector is
   *     [net weights | a0, a1, log nu, r1, r2, r3, d3]    n_theta = n_net + 7, d3 raw (its sign is free)
   * Everything kind 8 has: either stage set may carry a table, periodic pairs at order 0 or 1, pinn_predict /
   * pinn_disc_predict, both optimisers, pinn_set_pde_trainable (mask 0..127, bit 6 = d3; a new context trains none and
   * holds [0, 1, 0.01 / pi, 0, 0, 0, 0]), a frozen coefficient frozen bit for bit -- so the inference model is this kind
   * with nothing trained.  pinn_set_pde_params / pinn_get_pde_params carry 7 raw values, and nu = 0 is allowed: the
   * kernels then compute without the diffusion term, the nu slot of the tail holds 0.0, is not read and has gradient
   * entry exactly 0.0, and the nu bit cannot be trained (PINN_EINVAL from whichever of the two calls comes second, nothing
   * changed) until pinn_set_pde_params gives nu > 0 again.  pinn_set_weights never touches that flag: to restore a
   * checkpoint, set the params first, then the weights.  Hidden width above 64 is PINN_EUNSUPPORTED at create in both
   * dtypes (four Taylor channels fill the LDS).  Every call that refuses kinds 3, 4, 7 and 8 refuses this one with the
   * same code.  (Additive: one enum value, no entry point; the ABI version stays 6.) */
  PINN_PDE_ADRD_DISC = 9,
  /* the adr equation with a coefficient on u_t and a second time derivative, eight run-time coefficients
   * p = [a0, a1, nu, r1, r2, r3, b, kappa] (pinn_set_pde_params / pinn_get_pde_params with n = 8, all finite, any sign):
   *     f = b u_t + (a0 + a1 u) u_x - nu (u_xx + kappa u_tt) + r1 u + r2 u^2 + r3 u^3 - s(x, t)
   * u_xx + kappa u_tt travels through the net as ONE Taylor channel (L a = d1 L z + d2 (z_x^2 + kappa z_t^2) through a tanh),
   * so the sweeps carry four channels as PINN_PDE_ADR's do.  b = 1, kappa = 0 is PINN_PDE_ADR (the same bits); b = 0,
   * nu = c^2, kappa = -1 / c^2 the wave equation u_tt = c^2 u_xx (b: a telegraph damping; r1..r3: Klein-Gordon); with the
   * second input read as y, b = 0, nu = 1, kappa = 1 is Poisson's -Laplace u = s and r1 = -k^2 Helmholtz'.  A new context
   * holds [0, 1, 0.01 / pi, 0, 0, 0, 1, 0], which is Burgers.  Point classes: collocation points with an optional source
   * (pinn_set_source), data points, periodic pairs on u and u_x (pinn_set_boundary), and three-term wall points
   * (pinn_set_robin3; pinn_set_robin means gamma = 0).  Loss, terms and gradient row as PINN_PDE_ADR with Robin points.
   * Kernel path 7 for float64 2-20-...-20-1 nets with 4, 6 or 8 hidden layers (k_adr2_20d), path 0 otherwise, in float32 and
   * float64 (every other path: PINN_EUNSUPPORTED from pinn_set_kernel_path).  pinn_residual,
   * pinn_residual_at (N[u] without s), pinn_robin_residual, LHS redraws, both optimisers, tickets, snapshots, pinn_predict
   * and pinn_error_l2 as for PINN_PDE_ADR.  PINN_EUNSUPPORTED, before any device work and the context unchanged: point
   * weights, pinn_set_pde_trainable, pinn_set_coef_fields, pinn_rad_collocation, ensembles, communicators.
   * (Additive: one enum value and pinn_set_robin3; the ABI version stays 6.) */
  PINN_PDE_ADR2 = 10
};
enum { PINN_F32 = 0, PINN_F64 = 1 };
enum {
  PINN_OK = 0, PINN_EINVAL = -1, PINN_EHIP = -2, PINN_ESTATE = -3, PINN_ECOMM = -4,
  PINN_EUNSUPPORTED = -5
};

/* diagnostics */
const char* pinn_last_error(void);
int pinn_abi_version(void);   /* 2: + discrete-time models, device LHS, mailbox all-reduce, kernel paths 3..6; 3: + pinn_residual_at;
                                 4: + pinn_error_l2, pinn_get_status; 5: + pinn_runtime_versions, pinn_debug_t16_deal;
                                 6: + pinn_adam_enqueue / _collect, pinn_lbfgs_enqueue / _collect,
                                    pinn_weights_snapshot / _restore */
int pinn_device_count(int* n);
/* HIP runtime / driver (hipRuntimeGetVersion, hipDriverGetVersion) and RCCL (ncclGetVersion) this process bound; any
 * pointer may be NULL.  No device is touched. */
int pinn_runtime_versions(int* hip_runtime, int* hip_driver, int* rccl);
/* name[0..cap) <- hipDeviceProp_t.gcnArchName etc. for Logger's banner (utils/logger.py:13-15) */
int pinn_device_info(int device, char* name, int cap, int* n_cu, int64_t* hbm_bytes);

/* NeuralNetwork.__init__ (utils/neuralnetwork.py:8-47): layers = hp["layers"], lb/ub = the
 * Lambda normalisation bounds.  dtype = kernel arithmetic type. */
int pinn_create(pinn_ctx** out, const int* layers, int n_layers, const double* lb,
                const double* ub, int pde_kind, int dtype, int device);
int pinn_destroy(pinn_ctx* c);
int pinn_num_params(pinn_ctx* c, int64_t* n);       /* incl. lambda_1, lambda_2 for IDE */

/* Point sets.  *_total are the GLOBAL set sizes used as the mean() denominators, so that a
 * rank holding a shard (n < n_total) produces partial sums that add up across ranks.
 *   collocation: self.x_f, self.t_f      (inf_cont_burgers.py:55-56, inf_cont_schrodinger.py:56-57)
 *   data:        fit(X_u, u) arguments   (utils/neuralnetwork.py:138-143); targets [n, n_out];
 *                for PINN_PDE_BURGERS_IDE these points also carry the residual
 *                (ide_cont_burgers.py:88-91) and no collocation set is used.
 *   boundary:    X_lb, X_ub              (inf_cont_schrodinger.py:50-53): periodic pairs, row i of X_lb with row i of
 *                X_ub; PINN_PDE_SCHRODINGER (h and h_x of both outputs) and PINN_PDE_ADR (u and u_x). */
int pinn_set_collocation(pinn_ctx* c, const double* X_f, int64_t n, int64_t n_total);
int pinn_set_data(pinn_ctx* c, const double* X_u, const double* u, int64_t n, int64_t n_total);
/* Collocation points drawn on the device instead of handed over: points [first, first + count) of an
 * n_design-point Latin hypercube over [lb, ub] -- the role of `lb + (ub - lb) * lhs(2, N_f)`
 * (1d-burgers/burgersutil.py:122), same kind of design, counter-based stream (csrc/kernels_sampling.h), so ranks
 * can build disjoint shards of one design and a re-draw with a new seed is a single launch (no reallocation when
 * count is unchanged).  The mean() denominator becomes n_design.  pinn_get_collocation reads the current set
 * back, [n][2] float64 (also valid after pinn_set_collocation). */
int pinn_lhs_collocation(pinn_ctx* c, int64_t n_design, int64_t first, int64_t count, uint64_t seed);
int pinn_get_collocation(pinn_ctx* c, double* X, int64_t n);
/* Residual-based adaptive collocation (RAD, Wu et al. 2023: p(x) ~ |f(x)|^k / mean|f|^k + c_add), drawn on the device
 * (csrc/kernels_rad.h).  The pool is the n_pool-point design pinn_lhs_collocation(n_pool, seed) would draw, its residuals
 * are what pinn_residual_at returns at the current weights (stream order), and slots [first, first + count) of an
 * n_design-sample set are drawn from it WITH replacement (a set may hold a pool point more than once).  The weights are
 * quantised to integers, so every rank of a data-parallel job builds the same CDF and draws its own slice of one set
 * without communication.  pde 0, 2 and 5, float32 and float64; PINN_EUNSUPPORTED for identification and discrete-time
 * models, PINN_EINVAL for bad geometry, n_pool outside 1..2^24, k outside 1..4 or c_add outside [0, 64] -- both before
 * any device work, the set unchanged.  With the set assembled and count unchanged the call only enqueues work.  The mean()
 * denominator becomes n_design; the points survive pinn_set_data / pinn_set_boundary and are replaced by
 * pinn_set_collocation, pinn_lhs_collocation or the next adaptive draw.  (Additive: the ABI version stays 6.) */
int pinn_rad_collocation(pinn_ctx* c, int64_t n_design, int64_t first, int64_t count, int64_t n_pool, uint64_t seed,
                         int k, double c_add);
int pinn_set_boundary(pinn_ctx* c, const double* X_lb, const double* X_ub, int64_t n,
                      int64_t n_total);
/* Discrete-time models (pde_kind 3, 4, 7; layers[0] == 1, lb/ub hold one value each).  A stage set contributes
 *     sum_{p,j} ( U[p][j] + sum_k N(U)[p][k] M[j][k] - target[p] )^2        (a SUM, inf_disc_burgers.py:92-95)
 * to the loss, N acting on the first q outputs.  M is [n_out][q] row-major and already carries the step size
 * (dt * IRK_weights for U_0_model, inf_disc_burgers.py:89; dt * IRK_alpha and -dt * (IRK_beta - IRK_alpha) for
 * ide_disc_burgers.py:92,108); M == NULL: no IRK term, the set penalises U itself (the walls x_1,
 * inf_disc_burgers.py:93-95).  target is [n] (broadcast over the outputs like the reference's [n,1] tensor).
 * set is 0 or 1; its loss is reported in terms[set].  n == 0 removes the set. */
int pinn_disc_set_stage(pinn_ctx* c, int set, const double* x, const double* target, int64_t n,
                        const double* M, int q);
/* U_0_model / U_1_model at arbitrary points with the table of `set` (ide_disc_burgers.py:188-193):
 * out [n][n_out] = U + N(U) M^T.  pinn_predict returns the plain network outputs U [n][n_out]. */
int pinn_disc_predict(pinn_ctx* c, int set, const double* x, int64_t n, double* out);
/* Periodic pairs of PINN_PDE_ADR_DISC, PINN_PDE_ADR_DISC_IDE and PINN_PDE_ADRD_DISC: n pairs, x_lb[i] with x_ub[i] (each [n]).  They add
 *     sum_{i<n} sum_{j<n_out} (U_j(x_lb[i]) - U_j(x_ub[i]))^2   [+ (U_x,j(x_lb[i]) - U_x,j(x_ub[i]))^2 when order == 1]
 * to the loss -- over ALL outputs, the stages and the solution at t_1 -- reported in terms[2] (terms[0] and terms[1] stay the
 * two stage sets).  A third slot beside stage sets 0 and 1: any subset of the three may be present, at least one must be at
 * the next evaluation.  n == 0 removes the pairs.  Refusals, the context unchanged: PINN_EUNSUPPORTED for any kind but
 * those two; PINN_EINVAL for order outside {0, 1}, a non-finite point, n outside 0..2^24.  (Additive: the ABI
 * version stays 6.) */
int pinn_disc_set_periodic(pinn_ctx* c, const double* x_lb, const double* x_ub, int64_t n, int order);

/* get_params (inf_cont_burgers.py:92): p[0] = nu for PINN_PDE_BURGERS and PINN_PDE_BURGERS_DISC.
 * PINN_PDE_ADR: n must be 6, p = [a0, a1, nu, r1, r2, r3], all finite; otherwise PINN_EINVAL and the context keeps the
 * coefficients it had (a new context holds Burgers', [0, 1, 0.01 / pi, 0, 0, 0]).  PINN_PDE_ADR_DISC: the same.
 * PINN_PDE_ADR_IDE: n must be 6, RAW p = [a0, a1, nu, r1, r2, r3], all finite and nu > 0 (otherwise PINN_EINVAL, nothing
 * changed): written to the tail of the weight vector, log nu in the nu slot.  PINN_PDE_ADR_DISC_IDE: the same.
 * PINN_PDE_ADRD_DISC: n must be 7, RAW p = [a0, a1, nu, r1, r2, r3, d3], all finite and nu >= 0 (nu == 0: see the kind);
 * PINN_EINVAL for nu == 0 while the nu bit is trainable. */
int pinn_set_pde_params(pinn_ctx* c, const double* p, int n);
/* the current values: n = 6 raw coefficients for PINN_PDE_ADR, PINN_PDE_ADR_DISC, PINN_PDE_ADR_IDE and
 * PINN_PDE_ADR_DISC_IDE (the last two: nu as exp of the stored log nu, what training has made of them), n = 7 for
 * PINN_PDE_ADRD_DISC (nu = 0 while its flag is up), n = 1 (nu) for every other kind */
int pinn_get_pde_params(pinn_ctx* c, double* p, int n);
/* PINN_PDE_ADR_IDE and PINN_PDE_ADR_DISC_IDE: bit k of mask set = coefficient k of (a0, a1, nu, r1, r2, r3) is trained; a new context trains none
 * (mask 0).  PINN_EINVAL for a mask outside 0..63, PINN_EUNSUPPORTED for every other kind; the context is unchanged then.
 * PINN_PDE_ADRD_DISC: seven names (.., d3), mask 0..127; PINN_EINVAL for the nu bit while nu == 0.
 * Takes effect at the next evaluation; a running Adam / L-BFGS state is not reset.  (Additive: the ABI version stays 6.) */
int pinn_set_pde_trainable(pinn_ctx* c, int mask);

/* get_weights / set_weights (utils/neuralnetwork.py:68-89) */
int pinn_set_weights(pinn_ctx* c, const double* w, int64_t n);
int pinn_get_weights(pinn_ctx* c, double* w, int64_t n);

/* NeuralNetwork.grad / get_loss_and_flat_grad (utils/neuralnetwork.py:55-59, 91-103) at the
 * current weights: forward, residual, loss, flat gradient (+ all-reduce when a communicator is
 * attached).  grad may be NULL.  terms (may be NULL) <- {mse_f, mse_data, mse_boundary}. */
int pinn_loss_grad(pinn_ctx* c, double* loss, double* grad, double* terms);

/* tf.keras.optimizers.Adam (utils/neuralnetwork.py:19-22) + tf_optimization loop (:105-116).
 * pinn_adam_run does n_steps x {loss_grad; apply_gradients}; losses[i] (may be NULL) is the
 * loss *before* update i, as tf_optimization_step returns it.  With losses == NULL the call
 * returns without synchronising the stream. */
int pinn_adam_init(pinn_ctx* c, double lr, double beta1, double beta2, double eps);
int pinn_adam_run(pinn_ctx* c, int n_steps, double* losses);
/* the same, returning the three loss parts of every step, terms3[i] = (residual, data, boundary) before update i:
 * what the reference's Schrodinger loss prints on every evaluation (inf_cont_schrodinger.py:128) */
int pinn_adam_run_terms(pinn_ctx* c, int n_steps, double* terms3);

/* custom_lbfgs.lbfgs (utils/custom_lbfgs.py:39-236) as driven by nt_optimization_steps
 * (utils/neuralnetwork.py:131-136), device-resident.  pinn_lbfgs_begin does the initial
 * evaluation (:65-76); pinn_lbfgs_run advances up to n_iters iterations.
 *   iters[i], losses[i]: the (nIter, f) pairs custom_lbfgs would have passed to log_fn (:217-218)
 *   n_logged: how many pairs were written;  done: 0 running, 1 maxIter reached, >1 break reason
 * The last-iteration quirk is reproduced: the model weights end at the last *evaluated* x.
 * pinn_lbfgs_begin only enqueues (it returns before the initial evaluation has run, except with the
 * mailbox exchange attached); pinn_lbfgs_run synchronises once, at its end, to read state and log.
 * iters / losses hold n_iters entries, and that is tight: the call runs with nothing in flight, so every entry of earlier
 * chunks has been handed out; the initial evaluation logs nothing; each of the call's iterations but the max_iter-th is
 * followed by one evaluation, which logs one entry or ends the run (n_logged <= min(n_iters, iterations left), one less
 * when the call issues the max_iter-th; a run that breaks nowhere logs exactly that). */
int pinn_lbfgs_begin(pinn_ctx* c, int max_iter, double lr, int n_corr, double tol_fun,
                     double tol_x, double max_eval);
int pinn_lbfgs_run(pinn_ctx* c, int n_iters, int* iters, double* losses, int* n_logged,
                   int* done);
/* The same two loops with the host one chunk behind the GPU (ABI v6) -- how NeuralNetwork.fit logs every
 * log_frequency-th epoch (utils/neuralnetwork.py:105-109, utils/logger.py:45-51) without idling the device at a log line:
 * ..._enqueue puts a chunk of steps into the stream, with asynchronous copies of its losses / log entries / optimiser state
 * into pinned buffers behind an event, and returns a ticket at once; ..._collect waits for THAT chunk only and hands its
 * results out, while the chunk enqueued after it is already running.  Up to 4 chunks may be in flight; tickets are
 * collected in the order they were issued; pinn_lbfgs_begin drops whatever is still in flight (a restart).  The kernels
 * launched are those of pinn_adam_run / pinn_lbfgs_run on the same chunk sizes, so the results are bit-identical.
 * pinn_lbfgs_collect: iters / losses hold `cap` entries (enough: the iterations enqueued since the last collect + 1).
 * An L-BFGS chunk enqueued after the run has ended (done != 0 seen one chunk late) changes nothing on the device. */
int pinn_adam_enqueue(pinn_ctx* c, int n_steps, int* ticket);
int pinn_adam_enqueue_terms(pinn_ctx* c, int n_steps, int* ticket);   /* as pinn_adam_run_terms: collect returns 3 n values */
int pinn_adam_collect(pinn_ctx* c, int ticket, double* losses);
int pinn_lbfgs_enqueue(pinn_ctx* c, int n_iters, int* ticket);
int pinn_lbfgs_collect(pinn_ctx* c, int ticket, int cap, int* iters, double* losses, int* n_logged, int* done);
/* Device-side copies of the flat weight vector taken / put back in stream order (slots 0..3; ABI v6): what a caller that
 * judges a chunk one chunk late (the restart guard of NeuralNetwork.nt_optimization; the reference has neither) returns to
 * without a host round trip.  pinn_weights_restore also refreshes the compute-dtype mirror, like pinn_set_weights. */
int pinn_weights_snapshot(pinn_ctx* c, int slot);
int pinn_weights_restore(pinn_ctx* c, int slot);
/* 0: one-workgroup kernel performing the two-loop recursion in the reference's operation order;
 * 1 (default, history <= 61): compact form -- all dot products of an iteration in one parallel
 * kernel, recursion on the Gram matrices.  Same mathematics; rounding differs at 1e-16. */
int pinn_lbfgs_set_mode(pinn_ctx* c, int mode);
/* x as custom_lbfgs returns it (:236) -- one step past the model weights */
int pinn_lbfgs_get_x(pinn_ctx* c, double* x, int64_t n);

/* self.model(X_star) (utils/neuralnetwork.py:151-153): out[N, n_out] */
int pinn_predict(pinn_ctx* c, const double* X, int64_t n, double* out);
/* The scripts' error metric on the device: err = ||ref - pred||_2 / ||ref||_2 with pred = self.model(X) at the
 * n points X [n][2] (1d-burgers/inf_cont_burgers.py:114-116 via utils/logger.py:56-60) -- forward sweep, fixed-order
 * float64 reduction, 24 bytes back.  kind 0: ref is [n][n_out], compared element-wise; kind 1: ref is [n] and is
 * compared with the modulus sqrt(sum_o pred_o^2) (the |h| of 1dcomplex-schrodinger/inf_cont_schrodinger.py:155-158).
 * X and ref are kept on the device: a repeated call with the same grid (and pinn_predict / pinn_residual_at on it)
 * uploads nothing. */
int pinn_error_l2(pinn_ctx* c, const double* X, const double* ref, int64_t n, int kind, double* err);
/* f_model() at the stored collocation points (inf_cont_burgers.py:65-90): f[n_f, n_out]
 * (IDE: at the data points) */
int pinn_residual(pinn_ctx* c, double* f, int64_t n);
/* f_model(X) at n caller-supplied points X [n][2] -> f [n][n_out]: what the identification script's predict
 * evaluates on X_star (1d-burgers/ide_cont_burgers.py:169-172) */
int pinn_residual_at(pinn_ctx* c, const double* X, int64_t n, double* f);

/* Failure detection (the reference has none: a NaN loss just propagates, utils/custom_lbfgs.py:154).
 * n_evals = loss+gradient evaluations since pinn_create; first_nonfinite_eval = 1-based number of the first one whose
 * reduced loss was NaN/Inf, 0 if none.  Recording only: optimiser trajectories are unchanged.  When non-zero,
 * pinn_last_error() carries a message too.  Either pointer may be NULL. */
int pinn_get_status(pinn_ctx* c, int64_t* n_evals, int64_t* first_nonfinite_eval);

/* Data-parallel: one process per GPU, RCCL all-reduce(SUM) of [grad | loss terms].
 * Rank 0 calls pinn_comm_unique_id and ships the 128 bytes to the other ranks by any
 * out-of-band channel; every rank then calls pinn_comm_init. */
int pinn_comm_unique_id(char* id128);
int pinn_comm_init(pinn_ctx* c, const char* id128, int n_ranks, int rank);
/* Low-latency alternative to the RCCL call for the [P+4] vector: every rank maps every peer's mailbox (hipIpc) and
 * the reduction kernel itself stores, signals, waits and adds in rank order (csrc/kernels_xgmi.h).  Protocol:
 *   1. every rank: pinn_comm_xgmi_export(n_ranks, rank, handle64)        -> 64-byte hipIpcMemHandle_t
 *   2. ship all handles to all ranks (out of band, like the RCCL id), rank-major [n_ranks][64]
 *   3. every rank: pinn_comm_xgmi_attach(handles, n_ranks, &mapped)      -> mapped = 1 if every peer mailbox is mapped
 *   4. only if mapped on ALL ranks (agreed out of band): pinn_comm_xgmi_selftest(&ok) everywhere -- a few exchange
 *      rounds on integer-valued vectors checked against the closed-form sum, bounded waits (5 s)
 *   5. if ok on ALL ranks: pinn_comm_set_mode(2) everywhere; otherwise stay on / return to RCCL (mode 1).
 * pinn_comm_get_mode: 0 no communicator, 1 RCCL, 2 mailboxes.  Works without an RCCL communicator too. */
int pinn_comm_xgmi_export(pinn_ctx* c, int n_ranks, int rank, char* handle64);
int pinn_comm_xgmi_attach(pinn_ctx* c, const char* handles, int n_handles, int* mapped_ok);
int pinn_comm_xgmi_selftest(pinn_ctx* c, int* ok);
/* Wall time per exchange of the [P+4] vector with the given implementation (1 RCCL: k_reduce_rows + ncclAllReduce,
 * 2 mailboxes: k_reduce_xgmi), measured on this node: what init_engine_comm uses to pick the faster one.
 * Collective: every rank must call it with the same mode and iteration count. */
int pinn_comm_benchmark(pinn_ctx* c, int mode, int iters, double* us_per_iter);
int pinn_comm_set_mode(pinn_ctx* c, int mode);
int pinn_comm_get_mode(pinn_ctx* c, int* mode);

/* Measurement: bracket launches of the dominant kernel (the loss+grad kernels) with hipEvents
 * on the engine's stream.  An event record costs ~5 us on the GPU timeline, so only one
 * evaluation out of `every` is sampled (at most max_evals samples).  pinn_timing_read drains
 * them into avg_ms[5]: [0] forward sweep, [1] forward+reverse sweeps (the loss+grad kernel),
 * [2] whole evaluation, [3] what an EMPTY event bracket reads on this stream (calibrated at
 * enable time; subtract it from [1..2] to compare with rocprofv3 kernel durations),
 * [4] = 1 when [0] is the exact begin-to-end duration of the single loss+grad kernel (the events
 * were attached to the launch itself, hipExtLaunchKernelGGL: kernel paths 1, 2 and 7) and needs no correction;
 * n = evaluations sampled. */
int pinn_timing_enable(pinn_ctx* c, int max_evals, int every);
int pinn_timing_read(pinn_ctx* c, double* avg_ms, int* n);
int pinn_sync(pinn_ctx* c);
/* which kernel family serves the loss+grad evaluation: 0 generic (one lane per point), 1 fused width-20 (HBM stash),
 * 2 fused 8x20 float32 (MFMA GEMVs, register stash), 3 wide MFMA sweeps (width 100, two outputs, float32),
 * 4 shape-generic MFMA sweeps (any width <= 128 / 64 in float64, any depth), 5 / 6 = 4's forward / reverse half
 * paired with the generic other half (tests), 7 fused 8x20 float64 (v_mfma_f64_4x4x4 GEMVs, register stash, no
 * inter-wave exchange), 8 fused float64 MFMA sweep for hidden widths 65..128 and 2-4 hidden layers (forward + reverse of a
 * 16-point group in one kernel, stash in registers: the Schrodinger net in the reference's arithmetic).  The engine
 * picks the fastest eligible family at pinn_create. */
int pinn_set_kernel_path(pinn_ctx* c, int path);
int pinn_get_kernel_path(pinn_ctx* c, int* path);
/* Launch plan of kernel path 7 in float64: *split = 1 when the next evaluation takes the split one-tile launch, 0 otherwise.
 * Split launch: beside the main workgroup of every 64-point tile, helper workgroups (one per pair of tiles) on compute units
 * the launch would leave idle recompute the tile's forward sweep and write the weight-gradient columns of the last hidden
 * and the output layer into the tile's gradient row; the main workgroup leaves those blocks out.  No workgroup waits for
 * another; loss, gradient and every later bit are those of the plain launch.  It serves a solo context of the Burgers kinds
 * (pde 0, 1) without self-adaptive weights when every tile has a workgroup of its own and
 * tiles + ceil(tiles / 2) <= compute units; ensembles, the adr kinds and every other path never split (the kernel path
 * reported stays 7).  Environment PINN_F64_SPLIT, read by pinn_create: "auto" (default), "0" = never, "1" = required --
 * an evaluation, and this call, fail with PINN_EUNSUPPORTED where the kernel exists for the context but the tile count does
 * not fit; any other value fails pinn_create.  Assembles the point sets if they changed.  (Additive: the ABI version stays 6.) */
int pinn_get_f64_split(pinn_ctx* c, int* split);
/* Profiling build (-DPINN_STAMPS) only: one evaluation with a per-wave s_memtime timeline of the
 * fused kernel; out[wave][32] ticks, n_waves = 4 x workgroups.  PINN_EUNSUPPORTED otherwise. */
int pinn_debug_stamps(pinn_ctx* c, long long* out, int64_t cap, int64_t* n_waves);
/* Profiling build only: s_memtime stamps of the most recent k_lbc_coef launch (7 used of 16). */
int pinn_debug_coef_stamps(long long* out16);
/* Profiling build only: s_memtime stamps of workgroup 0's second group in the most recent k_t16_fused launch,
 * out[wave 0..7][64] (profiles/t16f_stamps.py names the phases). */
int pinn_debug_t16f_stamps(long long* out512);
/* Host-side launch plan of k_t16_fused for hidden width W (65..128; no device is touched): out[0..7] / out[8..15] = each
 * wave's range [lo, hi) in the list of full 16x16 gradient tiles, out[16..23] / out[24..31] = its range in the list of
 * 4-row / 4-column strips, out[32..39] = first feature row of the layer GEMMs it owns, out[40..47] = strips of four rows it
 * owns (4 = a 16-row tile), out[48] = 1 when the last tile per side runs as strips.  tests/test_host_api.py checks that
 * every tile and every row is dealt exactly once for every width. */
int pinn_debug_t16_deal(int W, int* out49);
/* Device and pinned host blocks this process's engine owns right now, and their bytes (every build; no device is touched).
 * Contexts and ensembles give back all they hold when destroyed: a test takes the pair before and after and compares.
 * Either pointer may be NULL.  (Additive: the ABI version stays 6.) */
int pinn_debug_live_buffers(int64_t* n, int64_t* bytes);

/* Ensembles: K = n_members (1..64) copies of one float64 Burgers net (kernel path 7: pde 0 or 1, 2-20-...-20-1 with 4, 6
 * or 8 hidden layers) trained side by side on ONE point set with one set of PDE parameters -- seeds, learning-rate
 * sweeps, repeated identification runs.  Each member has its own weights (lambda_1, lambda_2 included), Adam moments,
 * L-BFGS state, history and log, and non-finite status; member k ends bit-identical to a pinn_ctx trained alone from the
 * same weights with the same calls.  One evaluation of all members = one loss+gradient launch with a member grid dimension
 * + one member-batched reduction.  Per-member arrays are member-major: weights [K][P], gradients [K][P], terms [K][3].
 * Device memory per member, N_f = 10^4, 8 x 20: ~3.8 MB of gradient rows + ~2.5 MB of L-BFGS rings (n_corr = 50) + the
 * member's small per-context buffers (~6.5 MB); the point sets are held once (shared mode; per-member sets, below, add
 * K x n_pad x 24 B: 15 MB at K = 64, N_f = 10^4).  Calls are synchronous.
 * pinn_ens_create refuses float32, Schrodinger, discrete-time models and other shapes with PINN_EUNSUPPORTED and
 * K outside 1..64 with PINN_EINVAL, before touching a device; an ensemble has no communicator.  (Additive: the ABI
 * version stays 6; callers detect the feature by the presence of the symbols.) */
typedef struct pinn_ens pinn_ens;
int pinn_ens_create(pinn_ens** out, const int* layers, int n_layers, const double* lb, const double* ub, int pde_kind,
                    int dtype, int device, int n_members);
int pinn_ens_destroy(pinn_ens* e);
int pinn_ens_size(pinn_ens* e, int* n_members, int64_t* n_params);
/* the point sets and PDE parameters, shared by all members: pinn_set_collocation / _data / _pde_params */
int pinn_ens_set_collocation(pinn_ens* e, const double* X_f, int64_t n, int64_t n_total);
int pinn_ens_set_data(pinn_ens* e, const double* X_u, const double* u, int64_t n, int64_t n_total);
int pinn_ens_set_pde_params(pinn_ens* e, const double* p, int n);
/* w [K][P], n = K * P */
int pinn_ens_set_weights(pinn_ens* e, const double* w, int64_t n);
int pinn_ens_get_weights(pinn_ens* e, double* w, int64_t n);
/* losses [K]; grads [K][P] and terms [K][3] may be NULL */
int pinn_ens_loss_grad(pinn_ens* e, double* losses, double* grads, double* terms);
/* pinn_adam_init per member; lr_k [K] (may be NULL: lr for all) */
int pinn_ens_adam_init(pinn_ens* e, double lr, double beta1, double beta2, double eps, const double* lr_k);
/* n_steps Adam steps of every member; losses [n_steps][K] (may be NULL) = each member's loss before update i */
int pinn_ens_adam_run(pinn_ens* e, int n_steps, double* losses);
/* pinn_lbfgs_begin per member: n_corr, tol_fun, tol_x, max_eval shared; lr_k [K] / max_iter_k [K] may be NULL (lr /
 * max_iter for all) */
int pinn_ens_lbfgs_begin(pinn_ens* e, int n_corr, double tol_fun, double tol_x, double max_eval, double lr,
                         const double* lr_k, int max_iter, const int* max_iter_k);
/* up to n_iters iterations of every member that has not issued its max_iter yet (as pinn_lbfgs_run does per member; a
 * member whose run ended on the device stops moving while the others go on).  iters / losses [K][n_iters + 1] (may be
 * NULL): member k's log entries in row k, n_logged [K] <= n_iters of them (pinn_lbfgs_run's bound; the rows keep their
 * length); done [K] as pinn_lbfgs_run's done. */
int pinn_ens_lbfgs_run(pinn_ens* e, int n_iters, int* iters, double* losses, int* n_logged, int* done);
/* out [K][n] (one output); err [K] = pinn_error_l2 kind 0 per member */
int pinn_ens_predict(pinn_ens* e, const double* X, int64_t n, double* out);
int pinn_ens_error_l2(pinn_ens* e, const double* X, const double* ref, int64_t n, double* err);
/* pinn_get_status per member: n_evals [K], first_nonfinite_eval [K] (either may be NULL) */
int pinn_ens_get_status(pinn_ens* e, int64_t* n_evals, int64_t* first_nonfinite_eval);

/* Per-member point sets and viscosities (parameter sweeps, bagged ensembles, per-epoch resampling).  An ensemble starts
 * in shared mode; the first call below switches it to per-member mode, where member k has its own data, collocation set
 * and nu, held member-major ([K][n_pad] per coordinate), and the shared setters above broadcast (the same set or nu in
 * every member's slots).  Every member has the same counts n and totals n_total, so all share one launch plan; a call
 * whose counts differ from the sets in place rebuilds them as a pinn_ctx does.  Member k stays bit-identical to a
 * pinn_ctx given member k's points, data, nu and seeds with the same calls.  Arrays are member-major: X_f [K][n][2],
 * X_u [K][n][2], u [K][n], nu [K], seeds [K].  Refusals (PINN_EINVAL, nothing changed): null arrays, n_members != K,
 * n, count or n_design out of range, collocation points or a Latin hypercube for identification (pde 1, which has no
 * collocation set; its nu is accepted and unused, as by pinn_set_pde_params).  (Named pinn_ensk_: additive, detected
 * by the presence of the symbols.) */
int pinn_ensk_set_collocation(pinn_ens* e, const double* X_f, int64_t n, int64_t n_total);
int pinn_ensk_set_data(pinn_ens* e, const double* X_u, const double* u, int64_t n, int64_t n_total);
int pinn_ensk_set_pde_params(pinn_ens* e, const double* nu, int n_members);
/* pinn_lhs_collocation for every member in one launch: points [first, first + count) of the n_design-point design with
 * seed seeds[k] become member k's collocation set */
int pinn_ensk_lhs_collocation(pinn_ens* e, int64_t n_design, int64_t first, int64_t count, const uint64_t* seeds);

/* Ensembles of the adr kind: K members of one float64 PINN_PDE_ADR net (kernel path 7, 2-20-...-20-1 with 4, 6 or 8 hidden
 * layers), each with its OWN six coefficients a0, a1, nu, r1, r2, r3 -- Allen-Cahn over interface widths, Fisher-KPP over rho
 * and D, seeds and learning rates for any of them -- on shared or per-member point sets, periodic pairs included.  The
 * constructor returns an ordinary pinn_ens: every pinn_ens_ and pinn_ensk_ call above works on it as it is, except
 * pinn_ensk_set_pde_params (a Burgers call: PINN_EUNSUPPORTED here); terms [k][2] of pinn_ens_loss_grad is member k's
 * periodic part.  Member k ends bit-identical to a pinn_ctx of the adr kind given member k's weights, coefficients and points
 * with the same calls.
 * Coefficients: a new ensemble holds a new adr context's set, Burgers' [0, 1, 0.01 / pi, 0, 0, 0], for every member.
 * pinn_ens_set_pde_params with n = 6 gives one set to all members; pinn_adr_ensk_set_params gives member k row k of
 * p [K][6]; pinn_adr_ens_get_params reads the rows back.  Neither setter switches the ensemble to per-member point sets.
 * Pairs: pinn_adr_ens_set_boundary is pinn_set_boundary for all members (per-member mode: broadcast);
 * pinn_adr_ensk_set_boundary takes X_lb, X_ub [K][n][2], one common n, and switches to per-member mode as the pinn_ensk_ setters
 * above do (every member starts from the shared sets, pairs included).
 * Refusals, all before any device work and with nothing changed: a null argument or K outside 1..64 PINN_EINVAL, a shape
 * other than the one above PINN_EUNSUPPORTED (the constructor); n != 6 or a coefficient that is not finite, n_members != K,
 * counts out of range PINN_EINVAL; the three adr and the two boundary calls on a Burgers ensemble PINN_EUNSUPPORTED.
 * pinn_ens_create itself keeps refusing pde 5 and 6.  Not for members: Robin points, a source term, coefficient fields, point
 * weights, trainable coefficients, adaptive resampling, float32, other kernel paths, communicators.  (Additive: the ABI
 * version stays 6; callers detect the feature by the presence of the symbols.  Named pinn_adr_: the sets of pinn_ens_ and
 * pinn_ensk_ names are the Burgers ensemble's, complete as they stand.) */
int pinn_adr_ens_create(pinn_ens** out, const int* layers, int n_layers, const double* lb, const double* ub, int device,
                        int n_members);
int pinn_adr_ens_set_boundary(pinn_ens* e, const double* X_lb, const double* X_ub, int64_t n, int64_t n_total);
int pinn_adr_ensk_set_boundary(pinn_ens* e, const double* X_lb, const double* X_ub, int64_t n, int64_t n_total);
int pinn_adr_ensk_set_params(pinn_ens* e, const double* p, int n_members);
int pinn_adr_ens_get_params(pinn_ens* e, double* p, int n_members);

/* Self-adaptive point weights (SA-PINN, McClenny & Braga-Neto, arXiv:2009.04544) for Burgers inference (pde 0) in float64 on
 * kernel path 7.  Every data point j and collocation point i gets a trainable weight, and the loss becomes
 *     L = (1/N_f) sum_i lam_f,i^2 f_i^2 + (1/N_u) sum_j lam_u,j^2 (u_j - u*_j)^2
 * with the same global denominators as before.  Each Adam step (pinn_adam_run and its enqueue forms) descends in the network
 * weights and ASCENDS in the lam, both from one evaluation at (theta_t, lam_t): lam += alpha_t m^ / (sqrt(v^) + eps) with
 * dL/dlam = 2 lam r^2 / N, alpha_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t), and the step counter, beta1, beta2 and eps of
 * pinn_adam_init; every lam has its own moments.  The ascent runs inside the loss+gradient kernel (no extra launch).
 * pinn_loss_grad, the L-BFGS evaluations, pinn_residual*, pinn_predict and pinn_error_l2 read the weights and never move
 * them: L-BFGS minimises the weighted loss with lam frozen at their values after Adam, the paper's Adam -> L-BFGS schedule.
 *   pinn_sa_set_weights  enables the weighted loss; lam_u [n_u] in the order of pinn_set_data's rows, lam_f [n_f] in the
 *                        order of the collocation set (for a device-drawn set: what pinn_get_collocation returns); the counts
 *                        must equal the current local set sizes.  Zeroes the moments.
 *   pinn_sa_get_weights  reads them back (same shapes); PINN_EINVAL while the weights are off
 *   pinn_sa_adam_init    the ascent's rate lr (default 0: the weights are held fixed, their moments do not move)
 *   pinn_sa_disable      back to the plain kernel: results bit-identical to a context that never enabled the weights
 * pinn_set_collocation, pinn_lhs_collocation and pinn_rad_collocation reset the collocation weights to 1 and their moments to
 * 0, pinn_set_data the data weights.  Refusals, before any device work, the context unchanged: PINN_EUNSUPPORTED for pde != 0,
 * float32, a kernel path other than 7 or a communicator (pinn_comm_init, pinn_comm_xgmi_export and pinn_set_kernel_path to
 * another path are refused the same way while the weights are on); PINN_EINVAL for null arrays, counts that differ from the
 * set sizes, non-finite weights, a negative or non-finite lr.  (Additive: the ABI version stays 6.) */
int pinn_sa_set_weights(pinn_ctx* c, const double* lam_u, int64_t n_u, const double* lam_f, int64_t n_f);
int pinn_sa_get_weights(pinn_ctx* c, double* lam_u, int64_t n_u, double* lam_f, int64_t n_f);
int pinn_sa_adam_init(pinn_ctx* c, double lr);
int pinn_sa_disable(pinn_ctx* c);

/* Per-point loss weights of the adr kind (PINN_PDE_ADR), fixed or self-adaptive (McClenny & Braga-Neto, arXiv:2009.04544):
 *   L = (1/N_f) sum_i lam_f,i^2 f_i^2 + (1/N_u) sum_j lam_u,j^2 (u_j - u*_j)^2
 *       + (1/N_b) sum_p lam_b,p^2 [(u(lo_p) - u(hi_p))^2 + (u_x(lo_p) - u_x(hi_p))^2]
 * with the global denominators of the plain loss; a periodic pair has ONE weight.  pinn_loss_grad's terms are the three
 * weighted parts.  A static term weight W on a class is lam = sqrt(W) on its points with rate 0.  With a rate above 0 every
 * Adam step descends in the network weights and ascends in that class's lam from one evaluation:
 * dL/dlam = 2 lam r^2 / N (r^2 = f^2, (u - u*)^2 or a pair's two squares), stepped by
 * rate sqrt(1 - b2^t) / (1 - b1^t) m / (sqrt(v) + eps) with the step counter, b1, b2 and eps of pinn_adam_init; every lam has
 * its own moments, a class with rate 0 is not touched.  The ascent runs inside the loss+gradient kernel (no extra launch).
 * L-BFGS, pinn_loss_grad, pinn_predict, pinn_error_l2, pinn_residual, pinn_residual_at and pinn_rad_collocation read the
 * weights and never move them; the residual calls and the adaptive draw see the unweighted f.
 *   pinn_pw_set        enables the weighted loss; lam_u [n_u] in the order of pinn_set_data's rows, lam_f [n_f] in the order
 *                      of the collocation set (what pinn_get_collocation returns), lam_b [n_b] one per pair in the order of
 *                      pinn_set_boundary's rows.  The counts must equal the current local set sizes (0 for an empty set);
 *                      a NULL array with the right count means all ones.  Zeroes all moments.
 *   pinn_pw_get        reads them back (same shapes; a NULL array is skipped); PINN_EINVAL while the weights are off
 *   pinn_pw_adam_init  the ascent's rates per class (default 0, 0, 0: fixed weights)
 *   pinn_pw_disable    back to the plain kernel: results bit-identical to a context that never enabled the weights
 * pinn_set_collocation, pinn_lhs_collocation and pinn_rad_collocation reset the collocation weights to 1 and their moments to
 * 0, pinn_set_data the data weights, pinn_set_boundary the pairs'; the other classes keep theirs.  Refusals, before any
 * device work, the context unchanged: PINN_EUNSUPPORTED for any kind but PINN_PDE_ADR, float32, a kernel path other than 7 or
 * a communicator (pinn_comm_init, pinn_comm_xgmi_export and pinn_set_kernel_path to another path are refused the same way
 * while the weights are on); PINN_EINVAL for counts that differ from the set sizes, non-finite weights, a negative or
 * non-finite rate.  (Additive: the ABI version stays 6.) */
int pinn_pw_set(pinn_ctx* c, const double* lam_u, int64_t n_u, const double* lam_f, int64_t n_f, const double* lam_b,
                int64_t n_b);
int pinn_pw_get(pinn_ctx* c, double* lam_u, int64_t n_u, double* lam_f, int64_t n_f, double* lam_b, int64_t n_b);
int pinn_pw_adam_init(pinn_ctx* c, double rate_u, double rate_f, double rate_b);
int pinn_pw_disable(pinn_ctx* c);

/* Robin points of the adr kind (PINN_PDE_ADR): a fourth point class.  Point j is a location (x_j, t_j) with three numbers
 * (alpha_j, beta_j, g_j); its residual and the loss are
 *   r_j = alpha_j u(x_j, t_j) + beta_j u_x(x_j, t_j) - g_j
 *   L   = mean_f f^2 + mean_u (u - u*)^2 + mean_b [(u_lo - u_hi)^2 + (u_x,lo - u_x,hi)^2] + (1 / N_w) sum_j r_j^2
 * with N_w = n_total, the global count.  The coefficients are per point: (1, 0, g) is a Dirichlet value, (0, 1, g) a Neumann
 * flux, (h, 1, g) a Robin wall; g may differ from point to point (time-dependent wall data), and a point may lie inside the
 * domain (a derivative observation).  The Robin part is ADDED to the boundary part: pinn_loss_grad's terms[2] = periodic
 * part + Robin part; the gradient row keeps its layout.  Float32 and float64, kernel paths 0 and 7.
 *   pinn_set_robin       X_w [n][2] = (x, t), alpha, beta, g [n]; replaces the class, n = 0 removes it -- from then on every
 *                        result is bit-identical to a context that never had Robin points.  The points survive
 *                        pinn_set_collocation, pinn_lhs_collocation, pinn_rad_collocation, pinn_set_data and
 *                        pinn_set_boundary; they are no collocation points (pinn_get_collocation, pinn_residual and the
 *                        adaptive draw do not see them).
 *   pinn_robin_residual  r_j at the current weights, forward only; n must be the local count (n = 0: nothing is written)
 * Refusals, before any device work, the context unchanged: PINN_EUNSUPPORTED for any kind but PINN_PDE_ADR (PINN_PDE_ADR_IDE
 * included), while point weights are on (and pinn_pw_set is refused while Robin points are present), a kernel path other
 * than 0 or 7, a communicator (pinn_comm_init and pinn_comm_xgmi_export are refused the same way while Robin points are
 * present); PINN_EINVAL for null arrays with n > 0, n < 0 or n_total < n, a non-finite coordinate or coefficient, a point
 * with alpha = beta = 0 (it constrains nothing), a buffer of another length.  (Additive: the ABI version stays 6.) */
int pinn_set_robin(pinn_ctx* c, const double* X_w /*[n][2]*/, const double* alpha, const double* beta, const double* g,
                   int64_t n, int64_t n_total);
int pinn_robin_residual(pinn_ctx* c, double* out /*[n]*/, int64_t n);
/* Three-term wall points of PINN_PDE_ADR2: r_j = alpha_j u + beta_j u_x + gamma_j u_t - g_j, everything else as pinn_set_robin
 * (storage, N_w = n_total, the wall part added to terms[2], n = 0 removes the class; pinn_robin_residual returns r_j).
 * (0, 0, 1, v0) is the initial velocity of a wave or a Neumann wall y = const of a 2-D problem, (0, c, 1, 0) the Sommerfeld
 * wall u_t + c u_x = 0.  PINN_EINVAL for a point with alpha = beta = gamma = 0 and for what pinn_set_robin refuses so;
 * PINN_EUNSUPPORTED for every kind but PINN_PDE_ADR2.  (Additive: the ABI version stays 6.) */
int pinn_set_robin3(pinn_ctx* c, const double* X_w /*[n][2]*/, const double* alpha, const double* beta, const double* gamma,
                    const double* g, int64_t n, int64_t n_total);

/* Source term of the adr kind (PINN_PDE_ADR): a right-hand side s(x, t), given as one value per LOCAL collocation point.  The
 * residual of collocation point i and the loss are
 *   f_i = u_t + (a0 + a1 u) u_x - nu u_xx + r1 u + r2 u^2 + r3 u^3 - s_i
 *   L   = mean_f f^2 + (data, pairs and Robin parts as without a source)
 * With s = N[u*] for a closed-form u*, u* is the exact solution of any member of the family with any wall kind (the method
 * of manufactured solutions).  The gradient row, terms and every optimiser call keep their layout.  Float32 and float64,
 * kernel paths 0 and 7; Robin points may be present.
 *   pinn_set_source   s [n], n = the local collocation count; replaces the source.  s == NULL with n == 0 removes it -- from
 *                     then on every result is bit-identical to a context that never had a source.  A source of zeros gives
 *                     those bits too.  The source survives pinn_set_data, pinn_set_boundary, pinn_set_robin and
 *                     pinn_set_pde_params.
 * Stale rule: pinn_set_collocation and pinn_lhs_collocation replace the points, not the values, so a present source
 * becomes STALE.  While it is stale pinn_loss_grad, the Adam and L-BFGS entry points (enqueue forms included) and
 * pinn_residual return PINN_ESTATE and launch nothing; pinn_get_collocation still works -- it hands out the new points --
 * and pinn_set_source with values at them, or with n = 0, clears the state.
 * Residuals: pinn_residual (over the set) returns f including - s.  pinn_residual_at cannot know s at foreign points: it
 * returns the operator part N[u]; subtract s there yourself.
 * Refusals, before any device work, the context unchanged: PINN_EINVAL for a null array with n > 0, n < 0 or a non-finite
 * value (whatever the context is), and for n other than the local collocation count; PINN_EUNSUPPORTED for any kind but
 * PINN_PDE_ADR (PINN_PDE_ADR_IDE included), while point weights are on (and pinn_pw_set is refused while a source is
 * present), a kernel path other than 0 or 7, a communicator (pinn_comm_init and pinn_comm_xgmi_export are refused the same
 * way while a source is present).  pinn_rad_collocation is refused with PINN_EUNSUPPORTED while a source is present -- the
 * pool's residuals would lack s -- and does NOT make the source stale.  (Additive: the ABI version stays 6.) */
int pinn_set_source(pinn_ctx* c, const double* s /*[n]*/, int64_t n);

/* Coefficient fields of the adr kind (PINN_PDE_ADR): variable media.  Each LOCAL collocation point i gets a row of six
 * coefficients K_i = (a0, a1, nu, r1, r2, r3)_i, and the residual and the loss are
 *   f_i = u_t + (a0_i + a1_i u) u_x - nu_i u_xx + r1_i u + r2_i u^2 + r3_i u^3 - s_i      (s_i = 0 without a source)
 *   L   = mean_f f^2 + (data, pairs and Robin parts as without fields)
 * A rod of two materials, a diffusivity nu(x), a prescribed velocity field a0(x, t), a reaction rate that depends on place or
 * time; the conservative term -(nu(x) u_x)_x is the field nu with the field a0 = -nu'(x).  The table is dense, [n][6], no
 * mask: a coefficient that does not vary is a constant column.  The gradient row, terms and every optimiser call keep their
 * layout.  Float32 and float64, kernel paths 0 and 7; Robin points and a source may be present in any combination.
 *   pinn_set_coef_fields   K [n][6], n = the local collocation count; replaces the fields.  K == NULL with n == 0 removes them
 *                          -- from then on every result is bit-identical to a context that never had them.  A table whose
 *                          every row is the context's constant set gives the bits of the context without fields.  The fields
 *                          survive pinn_set_data, pinn_set_boundary, pinn_set_robin, pinn_set_source and pinn_set_pde_params.
 * While fields are present the six constants of pinn_set_pde_params are read by no evaluation; the call stays allowed, its
 * values are kept and count again after removal.
 * Stale rule (the source's): pinn_set_collocation and pinn_lhs_collocation make present fields STALE.  While they are stale
 * pinn_loss_grad, the Adam and L-BFGS entry points (enqueue forms included) and pinn_residual return PINN_ESTATE and launch
 * nothing; pinn_get_collocation still works, and pinn_set_coef_fields with rows at the new points, or with n = 0, clears the
 * state.  A source and fields may both be stale: each is cleared by its own setter, and the message names both.
 * Residuals: pinn_residual (over the set) returns f with the rows, including - s_i.  pinn_residual_at returns
 * PINN_EUNSUPPORTED while fields are present: the coefficients are not known at foreign points.
 * Refusals, before any device work, the context unchanged: PINN_EINVAL for a null array with n > 0, n < 0 or a non-finite
 * entry (whatever the context is -- a row is refused where pinn_set_pde_params would refuse it as a constant set), and for n
 * other than the local collocation count; PINN_EUNSUPPORTED for any kind but PINN_PDE_ADR (PINN_PDE_ADR_IDE included), while
 * point weights are on (and pinn_pw_set is refused while fields are present), a kernel path other than 0 or 7, a
 * communicator (pinn_comm_init and pinn_comm_xgmi_export are refused the same way while fields are present).
 * pinn_rad_collocation is refused with PINN_EUNSUPPORTED while fields are present and does NOT make them stale.
 * (Additive: the ABI version stays 6.) */
int pinn_set_coef_fields(pinn_ctx* c, const double* K /*[n][6]*/, int64_t n);

#ifdef __cplusplus
}
#endif
#endif /* PINN_HIP_H */
