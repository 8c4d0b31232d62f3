// engine.hip -- context, device memory, launch sequencing and the C ABI (include/pinn_hip.h)
// of the MI355X PINN engine.  Built for gfx950 only:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-slp-vectorize -fPIC -c engine.hip
//   hipcc ... -mllvm -amdgpu-mfma-vgpr-form=1 -fPIC -c fused20d_unit.hip          (see fused20d_api.h)
//   hipcc ... -fPIC -c fused20m_unit.hip                                              (see fused20m_api.h)
//   hipcc --offload-arch=gfx950 -shared -fPIC engine.o fused20d_unit.o fused20m_unit.o -o libpinn_hip.so -lrccl
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>
#include <chrono>
#include <type_traits>
#include <vector>

#include "../../include/pinn_hip.h"
#include "devbuf.h"
#include "optim_host.h"
#include "kernels_fused20.h"
#include "kernels_fused20m.h"
#include "fused20d_api.h"
#include "fused20m_api.h"
#include "kernels_wide.h"
#include "kernels_generic.h"
#include "kernels_optim.h"
#include "kernels_disc.h"
#include "kernels_sampling.h"
#include "kernels_rad.h"
#include "kernels_tile16.h"
#include "kernels_tile16f.h"
#include "kernels_xgmi.h"
#include "kernels_predict20.h"

#include <dlfcn.h>

using namespace pinn;

// ------------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------------
static thread_local std::string g_err;

static int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIPCHK(expr)                                                                      \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess)                                                                 \
      return fail(PINN_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),       \
                  __FILE__, __LINE__);                                                    \
  } while (0)

#define NCCLCHK(expr)                                                                     \
  do {                                                                                    \
    ncclResult_t r_ = (expr);                                                             \
    if (r_ != ncclSuccess)                                                                \
      return fail(PINN_ECOMM, "%s failed: %s (%s:%d)", #expr, ncclGetErrorString(r_),     \
                  __FILE__, __LINE__);                                                    \
  } while (0)

#define REQUIRE(cond, ...)                                \
  do {                                                    \
    if (!(cond)) return fail(PINN_EINVAL, __VA_ARGS__);   \
  } while (0)

// ------------------------------------------------------------------------------------------
// roctx ranges around the phases (the reference only prints wall-clock times, utils/logger.py:21-30):
// librocprofiler-sdk-roctx is looked up lazily, so the engine has no hard dependency on it and a range costs one
// predictable branch when no profiler is around.  rocprofv3 --marker-trace shows them as
// pinn_adam_run / pinn_lbfgs_run / pinn_loss_grad / pinn_predict / pinn_error_l2.
// ------------------------------------------------------------------------------------------
struct Roctx {
  int (*push)(const char*) = nullptr;
  int (*pop)() = nullptr;
  Roctx() {
    if (getenv("PINN_NO_ROCTX")) return;
    void* h = dlopen("librocprofiler-sdk-roctx.so", RTLD_LAZY | RTLD_GLOBAL);
    if (!h) h = dlopen("librocprofiler-sdk-roctx.so.1", RTLD_LAZY | RTLD_GLOBAL);
    if (!h) return;
    push = (int (*)(const char*))dlsym(h, "roctxRangePushA");
    pop = (int (*)())dlsym(h, "roctxRangePop");
    if (!push || !pop) push = nullptr, pop = nullptr;
  }
};
static Roctx& roctx() { static Roctx r; return r; }
struct Range {
  bool on;
  explicit Range(const char* name) : on(roctx().push != nullptr) { if (on) roctx().push(name); }
  ~Range() { if (on) roctx().pop(); }
};

// ------------------------------------------------------------------------------------------
// context
// ------------------------------------------------------------------------------------------
static constexpr int CHUNK_POINTS = 32768;   // points per forward/backward launch pair
static constexpr int LOSS_SLOTS = 4;         // residual, data, boundary, pad

// The kernel families that serve a loss+gradient evaluation.  The values are the numbers of the ABI (pinn_set_kernel_path,
// include/pinn_hip.h); what the engine knows about each path stands in PATHS and path_rows below, nowhere else.
enum KernelPath : int {
  KP_GENERIC = 0,    // one lane per point, chunked
  KP_FUSED20 = 1,    // width 20, one kernel, whole-set stash in HBM (kernels_fused20.h)
  KP_FUSED20M = 2,   // width 20 float32, one kernel, register stash (kernels_fused20m.h)
  KP_WIDE = 3,       // width 100, two outputs, float32: wide MFMA sweeps per chunk (kernels_wide.h)
  KP_T16 = 4,        // shape-generic MFMA sweeps per chunk (kernels_tile16.h)
  KP_T16_FWD = 5,    // 4's forward half with the generic reverse half (tests)
  KP_T16_BWD = 6,    // the generic forward half with 4's reverse half (tests)
  KP_FUSED20D = 7,   // width 20 float64, one kernel, register stash (kernels_fused20d.h)
  KP_T16_FUSED = 8,  // float64 widths 65..128: forward + reverse of a group in one kernel per chunk (kernels_tile16f.h)
  KP_COUNT
};

// Host side of a per-point weight array of fused20d_api.h: a header, then (lambda, m, v) per point, class behind class.
// hdr: the header as uploaded, n_hdr doubles of it; n[k]: the entries class k is laid out for; reset[k]: that class's set was
// replaced since (lam_prepare puts its weights back to 1).  A surface that has no pairs leaves that class empty.
enum { LAM_PAIRS, LAM_DATA, LAM_COL, LAM_CLASSES };
struct LamStore {
  DevBuf<double> buf;
  int n_hdr = 0;
  double hdr[PW_CONST] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // the longer of the two headers; the rest stays 0
  int n[LAM_CLASSES] = {0, 0, 0};
  bool reset[LAM_CLASSES] = {false, false, false};
};

struct pinn_ctx {
  int device = 0, dtype = PINN_F32, pde = PINN_PDE_BURGERS;
  KernelPath path = KP_GENERIC;
  hipStream_t stream = nullptr;
  bool own_stream = true;            // false: an ensemble member, on its ensemble's stream (pinn_ens_create)
  NetDesc nd{};
  int layers[MAX_DENSE + 1]{};
  int n_layers = 0;
  double lb[2]{}, ub[2]{}, nu = 0.0;
  double adr[8]{};                   // PINN_PDE_ADR: a0, a1, nu, r1, r2, r3 (pinn_set_pde_params); [6]: d3 of PINN_PDE_ADRD_DISC at create;
                                     // PINN_PDE_ADR2: [6] = b, [7] = kappa
  int adr_mask = 0;                  // PINN_PDE_ADR_IDE, PINN_PDE_ADR_DISC_IDE, PINN_PDE_ADRD_DISC: bit k set = coefficient k is trained (pinn_set_pde_trainable)
  bool nu_off = false;               // PINN_PDE_ADRD_DISC: nu == 0 (pinn_set_pde_params); the kernels get it by value, the nu slot holds 0.0

  // host copies of the point sets (float64, as handed over)
  PointSets sets;
  int64_t nf_total = 0, nu_total = 0, nb_total = 0;
  bool sets_dirty = true;
  SetDesc sd{};

  // device: training set (compute dtype)
  DevBuf<void> xs, ts, tgt;
  // device: parameters / optimiser (float64) + compute-dtype mirror.  In an ensemble member theta, theta_r, gl, adam_m, adam_v
  // and d_nonfinite (below) are views of the ensemble's blocks (ens_build)
  DevBuf<double> theta, gl, adam_m, adam_v;
  DevBuf<void> theta_r;
  DevBuf<float> img;                 // LDS weight image of k_fused20m (f32 only)
  DevBuf<int> row_index;             // k_fused20d: entry of a wave's gradient block list -> flat parameter index
  int n_cu = 256, n_wg = 0;          // compute units; workgroups of the persistent kernel
  int f64_split = -1;                // PINN_F64_SPLIT, read by pinn_create: -1 auto, 0 never, 1 required (split_plan)
  // device: scratch
  DevBuf<void> S, O, ZA, ZB, part;
  int chunk = 0, n_rows = 0, R = 0;
  // device: evaluation-only scratch (predict)
  DevBuf<void> xe, te, Oe;
  DevBuf<double> f_out;
  // evaluation points / reference values of the last predict / error call, kept on the host (to recognise a repeat:
  // the scripts evaluate the same X_star grid again and again) and on the device
  std::vector<double> ev_X, ev_ref;
  int ev_n_pad = 0;
  DevBuf<double> pred, d_ref, err_partial, err_res;
  PinnedBuf<double> h_err;           // [3]
  // first evaluation (1-based count since pinn_create) whose reduced loss was not finite; 0 = none so far.
  // The reference has no such guard (a NaN loss just propagates, custom_lbfgs.py:154); this only records it.
  DevBuf<unsigned long long> d_nonfinite;
  unsigned long long n_evals = 0;

  // Adam
  struct {
    double lr = 1e-3, b1 = 0.9, b2 = 0.999, eps = 1e-7;
    int64_t t = 0;
    bool ready = false, want_terms = false;
    DevBuf<double> loss_hist;        // N_PENDING regions of hist_stride steps x 3 loss parts (one per chunk in flight)
    size_t hist_stride = 0;          // layout, not a guard: where a ticket's region starts; follows the ring when it is replaced
  } adam;

  // Chunks of optimiser steps whose results the host has not collected yet (pinn_adam_enqueue / pinn_lbfgs_enqueue ->
  // ..._collect): the kernels of chunk k+1 are already in the stream while the host reads and logs chunk k, so a logging
  // boundary costs the GPU nothing.  Each chunk's results travel by asynchronous copies into its own pinned buffers, behind
  // its own event; tickets are collected in the order they were issued.
  struct Pending {
    int kind = 0;                      // 1 Adam, 2 L-BFGS
    int n = 0;                         // Adam: steps; L-BFGS: length of the log window copied
    int base = 0, issued_upto = 0;     // L-BFGS: first log entry of the window; iterations issued when it was enqueued
    bool want_terms = false;
    hipEvent_t ev = nullptr;
    PinnedBuf<double> h_loss;
    PinnedBuf<int> h_iter;
    PinnedBuf<LbfgsState> h_state;
  };
  static constexpr int N_SNAP = 4;     // pinn_weights_snapshot / _restore slots
  DevBuf<double> snap;
  unsigned snap_valid = 0;
  struct : Tickets { Pending pend[N_PENDING]; } tk;   // the counters (optim_host.h) and the slots they index

  // L-BFGS
  struct {
    int issued_at_read = 0;          // iters_issued when logged_read was last brought up to date
    DevBuf<LbfgsState> state;        // two copies (double buffered, see k_lbc_coef_apply); flip = current
    int flip = 0;
    DevBuf<double> x, d, gold, S, Y, ro, al, q, log_loss;
    DevBuf<int> log_iter;
    // (the host mirrors read back by pinn_lbfgs_run -- state + the log entries a chunk may have produced, three asynchronous
    //  copies behind ONE wait; two blocking hipMemcpy more cost ~25 us per call -- are the Pending buffers above)
    int max_iter = 0, ncorr = 0, logged_read = 0;
    double lr = 1.0, tol_fun = 0, tol_x = 0, max_eval = 0;
    int iters_issued = 0;
    bool post_pending = false;       // an evaluation whose break tests / log entry are still due
    bool ready = false;
    // compact (Gram-matrix) mode
    int mode = 1, mode_active = 0, M1 = 0;
    DevBuf<double> SY, YY, dots, cs, cy;
    DevBuf<LbcExtra> ex;
  } lbfgs;
  double t16_cost_full = T16_COST_FULL, t16_cost_strip = T16_COST_STRIP;   // k_t16_fused: weights of the gradient-tile dealing (t16_deal; PINN_T16_COSTS)
  long long t16_handover_ticks = 50000000ll;   // bound of that hand-over's wait, 100 MHz ticks (PINN_T16_HANDOVER_TICKS)
  bool t16_prepass_pinned = false;     // PINN_T16_PREPASS was given: the data-parallel default below does not apply
  bool t16_prepass = false;            // k_t16_fused: boundary outputs by a k_t16_fwd pre-pass instead of the in-kernel hand-over
                                       // (PINN_T16_PREPASS=1, or switched on for good after a hand-over that timed out)
  DevBuf<unsigned int> t16_bsync;      // k_t16_fused: boundary-group hand-over counter (never reset; t16_bcount = its value after the last launch)
  unsigned int t16_bcount = 0;
  DevBuf<double> t16_gscr;             // k_t16_fused: tile-major weight-gradient scratch, one block per workgroup

  // Where the collocation block comes from: handed over (sets.Xf), generated on the device (pinn_lhs_collocation) or drawn
  // by residual-based adaptive sampling (pinn_rad_collocation).  The two device origins take points first .. first + count - 1
  // of an n_design-point design
  enum ColFrom { COL_HANDED, COL_LHS, COL_RAD };
  struct ColOrigin { ColFrom from = COL_HANDED; int64_t n_design = 0, first = 0, count = 0; } col;
  struct { uint64_t seed = 0; } lhs;   // the device LHS's seed (kept when the origin changes: ens_to_k starts from it)
  // the adaptive draw (kernels_rad.h): the drawn points as a float64 device copy (cx, ct: ensure_sets re-places them after a
  // re-assembly) and the call's own buffers -- pool points, their Taylor outputs and residuals, integer weights, block sums,
  // totals -- so that no evaluation cache is disturbed
  struct {
    bool filled = false;
    DevBuf<double> cx, ct;
    DevBuf<void> px, pt, O;
    DevBuf<double> f;
    DevBuf<unsigned long long> w, bsum;
    DevBuf<RadTotals> tot;
  } rad;

  // self-adaptive point weights (pinn_sa_*, k_fused20d<0, H, ., false, false, true>): SA_CONST header, data and collocation points
  struct {
    bool on = false;
    double lr = 0.0;
    LamStore arr;
  } sa;
  // per-point loss weights of the adr kind (pinn_pw_*, k_fused20d<PDE_ADR, H, ., false, false, true>): PW_CONST header, two
  // entries per pair, data and collocation points
  struct {
    bool on = false;
    double rate[3] = {0.0, 0.0, 0.0};          // data, collocation, pairs
    LamStore arr;
  } pw;

  // Robin points of the adr kind (pinn_set_robin; template value PDE_ADR_ROBIN of the kernels): as handed over, and the
  // (alpha, beta) pairs on the device in the compute dtype.  The block stands behind the collocation block of the assembled
  // set: points first .. first + n - 1 (ensure_sets)
  struct {
    std::vector<double> X, alpha, beta, g;
    std::vector<double> gamma;         // PINN_PDE_ADR2 (pinn_set_robin3; zeros from pinn_set_robin): rows (alpha, beta, gamma, 0) in ab
    int64_t n_total = 0;
    DevBuf<void> ab;
    int first = 0, n = 0;
    DevBuf<double> out;                // pinn_robin_residual's device buffer
  } robin;

  // source term of the adr kind (pinn_set_source; template value PDE_ADR_SRC of the kernels): s_i as handed over, one value per
  // local collocation point.  ensure_sets places them in tgt at the collocation indices.  stale: the collocation points were
  // replaced since (pinn_set_collocation, pinn_lhs_collocation) -- the values belong to other points, nothing evaluates until
  // pinn_set_source is called again
  struct {
    std::vector<double> s;
    bool on = false, stale = false;
  } src;

  // coefficient fields of the adr kind (pinn_set_coef_fields; template value PDE_ADR_VAR of the kernels): the table as handed
  // over, K[6 i + j] = coefficient j of local collocation point i, and its device copy in the compute dtype (ensure_sets).
  // stale: as the source's flag, for the same reason and cleared by this kind's own setter.  While on, c->adr is kept but not
  // read by any evaluation
  struct {
    std::vector<double> K;
    bool on = false, stale = false;
    DevBuf<void> dev;
  } kf;

  // discrete-time models (pde 3, 4, 7): stage sets as handed over, device copies, scratch
  struct DiscSet { std::vector<double> x, t, M; int q = 0; bool has_M = false; };
  DiscSet dset[2];
  // periodic pairs of the adr_disc kind (pinn_disc_set_periodic): row i of lb with row i of ub; a third slot beside the two
  // stage sets, assembled by disc_ensure into groups of 8 pairs behind theirs
  struct { std::vector<double> lb, ub; int order = 0; } dper;
  DiscDesc dd{};
  DevBuf<int> d_ginfo;
  DevBuf<void> d_M[2], d_MT[2];        // empty: that stage set has no table
  DevBuf<void> d_Ast, d_A3, d_U3, d_Nn, d_R, d_dAp, d_lossp, d_lamp;

  // RCCL
  ncclComm_t comm = nullptr;
  int n_ranks = 1, rank = 0;
  // peer-mapped mailbox all-reduce (kernels_xgmi.h); comm_mode: 0 none, 1 RCCL, 2 mailboxes
  struct {
    void* box = nullptr;                      // this rank's mailbox (uncached, exported through hipIpc): raw, xg_release frees it
    void* opened[XG_MAX_RANKS] = {};          // peers' mailboxes as mapped here (nullptr for own rank)
    XgPeers peers{};
    DevBuf<int> err;
    unsigned int seq = 0;                     // evaluation counter; 0 is never used (an all-zero mailbox is invalid)
    bool attached = false, on = false;
    bool poisoned = false;                    // a peer was lost mid-step: weights / moments are a mix of two iterates
    int sharing = 1;                          // ranks whose mailbox lives on THIS device (1 = one rank per GPU, the product case)
    int grid_cap = 0;                         // > 0: at most this many workgroups in k_reduce_xgmi (a shared device, see there)
  } xg;

  // per-wave phase timeline of the fused kernel (profiling build only)
  DevBuf<long long> stamps;
  // timing
  std::vector<hipEvent_t> ev;
  int ev_used = 0, ev_cap_evals = 0, ev_every = 1;
  int64_t ev_seen = 0;
  bool timing = false;
  double ev_overhead_ms = 0.0;       // elapsed time of an empty event bracket on this stream (calibration)
};

static size_t real_size(const pinn_ctx* c) { return c->dtype == PINN_F64 ? 8 : 4; }
// The compute type of c as a type: calls f with a value of it (auto r; using real = decltype(r)), so a launch that differs
// between the two dtypes in `real` alone is written once.  Inlined by force, as by_kind below: the evaluation and the update
// kernels are issued from the optimisers' step loops, where a one-tile step is as short as the host's own work.
template <typename F>
__attribute__((always_inline)) static inline auto by_real(const pinn_ctx* c, F&& f) {
  if (c->dtype == PINN_F64) return f(double());
  return f(float());
}
static bool disc_kind(int pde) {
  return pde == PINN_PDE_BURGERS_DISC || pde == PINN_PDE_BURGERS_DISC_IDE || pde == PINN_PDE_ADR_DISC ||
         pde == PINN_PDE_ADR_DISC_IDE || pde == PINN_PDE_ADRD_DISC;
}
static bool is_disc(const pinn_ctx* c) { return disc_kind(c->pde); }
// the discrete-time model of the adr operator: template value DISC_ADR of the kernels of kernels_disc.h, six coefficients in
// c->adr as for the adr kind, and the one kind with periodic pairs (pinn_disc_set_periodic)
static bool is_adr_disc(const pinn_ctx* c) { return c->pde == PINN_PDE_ADR_DISC; }
// the same model with trainable coefficients: template value DISC_ADR_IDE, the six are the tail of theta as for adr_ide
// (adr_ide_write_tail, c->adr_mask), periodic pairs allowed
static bool is_adr_disc_ide(const pinn_ctx* c) { return c->pde == PINN_PDE_ADR_DISC_IDE; }
// adr_disc_ide with a dispersion term d3 U_xxx: template value DISC_ADRD (four Taylor channels), a tail of seven
// ([.., d3], raw) and a flag for nu == 0 (c->nu_off)
static bool is_adrd_disc(const pinn_ctx* c) { return c->pde == PINN_PDE_ADRD_DISC; }
static bool has_pairs(const pinn_ctx* c) { return is_adr_disc(c) || is_adr_disc_ide(c) || is_adrd_disc(c); }
static bool has_lambdas(int pde) { return pde == PINN_PDE_BURGERS_IDE || pde == PINN_PDE_BURGERS_DISC_IDE; }
// advection-diffusion-reaction with run-time coefficients: template value PDE_ADR of the continuous kernels
// (kernels_generic.h); it runs on the generic path 0 and, float64 width 20, on k_fused20d (path 7)
static bool is_adr(const pinn_ctx* c) { return c->pde == PINN_PDE_ADR; }
// the same equation with trainable coefficients: template value PDE_ADR_IDE, the six coefficients are the tail of theta
// ([a0, a1, log nu, r1, r2, r3]); the same two paths
static bool is_adr_ide(const pinn_ctx* c) { return c->pde == PINN_PDE_ADR_IDE; }
// the kinds whose tail is [a0, a1, log nu, r1, r2, r3] (adrd_disc: and d3) with a mask of the trained ones
static bool has_adr_tail(const pinn_ctx* c) { return is_adr_ide(c) || is_adr_disc_ide(c) || is_adrd_disc(c); }
// the adr equation with b u_t and u_xx + kappa u_tt as one Taylor channel: template value PDE_ADR2, eight coefficients in
// c->adr, the point classes of the adr kind with three-term wall points and a source; the generic path 0 and, float64
// width 20, k_adr2_20d (path 7)
static bool is_adr2(const pinn_ctx* c) { return c->pde == PINN_PDE_ADR2; }
// the kinds whose sets are the adr kind's: interleaved periodic pairs, no fused kernel of the Burgers kinds
static bool adr_family(const pinn_ctx* c) { return is_adr(c) || is_adr_ide(c) || is_adr2(c); }
// the kinds that take wall points (pinn_set_robin) and a source (pinn_set_source)
static bool has_walls(const pinn_ctx* c) { return is_adr(c) || is_adr2(c); }
// trailing equation parameters of the flat weight vector
static int tail_len(int pde) {
  return has_lambdas(pde) ? 2 : pde == PINN_PDE_ADR_IDE || pde == PINN_PDE_ADR_DISC_IDE ? 6 : pde == PINN_PDE_ADRD_DISC ? 7 : 0;
}
// what a kernel of kind PDE takes in the place of the scalar nu
template <typename real, int PDE>
static pde_coef_t<real, PDE> pde_coef(const pinn_ctx* c) {
  if constexpr (PDE == PDE_ADR)
    return AdrCoef<real>{(real)c->adr[0], (real)c->adr[1], (real)c->adr[2], (real)c->adr[3], (real)c->adr[4], (real)c->adr[5]};
  else if constexpr (PDE == PDE_ADR_ROBIN)
    return AdrRobinArg<real>{AdrCoef<real>{(real)c->adr[0], (real)c->adr[1], (real)c->adr[2], (real)c->adr[3], (real)c->adr[4], (real)c->adr[5]},
                             c->robin.ab.as<real>(), c->robin.first, c->robin.n,
                             (real)(c->robin.n_total > 0 ? 1.0 / (double)c->robin.n_total : 0.0)};
  else if constexpr (PDE == PDE_ADR_SRC)   // the set's own residuals: s by set index is tgt itself
    return AdrSrcArg<real>{pde_coef<real, PDE_ADR_ROBIN>(c), c->tgt.as<real>()};
  else if constexpr (PDE == PDE_ADR_VAR)   // the collocation slots of tgt are zero without a source
    return AdrVarArg<real>{pde_coef<real, PDE_ADR_SRC>(c), c->kf.dev.as<real>()};
  else if constexpr (PDE == PDE_ADR_IDE)
    return AdrIdeArg{c->adr_mask};
  else if constexpr (PDE == PDE_ADR2)      // src: the set's tgt, zero in the collocation block without a source
    return Adr2Arg<real>{pde_coef<real, PDE_ADR>(c), (real)c->adr[6], (real)c->adr[7], c->robin.ab.as<real>(), c->robin.first,
                         c->robin.n, (real)(c->robin.n_total > 0 ? 1.0 / (double)c->robin.n_total : 0.0), c->tgt.as<real>()};
  else
    return (real)c->nu;
}

// Where a kernel kind is asked for: the training evaluation (eval_loss_grad), the residual over the context's own set
// (pinn_residual), the residual at points that are not the set's (pinn_residual_at; the pool of rad_draw)
enum Where { AT_TRAINING, AT_SET, AT_FOREIGN };

// The template value of the adr kernels that a context of the adr kind (pde 5) runs.  The three places differ on purpose:
//   coefficient fields   have a row per collocation point of the set and none anywhere else: PDE_ADR_VAR never runs at
//                        foreign points (it would index the table and tgt by a point that has no entry).  pinn_residual_at
//                        and pinn_rad_collocation refuse such a context before they get here
//   a source term        is in the same position, but PDE_ADR_SRC has a null form that leaves s out (launch_residual), so a
//                        foreign point gets the operator part N[u].  pinn_rad_collocation refuses a source all the same
//   Robin points         change the training kernels alone, which then walk a fourth point class; a residual is taken at
//                        collocation points, so k_residual has no Robin form.  Training looks at the ASSEMBLED count
//                        (robin.n, ensure_sets), as the kernels' argument does
// Each kind is a superset of the one below it (kernels_generic.h), so the first extra present decides.
static int adr_kind(const pinn_ctx* c, Where w) {
  if (c->kf.on && w != AT_FOREIGN) return PDE_ADR_VAR;
  if (c->src.on) return PDE_ADR_SRC;
  if (c->robin.n > 0 && w == AT_TRAINING) return PDE_ADR_ROBIN;
  return PDE_ADR;
}
// the template value of the continuous kernels for any context that has them (not the discrete-time models)
static int pde_kind(const pinn_ctx* c, Where w) {
  switch (c->pde) {
    case PINN_PDE_BURGERS: return 0;
    case PINN_PDE_BURGERS_IDE: return 1;
    case PINN_PDE_ADR: return adr_kind(c, w);
    case PINN_PDE_ADR_IDE: return PDE_ADR_IDE;
    case PINN_PDE_ADR2: return PDE_ADR2;       // one kind: the wall count may be 0, tgt is zero without a source
    default: return 2;                     // Schrodinger
  }
}
// (dtype of c, kind) as template arguments: calls f(real(), Kind<PDE>()) for the kind pde_kind answered.  A caller whose
// kernels lack one of the kinds says so with an `if constexpr` of its own; nothing here instantiates a kernel
template <int PDE> using Kind = std::integral_constant<int, PDE>;
template <typename F>
__attribute__((always_inline)) static inline int by_kind(const pinn_ctx* c, int kind, F&& f) {
  return by_real(c, [&](auto r) __attribute__((always_inline)) -> int {
    switch (kind) {
      case 0: return f(r, Kind<0>());
      case 1: return f(r, Kind<1>());
      case 2: return f(r, Kind<2>());
      case PDE_ADR: return f(r, Kind<PDE_ADR>());
      case PDE_ADR_IDE: return f(r, Kind<PDE_ADR_IDE>());
      case PDE_ADR_ROBIN: return f(r, Kind<PDE_ADR_ROBIN>());
      case PDE_ADR_SRC: return f(r, Kind<PDE_ADR_SRC>());
      case PDE_ADR_VAR: return f(r, Kind<PDE_ADR_VAR>());
      case PDE_ADR2: return f(r, Kind<PDE_ADR2>());
    }
    return fail(PINN_EINVAL, "no kernel of kind %d", kind);
  });
}

// a source or coefficient fields whose points were replaced: refused in front of every evaluation, nothing launched.  One
// check for both per-collocation-point kinds of value; each is cleared by its own setter
static int src_fresh(const pinn_ctx* c, const char* who) {
  const bool s_stale = c->src.on && c->src.stale, k_stale = c->kf.on && c->kf.stale;
  if (s_stale && k_stale)
    return fail(PINN_ESTATE, "%s: the collocation points were replaced since the source term and the coefficient fields were "
                "set; their values belong to the old points -- call pinn_set_source and pinn_set_coef_fields with values at "
                "the new points (pinn_get_collocation), or with n = 0", who);
  if (k_stale)
    return fail(PINN_ESTATE, "%s: the collocation points were replaced since the coefficient fields were set; their rows belong "
                "to the old points -- call pinn_set_coef_fields with rows at the new points (pinn_get_collocation), or with "
                "n = 0", who);
  if (s_stale)
    return fail(PINN_ESTATE, "%s: the collocation points were replaced since the source term was set; its values belong to the "
                "old points -- call pinn_set_source with values at the new points (pinn_get_collocation), or with n = 0", who);
  return 0;
}
// local collocation count as the next assembly will see it: the one place that turns the origin into a count
static int64_t n_colloc(const pinn_ctx* c) {
  return c->col.from == pinn_ctx::COL_HANDED ? (int64_t)(c->sets.Xf.size() / 2) : c->col.count;
}

// the fused kernel serves width-20 Burgers nets whose staged weights fit the 160 KiB LDS
static bool fused_ok(const pinn_ctx* c) {
  if (!fused20_supported(c->nd) || c->pde == PINN_PDE_SCHRODINGER || is_disc(c) || adr_family(c)) return false;
  const size_t lds = c->dtype == PINN_F64 ? fused20_lds_bytes<double>(c->nd.n_hidden)
                                          : fused20_lds_bytes<float>(c->nd.n_hidden);
  return lds <= 160 * 1024;
}

// the register-stash kernel: float32, width 20, instantiated depths, weights + tiles within LDS
static bool fused_regs_ok(const pinn_ctx* c) {
  return c->dtype == PINN_F32 && fused20_supported(c->nd) && c->pde != PINN_PDE_SCHRODINGER && !is_disc(c) && !adr_family(c) &&
         fused20m_depth_ok(c->nd.n_hidden) && fused20m_lds_bytes(c->nd.n_hidden) <= 160 * 1024;
}

// the float64 register-stash kernel (kernels_fused20d.h): float64, width 20, 8 hidden layers, Burgers problems
static bool fused_f64_ok(const pinn_ctx* c) {
  return c->dtype == PINN_F64 && fused20_supported(c->nd) && c->pde != PINN_PDE_SCHRODINGER && !is_disc(c) &&
         fused20d_depth_ok(c->nd.n_hidden) && fused20d_lds_bytes(c->nd.n_hidden, c->nd.n_theta) <= 160 * 1024;
}

// the wide MFMA sweeps: float32, hidden width 100, two outputs (the Schrodinger net)
static bool wide_ok(const pinn_ctx* c) {
  return c->dtype == PINN_F32 && c->nd.width == 100 && c->nd.n_out == 2 && c->nd.n_hidden == 4 &&
         c->pde == PINN_PDE_SCHRODINGER;
}

// the shape-generic MFMA sweeps (kernels_tile16.h): any width up to 128 (64 in float64), any depth
static bool tile16_ok(const pinn_ctx* c) { return !is_disc(c) && c->nd.width <= 128 && c->nd.n_out <= 2; }
// the fused float64 sweep (kernels_tile16f.h): forward + reverse of a group in one kernel, stash in registers
static bool t16_fused_ok(const pinn_ctx* c) {
  return tile16_ok(c) && c->dtype == PINN_F64 && c->nd.width > 64 && c->nd.n_hidden >= 2 && c->nd.n_hidden <= 4;
}
static bool any_net_ok(const pinn_ctx*) { return true; }

// what the host code has to know about a kernel path; PATHS is indexed by KernelPath, its rows in the order 0..8
enum Stash { STASH_NONE, STASH_CHUNK, STASH_SET };   // the forward sweep's stash in HBM: none, one chunk's, the whole set's
struct PathInfo {
  const char* name;
  Stash stash;
  bool one_launch;                  // one kernel per evaluation, the timing events attached to the launch itself
  bool (*ok)(const pinn_ctx*);      // eligibility, and what pinn_set_kernel_path answers where it fails
  const char* needs;
};
static const PathInfo PATHS[KP_COUNT] = {
    {"generic", STASH_CHUNK, false, any_net_ok, ""},
    {"fused width-20", STASH_SET, true, fused_ok,
     "the fused path needs hidden width 20, a Burgers problem and weights that fit LDS"},
    {"float32 register stash", STASH_NONE, true, fused_regs_ok,
     "the register-stash path needs float32, hidden width 20, 4, 6, 8 or 10 hidden layers and a Burgers problem"},
    {"wide MFMA sweeps", STASH_CHUNK, false, wide_ok, "the wide path needs float32, hidden width 100 and two outputs"},
    // KP_T16 and its two halves
    {"shape-generic MFMA sweeps", STASH_CHUNK, false, tile16_ok, "the shape-generic MFMA sweeps need hidden width <= 128"},
    {"shape-generic MFMA sweeps", STASH_CHUNK, false, tile16_ok, "the shape-generic MFMA sweeps need hidden width <= 128"},
    {"shape-generic MFMA sweeps", STASH_CHUNK, false, tile16_ok, "the shape-generic MFMA sweeps need hidden width <= 128"},
    {"float64 register stash", STASH_NONE, true, fused_f64_ok,
     "the float64 register-stash path needs float64, hidden width 20, 4, 6 or 8 hidden layers and a Burgers problem"},
    // KP_T16_FUSED (no stash: 257 MB at cfg 4 that nothing would touch)
    {"fused float64 MFMA sweep", STASH_NONE, false, t16_fused_ok,
     "the fused float64 sweep needs float64, hidden width 65..128 and 2, 3 or 4 hidden layers"},
};
// default kernel family, fastest first: width-20 f32 (MFMA GEMVs, register stash), its float64 counterpart (4x4x4 MFMA
// GEMVs, no exchange), width-20 HBM-stash, wide MFMA sweeps (width 100, 2 outputs), the fused float64 sweep, the
// shape-generic MFMA sweeps, generic
static const KernelPath PATH_PREFERENCE[] = {KP_FUSED20M, KP_FUSED20D, KP_FUSED20, KP_WIDE, KP_T16_FUSED, KP_T16, KP_GENERIC};
// the adr kind's two implementations
static bool adr_has_path(KernelPath p) { return p == KP_GENERIC || p == KP_FUSED20D; }
static bool path_ok(const pinn_ctx* c, KernelPath p) {
  return PATHS[p].ok(c) && (!adr_family(c) || adr_has_path(p));
}

static bool t16_fwd_on(const pinn_ctx* c) { return c->path == KP_T16 || c->path == KP_T16_FWD; }
static bool t16_bwd_on(const pinn_ctx* c) { return c->path == KP_T16 || c->path == KP_T16_BWD || c->path == KP_T16_FUSED; }
// Launch plan of the shape-generic sweeps for a chunk of `pts` points (measured, profiles/r01_t16_plan.txt):
//   widths <= 64, float32: few groups (<= 3 per CU: every group resident at once) -> weights straight from L2, three
//     workgroups per CU; many groups -> weights staged in LDS, two workgroups per CU;
//   widths <= 64, float64: weights from L2 (the LDS copy would leave room for one workgroup per CU only), two per CU;
//   widths > 64: the eight-wave variants, weights from L2, one workgroup per CU (float64: LDS is full; float32: round 2's
//     four waves with the layer's weights staged in LDS, two per CU, were dropped for it).
static bool t16_lds_weights(const pinn_ctx* c, int pts) {
  if (c->nd.width > 64 || c->dtype == PINN_F64) return false;
  return pts / 16 > 3 * c->n_cu;
}
static int t16_wgs(const pinn_ctx* c, int pts) {
  const int g = pts / 16;
  int per_cu = (c->nd.width <= 64 && c->dtype != PINN_F64 && g <= 3 * c->n_cu) ? 3 : 2;
  // ... but never more workgroups than are resident at once: a persistent grid larger than what the CUs' LDS admits
  // runs in two batches whose group counts round up separately (width 100: 1250 groups on 512 workgroups of which
  // 256 fit = 3 + 3 group times instead of 5).  Widths > 64 take 140-147 KB per workgroup: one per CU.
  const size_t rs = c->dtype == PINN_F64 ? 8 : 4;
  size_t lds;
  if (c->nd.width > 64) {
    lds = t16_fwd_lds<8>(rs, false) > t16_bwd_lds<8>(rs, false) ? t16_fwd_lds<8>(rs, false) : t16_bwd_lds<8>(rs, false);
    per_cu = 1;                                // the eight-wave variants: one workgroup = two waves per SIMD
  } else {
    const bool wl = t16_lds_weights(c, pts);
    lds = t16_fwd_lds<4>(rs, wl) > t16_bwd_lds<4>(rs, wl) ? t16_fwd_lds<4>(rs, wl) : t16_bwd_lds<4>(rs, wl);
  }
  const int fit = (int)((size_t)160 * 1024 / lds) > 0 ? (int)((size_t)160 * 1024 / lds) : 1;
  if (per_cu > fit) per_cu = fit;
  const int cap = per_cu * c->n_cu;
  return g < cap ? g : cap;
}
// persistent workgroups of the wide sweeps for a chunk of `pts` points
static int wide_wgs(const pinn_ctx* c, int pts) { return pts / 16 < c->n_cu ? pts / 16 : c->n_cu; }

// partial gradient rows the path leaves in c->part for the assembled set (c->sd, c->chunk, c->n_rows and c->n_wg as
// ensure_sets set them): what `part` is sized for and what the reduction sums
static int path_rows(const pinn_ctx* c) {
  if (t16_bwd_on(c)) return t16_wgs(c, c->chunk);              // one row per workgroup of a full chunk
  switch (c->path) {
    case KP_WIDE: return wide_wgs(c, c->chunk);
    case KP_FUSED20M: case KP_FUSED20D: return c->n_wg;        // persistent workgroups
    case KP_FUSED20: return fused20_rows(c->sd);
    default: return c->n_rows;                                 // one row per 64 points of a chunk
  }
}

static int upload_real(pinn_ctx* c, void* dst, const double* src, size_t n) {
  if (c->dtype == PINN_F64) {
    HIPCHK(hipMemcpyAsync(dst, src, n * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  } else {
    std::vector<float> tmp(n);
    for (size_t i = 0; i < n; ++i) tmp[i] = (float)src[i];
    HIPCHK(hipMemcpyAsync(dst, tmp.data(), n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  return 0;
}

// device-side Latin hypercube: (re)writes the collocation slots of xs/ts in place (kernels_sampling.h)
static int lhs_fill(pinn_ctx* c) {
  const int64_t cnt = c->col.count;
  if (cnt <= 0) return 0;
  const size_t off = (size_t)colloc_first(c->sd);
  const uint64_t n = (uint64_t)c->col.n_design;
  const uint32_t lo = (uint32_t)c->lhs.seed, hi = (uint32_t)(c->lhs.seed >> 32);
  const InMap<double> m(c->lb, c->ub);
  const dim3 grid((unsigned)((cnt + 255) / 256)), block(256);
  by_real(c, [&](auto r) {
    using real = decltype(r);
    hipLaunchKernelGGL((k_lhs_fill<real>), grid, block, 0, c->stream, c->xs.as<real>() + off, c->ts.as<real>() + off, cnt,
                       (uint64_t)c->col.first, n, lhs_half_bits(n), lo, hi, m.lbx, m.lbt, m.ex, m.et);
  });
  HIPCHK(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------------------------
// training-set assembly: [boundary-lo | boundary-hi | data | collocation | pad]; the adr kind's Robin points, if any, are a
// block of their own between the collocation block and the padding.  SetDesc does not count them (sd.n_all ends the
// collocation block, as every kernel's point classes expect); sd.n_pad covers them.  pointsets.h builds the SetDesc and
// assembles the set; the extras of this context are laid on top here
// ------------------------------------------------------------------------------------------
static int ensure_sets(pinn_ctx* c) {
  if (!c->sets_dirty) return 0;
  const PointSets& ps = c->sets;
  const int n_b = (int)(ps.Xlo.size() / 2), n_u = (int)(ps.Xu.size() / 2), n_f = (int)n_colloc(c);
  const int NO = c->nd.n_out;
  if (c->pde == PINN_PDE_BURGERS_IDE)
    REQUIRE(n_f == 0, "identification evaluates the residual at the data points; no collocation set");
  if (c->pde != PINN_PDE_SCHRODINGER && !adr_family(c)) REQUIRE(n_b == 0, "boundary pairs are Schrodinger-only");
  const int n_w = has_walls(c) ? (int)(c->robin.X.size() / 2) : 0;
  const SetDesc sd = make_set_desc(n_b, n_u, n_f, c->nb_total, c->nu_total, c->nf_total, n_w);
  const int n_all = sd.n_all, n_pad = sd.n_pad;
  REQUIRE(n_all > 0, "no training points set");
  REQUIRE(2 * n_b <= CHUNK_POINTS / 2, "too many boundary pairs for one chunk (%d)", n_b);
  c->sd = sd;

  // the adr family's pairs stand interleaved on every kernel path; a device origin's slots are filled below
  const bool on_device = c->col.from != pinn_ctx::COL_HANDED;
  std::vector<double> hx(n_pad), ht(n_pad), htg((size_t)NO * n_pad);
  assemble_set(ps, sd, NO, adr_family(c), on_device, c->lb, hx.data(), ht.data(), htg.data());
  const size_t off = (size_t)colloc_first(sd);
  if (has_walls(c) && c->src.on && !c->src.stale) {                // s_i rides in tgt at the collocation point's own index
    REQUIRE((int)c->src.s.size() == n_f, "the source term holds %lld values, the collocation set %d points",
            (long long)c->src.s.size(), n_f);
    for (int i = 0; i < n_f; ++i) htg[off + i] = c->src.s[i];
  }
  if (is_adr(c) && c->kf.on && !c->kf.stale)
    REQUIRE((int)(c->kf.K.size() / 6) == n_f, "the coefficient fields hold %lld rows, the collocation set %d points",
            (long long)(c->kf.K.size() / 6), n_f);
  c->robin.first = robin_first(sd); c->robin.n = n_w;
  for (int j = 0, g = robin_first(sd); j < n_w; ++j, ++g) {        // g_j rides in tgt at the point's own index
    hx[g] = c->robin.X[2 * j]; ht[g] = c->robin.X[2 * j + 1];
    htg[g] = c->robin.g[j];
  }
  if (c->col.from == pinn_ctx::COL_RAD && c->rad.filled && n_f > 0) {   // the last adaptive draw, kept through re-assemblies
    HIPCHK(hipMemcpyAsync(hx.data() + off, c->rad.cx, (size_t)n_f * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(ht.data() + off, c->rad.ct, (size_t)n_f * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }

  const size_t rs = real_size(c);
  HIPCHK(c->xs.reserve_bytes(n_pad * rs));
  HIPCHK(c->ts.reserve_bytes(n_pad * rs));
  HIPCHK(c->tgt.reserve_bytes((size_t)NO * n_pad * rs));
  HIPCHK(c->O.reserve_bytes((size_t)NO * n_pad * 4 * rs));
  if (upload_real(c, c->xs, hx.data(), n_pad)) return PINN_EHIP;
  if (upload_real(c, c->ts, ht.data(), n_pad)) return PINN_EHIP;
  if (upload_real(c, c->tgt, htg.data(), (size_t)NO * n_pad)) return PINN_EHIP;
  if (n_w > 0) {
    const int rw = is_adr2(c) ? 4 : 2;             // PDE_ADR2: rows (alpha, beta, gamma, 0), one 16- or 32-byte load each
    std::vector<double> hab((size_t)rw * n_w, 0.0);
    for (int j = 0; j < n_w; ++j) {
      hab[rw * j] = c->robin.alpha[j]; hab[rw * j + 1] = c->robin.beta[j];
      if (rw == 4) hab[rw * j + 2] = c->robin.gamma[j];
    }
    HIPCHK(c->robin.ab.reserve_bytes(hab.size() * rs));
    if (upload_real(c, c->robin.ab, hab.data(), hab.size())) return PINN_EHIP;
  }
  if (is_adr(c) && c->kf.on && !c->kf.stale && n_f > 0) {           // the table, row i for collocation point 2 n_b + n_u + i
    HIPCHK(c->kf.dev.reserve_bytes(c->kf.K.size() * rs));
    if (upload_real(c, c->kf.dev, c->kf.K.data(), c->kf.K.size())) return PINN_EHIP;
  }
  if (c->col.from == pinn_ctx::COL_LHS) { if (int rc = lhs_fill(c)) return rc; }

  c->chunk = n_pad < CHUNK_POINTS ? n_pad : CHUNK_POINTS;
  c->n_rows = c->chunk / 64;
  const size_t W = c->nd.width, H = c->nd.n_hidden;
  c->n_wg = (n_pad / 64 < c->n_cu) ? n_pad / 64 : c->n_cu;   // persistent workgroups (KP_FUSED20M, KP_FUSED20D)
  // the fused kernel keeps the whole set's stash (one launch); the generic path works in chunks
  const Stash stash = PATHS[c->path].stash;
  const size_t stash_pts = stash == STASH_SET ? (size_t)n_pad : (size_t)c->chunk;
  const size_t need_S = stash == STASH_NONE ? 16 : H * W * stash_pts * 4 * rs;
  const size_t need_Z = stash == STASH_NONE ? 16 : W * (size_t)c->chunk * 4 * rs;
  const size_t need_part = (size_t)path_rows(c) * c->R * rs;
  HIPCHK(c->S.reserve_bytes(need_S));
  HIPCHK(c->ZA.reserve_bytes(need_Z));
  HIPCHK(c->ZB.reserve_bytes(need_Z));
  HIPCHK(c->part.reserve_bytes(need_part));
  c->sets_dirty = false;
  return 0;
}

// ------------------------------------------------------------------------------------------
// one loss+gradient evaluation at the current weights -> c->gl  (no host sync)
// ------------------------------------------------------------------------------------------
struct AdamFuse {          // single-GPU Adam step applied by the reduction kernel itself
  double alpha;
  double* loss3;
  double alpha_sa = 0.0;   // self-adaptive weights: the ascent's step size, applied by the evaluation kernel (0: none)
  double bc_pw = 0.0;      // adr point weights: the step's bias-correction factor sqrt(1 - b2^t) / (1 - b1^t) (0: none)
};

// A per-point weight array as the assembled set wants it now: the header as the kernel reads it and the entries per class
// (LamStore).  The two surfaces differ in this and in nothing else.
struct LamLayout {
  int n_hdr;
  double hdr[PW_CONST];
  int n[LAM_CLASSES];
  size_t at(int k) const {                       // first double of class k's entries
    size_t o = (size_t)n_hdr;
    for (int j = 0; j < k; ++j) o += (size_t)3 * n[j];
    return o;
  }
  size_t doubles() const { return at(LAM_CLASSES); }
};
// self-adaptive weights: Adam's constants; data and collocation points
static LamLayout sa_layout(const pinn_ctx* c) {
  return LamLayout{SA_CONST, {c->adam.b1, c->adam.b2, c->adam.eps}, {0, c->sd.n_u, c->sd.n_f}};
}
// adr point weights: the constants, then the ascent rate at 3 + point class (fused20d_api.h).  The pairs are stored
// pair-interleaved, one entry per POINT: a pair counts twice
static LamLayout pw_layout(const pinn_ctx* c) {
  LamLayout L{PW_CONST, {c->adam.b1, c->adam.b2, c->adam.eps}, {2 * c->sd.n_b, c->sd.n_u, c->sd.n_f}};
  L.hdr[3 + CLS_BLO] = c->pw.rate[2]; L.hdr[3 + CLS_DATA] = c->pw.rate[0]; L.hdr[3 + CLS_COL] = c->pw.rate[1];
  return L;
}

// start values: h holds L.doubles() doubles, the entries filled in; the header is written here.  Synchronous.
static int lam_upload(pinn_ctx* c, LamStore& s, const LamLayout& L, std::vector<double>& h) {
  memcpy(h.data(), L.hdr, L.n_hdr * sizeof(double));
  HIPCHK(s.buf.reserve(h.size()));
  HIPCHK(hipMemcpyAsync(s.buf, h.data(), h.size() * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  for (int k = 0; k < LAM_CLASSES; ++k) { s.n[k] = L.n[k]; s.reset[k] = false; }
  s.n_hdr = L.n_hdr;
  memcpy(s.hdr, L.hdr, sizeof s.hdr);
  return 0;
}

// the array as the device holds it, in the layout it was uploaded with.  Synchronous.
static int lam_download(pinn_ctx* c, const LamStore& s, std::vector<double>& h) {
  h.resize((size_t)s.n_hdr + (size_t)3 * s.n[0] + (size_t)3 * s.n[1] + (size_t)3 * s.n[2]);
  HIPCHK(hipMemcpyAsync(h.data(), s.buf, h.size() * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

// (Re)build the device array for the assembled set when a class's set was replaced (its weights back to 1, its moments to 0;
// the other classes keep theirs), or rewrite its header alone when only the ascent's constants or rates changed.
// Synchronous, and only then: the common case returns at once.
static int lam_prepare(pinn_ctx* c, LamStore& s, const LamLayout& L) {
  bool keep[LAM_CLASSES], keep_all = true, keep_any = false;
  for (int k = 0; k < LAM_CLASSES; ++k) {
    keep[k] = s.buf && !s.reset[k] && s.n[k] == L.n[k];
    keep_all = keep_all && keep[k];
    keep_any = keep_any || (keep[k] && L.n[k] > 0);
  }
  if (keep_all) {
    if (memcmp(L.hdr, s.hdr, sizeof s.hdr) == 0) return 0;
    HIPCHK(hipMemcpyAsync(s.buf, L.hdr, L.n_hdr * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    memcpy(s.hdr, L.hdr, sizeof s.hdr);
    return 0;
  }
  std::vector<double> old;
  if (keep_any) { if (int rc = lam_download(c, s, old)) return rc; }
  std::vector<double> h(L.doubles(), 0.0);
  size_t from = (size_t)s.n_hdr;                   // class k's entries in the old layout
  for (int k = 0; k < LAM_CLASSES; ++k) {
    double* const to = h.data() + L.at(k);
    for (size_t i = 0; i < (size_t)3 * L.n[k]; ++i) to[i] = keep[k] ? old[from + i] : (i % 3 == 0 ? 1.0 : 0.0);
    from += (size_t)3 * s.n[k];
  }
  return lam_upload(c, s, L, h);
}

// k_t16_fused (KP_T16_FUSED) leaves the hidden-layer weight gradients in its tile-major scratch: the reductions read them there
static TileScratch tile_scratch(const pinn_ctx* c) {
  TileScratch ts{};
  if (c->path != KP_T16_FUSED || c->dtype != PINN_F64 || !c->t16_gscr) return ts;
  const int W = c->nd.width, ntl = (W + 15) / 16;
  ts.gscr = c->t16_gscr;
  ts.n_tiles = ntl * ntl; ts.ntl = ntl; ts.W = W;
  ts.n_slots = (c->nd.n_hidden - 1) * ts.n_tiles;
  ts.stride = (long long)ts.n_slots * 256;
  ts.edge = t16_deal(W).edge;
  ts.off_w1 = c->nd.off_w[1];
  ts.pitch = W * W + W;
  return ts;
}

// grid of k_reduce_xgmi: one workgroup per 64 columns (+ one per scratch slot), capped when ranks share the device
static dim3 xg_grid(const pinn_ctx* c, int R, int n_slots = 0) {
  const int n_cb = (R + RED_COLS - 1) / RED_COLS + n_slots;
  return dim3((unsigned)((c->xg.grid_cap > 0 && c->xg.grid_cap < n_cb) ? c->xg.grid_cap : n_cb));
}

// deterministic sum of the per-workgroup gradient rows -> c->gl (f64), optionally with the Adam step behind it
template <typename real>
static int launch_reduce(pinn_ctx* c, int n_rows, const AdamFuse* af) {
  const TileScratch ts = tile_scratch(c);
  const dim3 rgrid((c->R + RED_COLS - 1) / RED_COLS + (ts.gscr ? ts.n_slots : 0));
  if (c->xg.on) {   // rows -> vector -> every peer's mailbox -> sum over ranks (-> Adam), one launch
    if (++c->xg.seq == 0) c->xg.seq = 2;          // 32-bit wrap: skip 0, keep the parity alternating
    const unsigned int seq = c->xg.seq;
    const dim3 xgrid = xg_grid(c, c->R, ts.gscr ? ts.n_slots : 0);
    if (af)
      hipLaunchKernelGGL((k_reduce_xgmi<real, true>), xgrid, dim3(RED_THREADS), 0, c->stream, c->part.as<real>(),
                         n_rows, c->R, c->gl, c->xg.peers, seq, XG_TIMEOUT_TICKS, c->xg.err, c->nd.n_theta, c->theta,
                         c->theta_r.as<real>(), c->adam_m, c->adam_v, af->alpha, c->adam.b1, c->adam.b2, c->adam.eps, af->loss3, c->nd,
                         c->img, ts);
    else
      hipLaunchKernelGGL((k_reduce_xgmi<real, false>), xgrid, dim3(RED_THREADS), 0, c->stream, c->part.as<real>(),
                         n_rows, c->R, c->gl, c->xg.peers, seq, XG_TIMEOUT_TICKS, c->xg.err, 0, (double*)nullptr,
                         (real*)nullptr, (double*)nullptr, (double*)nullptr, 0.0, 0.0, 0.0, 0.0, (double*)nullptr,
                         c->nd, (float*)nullptr, ts);
    HIPCHK(hipGetLastError());
    return 0;
  }
  if (af)
    hipLaunchKernelGGL((k_reduce_adam<real>), rgrid, dim3(RED_THREADS), 0, c->stream, c->part.as<real>(),
                       n_rows, c->R, c->gl, c->nd.n_theta, c->theta, c->theta_r.as<real>(), c->adam_m,
                       c->adam_v, af->alpha, c->adam.b1, c->adam.b2, c->adam.eps, af->loss3, c->nd, c->img, c->n_evals,
                       c->d_nonfinite, ts);
  else
    hipLaunchKernelGGL((k_reduce_rows<real>), rgrid, dim3(RED_THREADS), 0, c->stream, c->part.as<real>(),
                       n_rows, c->R, c->gl, c->nd.n_theta, c->n_evals, c->d_nonfinite, ts);
  HIPCHK(hipGetLastError());
  return 0;
}

// shape-generic MFMA sweeps for one chunk (kernels_tile16.h)
template <typename real, int NT, bool WLDS>
static int t16_launch_fwd(pinn_ctx* c, const void* xs, const void* ts, int n_pad, int chunk, void* O, int base, int pts,
                          real lbx, real lbt, real sx, real st) {
  static unsigned long long attr = 0;
  // eight waves per workgroup where LDS admits one workgroup per CU only (widths above 64): two waves per SIMD
  constexpr int NWV = (NT == 8 && !WLDS) ? 8 : 4;
  const size_t lds = t16_fwd_lds<NT>(sizeof(real), WLDS, NWV);
  if (first_call_on_device(attr))
    HIPCHK(hipFuncSetAttribute((const void*)k_t16_fwd<real, NT, WLDS, NWV>, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)lds));
  hipLaunchKernelGGL((k_t16_fwd<real, NT, WLDS, NWV>), dim3(t16_wgs(c, pts)), dim3(64 * NWV), lds, c->stream, c->nd,
                     c->theta_r.as<real>(), (const real*)xs, (const real*)ts, base, n_pad, chunk,
                     pts / 16, lbx, lbt, sx, st, c->S.as<vec4<real>>(), (vec4<real>*)O);
  return 0;
}
template <typename real, int NT, int PDE, bool WLDS>
static int t16_launch_bwd(pinn_ctx* c, int base, int pts, real lbx, real lbt, real sx, real st, int accumulate) {
  static unsigned long long attr = 0;
  constexpr int NWV = (NT == 8 && !WLDS) ? 8 : 4;
  const size_t lds = t16_bwd_lds<NT>(sizeof(real), WLDS);
  if (first_call_on_device(attr))
    HIPCHK(hipFuncSetAttribute((const void*)k_t16_bwd<real, NT, PDE, WLDS, NWV>, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)lds));
  // one partial row per workgroup: never launch more workgroups than the rows sized for a full chunk (t16_wgs is
  // not monotone in pts: a short last chunk may prefer three workgroups per CU where the full chunk took two)
  const int rows_cap = t16_wgs(c, c->chunk);
  const int wgs = t16_wgs(c, pts) < rows_cap ? t16_wgs(c, pts) : rows_cap;
  hipLaunchKernelGGL((k_t16_bwd<real, NT, PDE, WLDS, NWV>), dim3(wgs), dim3(64 * NWV), lds, c->stream, c->nd, c->sd,
                     c->theta_r.as<real>(), c->xs.as<real>(), c->ts.as<real>(), c->tgt.as<real>(), base,
                     c->sd.n_pad, c->chunk, pts / 16, lbx, lbt, sx, st, (real)c->nu, c->S.as<vec4<real>>(),
                     c->O.as<vec4<real>>(), c->part.as<real>(), c->R, accumulate);
  return 0;
}
template <typename real>
static int t16_fwd(pinn_ctx* c, const void* xs, const void* ts, int n_pad, int chunk, void* O, int base, int pts,
                   real lbx, real lbt, real sx, real st) {
  // widths up to 64: four feature tiles; up to 128: eight (the weights then stay in L2)
  if (c->nd.width > 64)
    return t16_launch_fwd<real, 8, false>(c, xs, ts, n_pad, chunk, O, base, pts, lbx, lbt, sx, st);
  if (!t16_lds_weights(c, pts))
    return t16_launch_fwd<real, 4, false>(c, xs, ts, n_pad, chunk, O, base, pts, lbx, lbt, sx, st);
  return t16_launch_fwd<real, 4, true>(c, xs, ts, n_pad, chunk, O, base, pts, lbx, lbt, sx, st);
}
// plain forward sweep of one chunk for pinn_predict / pinn_residual: the MFMA sweep for nets wide enough to profit
template <typename real>
static int forward_chunk(pinn_ctx* c, const void* xs, const void* ts, int n_pad, int chunk, void* O, int base, int pts) {
  const InMap<real> m(c->lb, c->ub);
  constexpr int JT2 = sizeof(real) == 4 ? 20 : 10;
  if (is_adr2(c)) {                              // the fourth channel carries kappa: this kind's own sweep, whatever the width
    hipLaunchKernelGGL((k_forward_adr2<real, JT2>), dim3(pts / 64), dim3(64), 0, c->stream, c->nd, c->theta_r.as<real>(),
                       (const real*)xs, (const real*)ts, base, n_pad, chunk, m.lbx, m.lbt, m.sx, m.st, c->S.as<vec4<real>>(),
                       (vec4<real>*)O, (real)c->adr[7]);
    return 0;
  }
  if (tile16_ok(c) && c->nd.width >= 24)
    return t16_fwd<real>(c, xs, ts, n_pad, chunk, O, base, pts, m.lbx, m.lbt, m.sx, m.st);
  constexpr int JT = sizeof(real) == 4 ? 20 : 10;
  hipLaunchKernelGGL((k_forward<real, JT>), dim3(pts / 64), dim3(64), 0, c->stream, c->nd, c->theta_r.as<real>(),
                     (const real*)xs, (const real*)ts, base, n_pad, chunk, m.lbx, m.lbt, m.sx, m.st, c->S.as<vec4<real>>(),
                     (vec4<real>*)O);
  return 0;
}

template <typename real, int PDE>
static int t16_bwd(pinn_ctx* c, int base, int pts, real lbx, real lbt, real sx, real st, int accumulate) {
  if (c->nd.width > 64)
    return t16_launch_bwd<real, 8, PDE, false>(c, base, pts, lbx, lbt, sx, st, accumulate);
  if (!t16_lds_weights(c, pts))
    return t16_launch_bwd<real, 4, PDE, false>(c, base, pts, lbx, lbt, sx, st, accumulate);
  return t16_launch_bwd<real, 4, PDE, true>(c, base, pts, lbx, lbt, sx, st, accumulate);
}

template <int PDE, int H>
static int t16_fused_launch(pinn_ctx* c, const SetDesc& sd, int base, int pts, int ci, int wgs, int n_bg, double lbx,
                            double lbt, double sx, double st) {
  static unsigned long long attr = 0;
  if (first_call_on_device(attr))
    HIPCHK(hipFuncSetAttribute((const void*)k_t16_fused<PDE, H>, hipFuncAttributeMaxDynamicSharedMemorySize,
                               160 * 1024));
  hipLaunchKernelGGL((k_t16_fused<PDE, H>), dim3(wgs), dim3(512), t16_fused_lds(c->nd.width, H, c->nd.n_out), c->stream, c->nd, sd,
                     c->theta_r.as<double>(), c->xs.as<double>(), c->ts.as<double>(), c->tgt.as<double>(), base,
                     sd.n_pad, pts / 16, lbx, lbt, sx, st, (double)c->nu, c->O.as<vec4<double>>(), c->part.as<double>(), c->R,
                     ci > 0 ? 1 : 0, c->t16_bsync, c->t16_bcount, n_bg, c->t16_gscr, c->t16_handover_ticks,
                     t16_deal(c->nd.width, c->t16_cost_full, c->t16_cost_strip));
  HIPCHK(hipGetLastError());
  return 0;
}

// what every k_fused20d launch of context c takes (fused20d_api.h): the solo plan on c's set and weights.  An ensemble
// overrides the weights, the rows, the member count and, with per-member sets, the points.
static F20dLaunch fused20d_args(const pinn_ctx* c, hipEvent_t* ev4) {
  const InMap<double> m(c->lb, c->ub);
  return F20dLaunch{c->nd, c->sd, c->theta_r.as<double>(), c->xs.as<double>(), c->ts.as<double>(),
                    c->tgt.as<double>(), m.lbx, m.lbt, m.sx, m.st, c->part.as<double>(), c->R, c->n_wg, 1, c->row_index,
                    c->stream, c->stamps, ev4 ? ev4[0] : nullptr, ev4 ? ev4[1] : nullptr};
}

// Whether the next evaluation of c takes the split one-tile launch of path 7 (k_split20d, fused20d_api.h): 1 yes, 0 no,
// -1 PINN_F64_SPLIT=1 asks for it where the kernel exists but the tile count does not fit.  The kernel exists for a solo
// float64 context of the Burgers kinds on path 7 without point weights (ensembles launch through ens_eval, which never
// splits); the tile count fits when every tile has a workgroup of its own and the helpers -- one per pair of tiles -- find
// compute units beside them.  Needs c->sd and c->n_wg (ensure_sets).
static int split_plan(const pinn_ctx* c) {
  if (!fused20d_split_built() || c->f64_split == 0) return 0;
  if (c->path != KP_FUSED20D || c->dtype != PINN_F64 || !c->own_stream) return 0;
  if ((c->pde != PINN_PDE_BURGERS && c->pde != PINN_PDE_BURGERS_IDE) || c->sa.on || c->pw.on) return 0;
  const int n_tiles = c->sd.n_pad / 64;
  const bool fits = n_tiles > 0 && c->n_wg >= n_tiles && fused20d_split_grid(n_tiles) <= c->n_cu;
  return fits ? 1 : c->f64_split == 1 ? -1 : 0;
}

// KP_FUSED20D: the plain, the weighted (self-adaptive) or the adr evaluation, one launch
template <typename real, int PDE>
static int launch_fused20d(pinn_ctx* c, hipEvent_t* ev4, const AdamFuse* af) {
  int rc = hipErrorInvalidValue;
  if constexpr (sizeof(real) == 8 && PDE != 2) {
    const bool weighted = PDE == 0 && c->sa.on;     // an Adam step moves the weights too
    if (weighted) { if (int e = lam_prepare(c, c->sa.arr, sa_layout(c))) return e; }
    const bool pw = PDE == PDE_ADR && c->pw.on;      // the adr kind's point weights; an Adam step moves them too
    if (pw) { if (int e = lam_prepare(c, c->pw.arr, pw_layout(c))) return e; }
    F20dLaunch a = fused20d_args(c, ev4);
    if constexpr (PDE == 0 || PDE == 1) {
      const int sp = split_plan(c);
      if (sp < 0)
        return fail(PINN_EUNSUPPORTED, "PINN_F64_SPLIT=1: %d tiles need %d workgroups, this device has %d compute units",
                    c->sd.n_pad / 64, fused20d_split_grid(c->sd.n_pad / 64), c->n_cu);
      a.split = sp == 1;
    }
    if (pw) rc = fused20d_launch_any(a, AdrPwArgs{pde_coef<double, PDE_ADR>(c), c->pw.arr.buf, af ? af->bc_pw : 0.0});
    else if constexpr (pde_is_adr(PDE)) rc = fused20d_launch_any(a, pde_coef<double, PDE>(c));
    else if (weighted) rc = fused20d_launch_any(a, SaArgs{(double)c->nu, c->sa.arr.buf, af ? af->alpha_sa : 0.0});
    else rc = fused20d_launch_any(PDE, a, (double)c->nu);
  }
  if (rc) return fail(PINN_EHIP, "fused20d launch failed: %s", hipGetErrorString((hipError_t)rc));
  return 0;
}

// KP_FUSED20M: one launch; depth 8 is instantiated here, depths 4, 6 and 10 in fused20m_unit.hip
template <typename real, int PDE>
static int launch_fused20m(pinn_ctx* c, hipEvent_t* ev4) {
  int rc = hipErrorInvalidValue;
  if constexpr (sizeof(real) == 4 && PDE != 2 && !pde_is_adr(PDE)) {
    const InMap<float> m(c->lb, c->ub);
    hipEvent_t const e0 = ev4 ? ev4[0] : nullptr, e1 = ev4 ? ev4[1] : nullptr;
    if (c->nd.n_hidden == 8)
      rc = fused20m_launch<PDE, 8>(c->nd, c->sd, c->theta_r.as<float>(), c->img, c->xs.as<float>(),
                                   c->ts.as<float>(), c->tgt.as<float>(), m.lbx, m.lbt, m.sx, m.st, (float)c->nu,
                                   c->part.as<float>(), c->R, c->n_wg, c->stream, c->stamps, e0, e1);
    else
      rc = fused20m_launch_depth(PDE, c->nd, c->sd, c->theta_r.as<float>(), c->img, c->xs.as<float>(),
                                 c->ts.as<float>(), c->tgt.as<float>(), m.lbx, m.lbt, m.sx, m.st, (float)c->nu,
                                 c->part.as<float>(), c->R, c->n_wg, c->stream, c->stamps, e0, e1);
  }
  if (rc) return fail(PINN_EHIP, "fused20m launch failed: %s", hipGetErrorString((hipError_t)rc));
  return 0;
}

// KP_FUSED20: one launch, the whole set's stash in HBM
template <typename real, int PDE>
static int launch_fused20(pinn_ctx* c, hipEvent_t* ev4) {
  int rc = hipErrorInvalidValue;
  if constexpr (!pde_is_adr(PDE)) {
    const InMap<real> m(c->lb, c->ub);
    rc = fused20_launch<real, PDE>(c->nd, c->sd, c->theta_r.as<real>(), c->xs.as<real>(), c->ts.as<real>(),
                                   c->tgt.as<real>(), m.lbx, m.lbt, m.sx, m.st, (real)c->nu, c->S.as<vec4<real>>(),
                                   c->part.as<real>(), c->R, c->stream, c->stamps, ev4 ? ev4[0] : nullptr,
                                   ev4 ? ev4[1] : nullptr);
  }
  if (rc) return fail(PINN_EHIP, "fused20 launch failed: %s", hipGetErrorString((hipError_t)rc));
  return 0;
}

// KP_T16_FUSED, chunk ci = points [base, base + pts): forward + reverse in one kernel.  ev1 (first chunk, timing on) is
// recorded in front of the kernel, behind a pre-pass.
template <typename real, int PDE>
static int chunk_t16_fused(pinn_ctx* c, const InMap<real>& m, hipEvent_t ev1, int base, int pts, int ci) {
  if constexpr (sizeof(real) == 8 && !pde_is_adr(PDE)) {
    const SetDesc& sd = c->sd;
    const int rows_cap = t16_wgs(c, c->chunk);
    const int wgs = t16_wgs(c, pts) < rows_cap ? t16_wgs(c, pts) : rows_cap;
    // periodic-boundary seeds read the outputs of a partner point another workgroup may own.  The boundary points
    // fill the first groups of the set: when each of them is the first group of its workgroup the kernel hands
    // the outputs over itself (kernels_tile16f.h); otherwise a forward sweep over those groups runs first
    int n_bg = (PDE == 2 && base == 0 && sd.n_b > 0) ? (2 * sd.n_b + 15) / 16 : 0;
    // the kernel's direct-store mode writes every entry of a fresh partial row exactly once, from the workgroup
    // that owns the row: every launched workgroup must own a group, and chunk 0 must fill all rows_cap rows
    REQUIRE(wgs >= 1 && wgs <= pts / 16 && (ci > 0 || wgs == rows_cap),
            "k_t16_fused launch plan: %d workgroups for %d groups (rows %d, chunk %d)", wgs, pts / 16, rows_cap, ci);
    if (n_bg > wgs || (n_bg > 0 && c->t16_prepass)) {
      const size_t need_S = (size_t)c->nd.n_hidden * c->nd.width * (size_t)c->chunk * 4 * sizeof(double);   // (k_t16_fwd stashes)
      HIPCHK(c->S.reserve_bytes(need_S));
      if (int rc = t16_fwd<real>(c, c->xs, c->ts, sd.n_pad, c->chunk, c->O, 0, 16 * n_bg < pts ? 16 * n_bg : pts, m.lbx, m.lbt, m.sx, m.st)) return rc;
      n_bg = 0;
    }
    if (!c->t16_bsync) {
      HIPCHK(c->t16_bsync.reserve(16));
      HIPCHK(hipMemsetAsync(c->t16_bsync, 0, 64, c->stream));
      c->t16_bcount = 0;
    }
    c->t16_bcount += (unsigned int)n_bg;
    {  // tile-major scratch of the hidden-layer weight gradients: one block per workgroup (kernels_tile16f.h)
      const size_t ntl = ((size_t)c->nd.width + 15) / 16;
      const size_t need = (size_t)rows_cap * (c->nd.n_hidden - 1) * ntl * ntl * 256 * sizeof(double);
      HIPCHK(c->t16_gscr.reserve_bytes(need));
    }
    if (ev1) HIPCHK(hipEventRecord(ev1, c->stream));
    switch (c->nd.n_hidden) {            // the stash is a register array: the depth is a template parameter
      case 2: return t16_fused_launch<PDE, 2>(c, sd, base, pts, ci, wgs, n_bg, m.lbx, m.lbt, m.sx, m.st);
      case 3: return t16_fused_launch<PDE, 3>(c, sd, base, pts, ci, wgs, n_bg, m.lbx, m.lbt, m.sx, m.st);
      case 4: return t16_fused_launch<PDE, 4>(c, sd, base, pts, ci, wgs, n_bg, m.lbx, m.lbt, m.sx, m.st);
    }
  }
  return PINN_EINVAL;
}

// forward half of a chunk -> stash c->S, outputs c->O: the shape-generic MFMA sweep, the wide one or one lane per point
template <typename real>
static int chunk_fwd(pinn_ctx* c, const InMap<real>& m, int base, int pts) {
  const int n_pad = c->sd.n_pad;
  if (t16_fwd_on(c)) return t16_fwd<real>(c, c->xs, c->ts, n_pad, c->chunk, c->O, base, pts, m.lbx, m.lbt, m.sx, m.st);
  if constexpr (sizeof(real) == 4) {
    if (c->path == KP_WIDE) {
      static unsigned long long attr = 0;
      if (first_call_on_device(attr))
        HIPCHK(hipFuncSetAttribute((const void*)k_wide_fwd<100, 2>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)wide_lds_bytes<100>()));
      hipLaunchKernelGGL((k_wide_fwd<100, 2>), dim3(wide_wgs(c, pts)), dim3(256), wide_lds_bytes<100>(), c->stream, c->nd,
                         c->theta_r.as<float>(), c->img, c->xs.as<float>(), c->ts.as<float>(), base, n_pad,
                         c->chunk, pts / 16, m.lbx, m.lbt, m.sx, m.st, c->S.as<vec4<float>>(), c->O.as<vec4<float>>());
      return 0;
    }
  }
  constexpr int JT = sizeof(real) == 4 ? 20 : 10;
  hipLaunchKernelGGL((k_forward<real, JT>), dim3(pts / 64), dim3(64), 0, c->stream, c->nd, c->theta_r.as<real>(),
                     c->xs.as<real>(), c->ts.as<real>(), base, n_pad, c->chunk, m.lbx, m.lbt, m.sx, m.st,
                     c->S.as<vec4<real>>(), c->O.as<vec4<real>>());
  return 0;
}

// reverse half of a chunk: its partial gradient rows written to (accumulate = 0) or added to c->part
template <typename real, int PDE>
static int chunk_bwd(pinn_ctx* c, const InMap<real>& m, int base, int pts, int accumulate) {
  const SetDesc& sd = c->sd;
  if constexpr (!pde_is_adr(PDE)) {
    if (t16_bwd_on(c)) return t16_bwd<real, PDE>(c, base, pts, m.lbx, m.lbt, m.sx, m.st, accumulate);
  }
  if constexpr (sizeof(real) == 4 && PDE == 2) {
    if (c->path == KP_WIDE) {
      static unsigned long long attr = 0;
      if (first_call_on_device(attr))
        HIPCHK(hipFuncSetAttribute((const void*)k_wide_bwd<100, 2, 2, 4>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)wide_lds_bytes<100>()));
      hipLaunchKernelGGL((k_wide_bwd<100, 2, 2, 4>), dim3(wide_wgs(c, pts)), dim3(256), wide_lds_bytes<100>(), c->stream,
                         c->nd, sd, c->theta_r.as<float>(), c->img, c->xs.as<float>(), c->ts.as<float>(),
                         c->tgt.as<float>(), base, sd.n_pad, c->chunk, pts / 16, m.lbx, m.lbt, m.sx, m.st, (float)c->nu,
                         c->S.as<vec4<float>>(), c->O.as<vec4<float>>(), c->part.as<float>(), c->R, accumulate);
      return 0;
    }
  }
  constexpr int KT = sizeof(real) == 4 ? 10 : 5;
  hipLaunchKernelGGL((k_backward<real, PDE, KT>), dim3(pts / 64), dim3(64), 0, c->stream, c->nd, sd,
                     c->theta_r.as<real>(), c->xs.as<real>(), c->ts.as<real>(), c->tgt.as<real>(), base, sd.n_pad,
                     c->chunk, m.lbx, m.lbt, m.sx, m.st, pde_coef<real, PDE>(c), c->S.as<vec4<real>>(),
                     c->O.as<vec4<real>>(), c->ZA.as<vec4<real>>(), c->ZB.as<vec4<real>>(), c->part.as<real>(), c->R, accumulate);
  return 0;
}

// the chunked paths: chunk after chunk on the stream, the first chunk's rows written, the later ones' added
template <typename real, int PDE>
static int launch_chunks(pinn_ctx* c, hipEvent_t* ev4) {
  const InMap<real> m(c->lb, c->ub);
  const int n_pad = c->sd.n_pad;
  for (int base = 0, ci = 0; base < n_pad; base += c->chunk, ++ci) {
    const int pts = (n_pad - base < c->chunk) ? n_pad - base : c->chunk;
    hipEvent_t const ev1 = (ev4 && ci == 0) ? ev4[1] : nullptr;       // between the halves of the first chunk
    if (c->path == KP_T16_FUSED) {
      if (int rc = chunk_t16_fused<real, PDE>(c, m, ev1, base, pts, ci)) return rc;
    } else {
      if (int rc = chunk_fwd<real>(c, m, base, pts)) return rc;
      if (ev1) HIPCHK(hipEventRecord(ev1, c->stream));
      if (int rc = chunk_bwd<real, PDE>(c, m, base, pts, ci > 0 ? 1 : 0)) return rc;
    }
  }
  return 0;
}

// PDE_ADR2: one launch of k_adr2_20d on path 7 (float64); on path 0 chunk after chunk, k_forward_adr2 and
// k_backward<real, PDE_ADR2>
template <typename real>
static int launch_adr2(pinn_ctx* c, hipEvent_t* ev4) {
  if (c->path == KP_FUSED20D) {
    int rc = hipErrorInvalidValue;
    if constexpr (sizeof(real) == 8) rc = adr2_20d_launch_any(fused20d_args(c, ev4), pde_coef<double, PDE_ADR2>(c));
    if (rc) return fail(PINN_EHIP, "adr2_20d launch failed: %s", hipGetErrorString((hipError_t)rc));
    return 0;
  }
  if (c->path != KP_GENERIC) return fail(PINN_EUNSUPPORTED, "the adr2 kind (pde 10) runs on kernel paths 0 and 7 only");
  const InMap<real> m(c->lb, c->ub);
  const int n_pad = c->sd.n_pad;
  constexpr int KT = sizeof(real) == 4 ? 10 : 5;
  for (int base = 0, ci = 0; base < n_pad; base += c->chunk, ++ci) {
    const int pts = (n_pad - base < c->chunk) ? n_pad - base : c->chunk;
    if (int rc = forward_chunk<real>(c, c->xs, c->ts, n_pad, c->chunk, c->O, base, pts)) return rc;
    if (ev4 && ci == 0) HIPCHK(hipEventRecord(ev4[1], c->stream));
    hipLaunchKernelGGL((k_backward<real, PDE_ADR2, KT>), dim3(pts / 64), dim3(64), 0, c->stream, c->nd, c->sd,
                       c->theta_r.as<real>(), c->xs.as<real>(), c->ts.as<real>(), c->tgt.as<real>(), base, n_pad, c->chunk,
                       m.lbx, m.lbt, m.sx, m.st, pde_coef<real, PDE_ADR2>(c), c->S.as<vec4<real>>(), c->O.as<vec4<real>>(),
                       c->ZA.as<vec4<real>>(), c->ZB.as<vec4<real>>(), c->part.as<real>(), c->R, ci > 0 ? 1 : 0);
  }
  return 0;
}

// events of a sampled evaluation: [0] start, [1] forward done, [2] sweeps done; the one-launch paths attach [0] and [1] to
// their kernel (its own begin and end).  Out of line: each (dtype, kind) is a function of its own behind eval_loss_grad's
// switch, so a step walks the code of its own kind and not one body that holds all sixteen
template <typename real, int PDE>
__attribute__((noinline)) static int launch_sweeps(pinn_ctx* c, hipEvent_t* ev4, const AdamFuse* af) {
  if (ev4 && !PATHS[c->path].one_launch) HIPCHK(hipEventRecord(ev4[0], c->stream));
  int rc;
  if constexpr (PDE == PDE_ADR2) rc = launch_adr2<real>(c, ev4);
  else switch (c->path) {
    case KP_FUSED20D: rc = launch_fused20d<real, PDE>(c, ev4, af); break;
    case KP_FUSED20M: rc = launch_fused20m<real, PDE>(c, ev4); break;
    case KP_FUSED20: rc = launch_fused20<real, PDE>(c, ev4); break;
    default: rc = launch_chunks<real, PDE>(c, ev4); break;
  }
  if (rc) return rc;
  if (ev4) HIPCHK(hipEventRecord(ev4[2], c->stream));
  return launch_reduce<real>(c, path_rows(c), af);
}

// ------------------------------------------------------------------------------------------
// discrete-time models: stage-set assembly and the four-launch evaluation (kernels_disc.h)
// ------------------------------------------------------------------------------------------
static int disc_layout(pinn_ctx* c, DiscDesc& dd, int n_groups, int q) {
  dd.n_groups = n_groups; dd.n_pad = 16 * n_groups;
  dd.ldo = (c->nd.n_out + 63) / 64 * 64; dd.n_chunks = dd.ldo / 64;
  dd.q = q; dd.wp = (c->nd.width + 63) / 64 * 64;
  dd.identify = c->pde == PINN_PDE_BURGERS_DISC_IDE ? 1 : 0;
  return 0;
}

static int disc_upload_tables(pinn_ctx* c, int ldo) {
  const size_t rs = real_size(c);
  const int NO = c->nd.n_out;
  for (int s = 0; s < 2; ++s) {
    c->d_M[s].reset();                       // freed every time: an empty buffer tells the kernels that the set has no table
    c->d_MT[s].reset();
    const pinn_ctx::DiscSet& ds = c->dset[s];
    if (!ds.has_M || ds.x.empty()) continue;
    std::vector<double> Mp((size_t)ldo * ldo, 0.0), MTp((size_t)ldo * ldo, 0.0);
    for (int j = 0; j < NO; ++j)
      for (int k = 0; k < ds.q; ++k) {
        const double v = ds.M[(size_t)j * ds.q + k];
        Mp[(size_t)j * ldo + k] = v;
        MTp[(size_t)k * ldo + j] = v;
      }
    HIPCHK(c->d_M[s].reserve_bytes(Mp.size() * rs));
    HIPCHK(c->d_MT[s].reserve_bytes(Mp.size() * rs));
    if (upload_real(c, c->d_M[s], Mp.data(), Mp.size()) || upload_real(c, c->d_MT[s], MTp.data(), MTp.size()))
      return PINN_EHIP;
  }
  return 0;
}

static int disc_dk(const pinn_ctx* c);
static int disc_alloc_scratch(pinn_ctx* c, const DiscDesc& dd, DevBuf<void>* Ast, DevBuf<void>* A3, DevBuf<void>& U3,
                              DevBuf<void>& Nn, DevBuf<void>& Rb) {
  const size_t rs = real_size(c), H = c->nd.n_hidden, NC = disc_nc(disc_dk(c));     // Taylor channels of the kind
  if (Ast) HIPCHK(Ast->reserve_bytes(H * NC * (size_t)dd.n_pad * dd.wp * rs));
  if (A3) HIPCHK(A3->reserve_bytes(NC * (size_t)dd.n_pad * dd.wp * rs));
  HIPCHK(U3.reserve_bytes(NC * (size_t)dd.n_pad * dd.ldo * rs));
  HIPCHK(Nn.reserve_bytes((size_t)dd.n_pad * dd.ldo * rs));
  HIPCHK(Rb.reserve_bytes((size_t)dd.n_pad * dd.ldo * rs));
  return 0;
}

static int disc_ensure(pinn_ctx* c) {
  if (!c->sets_dirty) return 0;
  const int n0 = (int)c->dset[0].x.size(), n1 = (int)c->dset[1].x.size();
  const int np = has_pairs(c) ? (int)c->dper.lb.size() : 0;     // periodic pairs: any subset of the three slots may be present
  REQUIRE(n0 + n1 + np > 0, "no stage set given (pinn_disc_set_stage)");
  int q = 0;
  for (int s = 0; s < 2; ++s)
    if (!c->dset[s].x.empty() && c->dset[s].has_M) {
      REQUIRE(q == 0 || q == c->dset[s].q, "the two stage sets use different q (%d vs %d)", q, c->dset[s].q);
      q = c->dset[s].q;
    }
  const int G0 = (n0 + 15) / 16, G1 = (n1 + 15) / 16, Gp = (np + 7) / 8, G = G0 + G1 + Gp;
  DiscDesc dd{};
  disc_layout(c, dd, G, q);
  std::vector<double> hx(dd.n_pad, c->lb[0]), ht(dd.n_pad, 0.0);
  std::vector<int> gi(G);
  int g = 0;
  for (int s = 0; s < 2; ++s) {
    const std::vector<double>& x = c->dset[s].x;
    const int n = (int)x.size();
    for (int b = 0; b < n; b += 16, ++g) {
      const int nv = n - b < 16 ? n - b : 16;
      gi[g] = disc_ginfo(s, nv);
      for (int i = 0; i < nv; ++i) { hx[16 * g + i] = x[b + i]; ht[16 * g + i] = c->dset[s].t[b + i]; }
    }
  }
  // periodic groups behind the stage sets': rows 0..7 the lb points of up to 8 pairs, rows 8..15 their ub partners; the rows
  // of a pair that is not there sit at the first lb point (inside the domain) and are masked by the pair count
  for (int b = 0; b < np; b += 8, ++g) {
    const int nv = np - b < 8 ? np - b : 8;
    gi[g] = disc_ginfo_periodic(nv, c->dper.order);
    for (int i = 0; i < 16; ++i) hx[16 * g + i] = c->dper.lb[0];
    for (int i = 0; i < nv; ++i) { hx[16 * g + i] = c->dper.lb[b + i]; hx[16 * g + 8 + i] = c->dper.ub[b + i]; }
  }
  const size_t rs = real_size(c);
  HIPCHK(c->xs.reserve_bytes(dd.n_pad * rs));
  HIPCHK(c->tgt.reserve_bytes(dd.n_pad * rs));
  HIPCHK(c->d_ginfo.reserve(G));
  if (upload_real(c, c->xs, hx.data(), dd.n_pad) || upload_real(c, c->tgt, ht.data(), dd.n_pad)) return PINN_EHIP;
  HIPCHK(hipMemcpy(c->d_ginfo, gi.data(), G * sizeof(int), hipMemcpyHostToDevice));
  if (disc_upload_tables(c, dd.ldo)) return PINN_EHIP;
  if (disc_alloc_scratch(c, dd, &c->d_Ast, &c->d_A3, c->d_U3, c->d_Nn, c->d_R)) return PINN_EHIP;
  HIPCHK(c->d_dAp.reserve_bytes((size_t)dd.n_chunks * disc_nc(disc_dk(c)) * dd.n_pad * dd.wp * rs));
  HIPCHK(c->d_lossp.reserve_bytes((size_t)G * dd.n_chunks * rs));
  // [group * chunk][2], [...][6] for adr_disc_ide, [...][7] for adrd_disc
  const size_t n_lam = (size_t)G * dd.n_chunks * (has_adr_tail(c) ? tail_len(c->pde) : 2);
  HIPCHK(c->d_lamp.reserve_bytes(n_lam * rs));
  // cleared in stream order: the context's stream is non-blocking, so a hipMemset on the null stream (asynchronous to the
  // host for device memory) is not ordered before the first evaluation's kernels and can wipe rows they have written
  HIPCHK(hipMemsetAsync(c->d_lamp, 0, n_lam * rs, c->stream));
  const size_t need_part = (size_t)G * c->R * rs;
  HIPCHK(c->part.reserve_bytes(need_part));
  HIPCHK(hipMemsetAsync(c->part, 0, need_part, c->stream));
  c->dd = dd;
  c->n_rows = G;
  c->sets_dirty = false;
  return 0;
}

// the operator kind of a discrete-time context (template value DK of kernels_disc.h) and its coefficient block, by value:
// (1, nu) for the Burgers kinds (identification reads its own from the weight vector), the six of c->adr for adr_disc with
// the rows the periodic groups' slope differences travel in (the context's Nn, or none for a prediction), the mask and those
// rows for adr_disc_ide, and with them the nu == 0 flag for adrd_disc
static int disc_dk(const pinn_ctx* c) {
  return is_adrd_disc(c) ? DISC_ADRD : is_adr_disc_ide(c) ? DISC_ADR_IDE : is_adr_disc(c) ? DISC_ADR : DISC_BURGERS;
}
template <typename real, int DK>
static disc_coef_t<real, DK> disc_coef(const pinn_ctx* c, const real* pair_dx) {
  if constexpr (DK == DISC_ADRD)
    return DiscAdrdArg<real>{c->adr_mask, c->nu_off ? 1 : 0, pair_dx};
  else if constexpr (DK == DISC_ADR_IDE)      // the coefficients are the tail of the weight vector; by value, which of them train
    return DiscAdrIdeArg<real>{c->adr_mask, pair_dx};
  else if constexpr (DK == DISC_ADR)
    return DiscAdrArg<real>{(real)c->adr[0], (real)c->adr[1], (real)c->adr[2], (real)c->adr[3], (real)c->adr[4], (real)c->adr[5],
                            pair_dx};
  else
    return DiscC12<real>{real(1), (real)c->nu};
}

template <typename real, int NT, int DK>
static int disc_set_lds() {
  static unsigned long long done = 0;
  if (!first_call_on_device(done)) return 0;
  HIPCHK(hipFuncSetAttribute((const void*)k_disc_fwd<real, NT, DK>, hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)disc_fwd_lds<NT, DK>(sizeof(real))));
  HIPCHK(hipFuncSetAttribute((const void*)k_disc_bwd_out<real, NT, DK>, hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)disc_out_lds<NT, DK>(sizeof(real))));
  HIPCHK(hipFuncSetAttribute((const void*)k_disc_bwd_hidden<real, NT, DK>, hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)disc_hid_lds<NT, DK>(sizeof(real))));
  return 0;
}

template <typename real, int NT, int DK>
static int disc_eval(pinn_ctx* c, hipEvent_t* ev4, const AdamFuse* af) {
  const DiscDesc dd = c->dd;
  const InMap<real> m(c->lb, c->ub);
  const disc_coef_t<real, DK> cf = disc_coef<real, DK>(c, c->d_Nn.as<real>());
  if (int rc = disc_set_lds<real, NT, DK>()) return rc;
  const dim3 grid(dd.n_groups, dd.n_chunks), block(256);
  const real* th = c->theta_r.as<real>();
  if (ev4) HIPCHK(hipEventRecord(ev4[0], c->stream));
  hipLaunchKernelGGL((k_disc_fwd<real, NT, DK>), grid, block, (disc_fwd_lds<NT, DK>(sizeof(real))), c->stream, c->nd, dd, th,
                     c->xs.as<real>(), m.lbx, m.sx, cf, c->d_Ast.as<real>(), c->d_A3.as<real>(), c->d_U3.as<real>(),
                     c->d_Nn.as<real>(), 1);
  hipLaunchKernelGGL((k_disc_irk<real, DK>), grid, block, 0, c->stream, dd, c->nd.n_out, c->d_ginfo,
                     c->d_MT[0].as<real>(), c->d_MT[1].as<real>(), c->d_Nn.as<real>(),
                     c->d_U3.as<real>(), c->tgt.as<real>(), c->d_R.as<real>(), c->d_lossp.as<real>(), 0);
  if (ev4) HIPCHK(hipEventRecord(ev4[1], c->stream));
  hipLaunchKernelGGL((k_disc_bwd_out<real, NT, DK>), grid, block, (disc_out_lds<NT, DK>(sizeof(real))), c->stream, c->nd, dd,
                     th, c->d_ginfo, c->d_M[0].as<real>(), c->d_M[1].as<real>(), c->d_R.as<real>(),
                     c->d_U3.as<real>(), c->d_A3.as<real>(), cf, c->part.as<real>(), c->R, c->d_dAp.as<real>(),
                     c->d_lamp.as<real>());
  hipLaunchKernelGGL((k_disc_bwd_hidden<real, NT, DK>), dim3(dd.n_groups), block, (disc_hid_lds<NT, DK>(sizeof(real))),
                     c->stream, c->nd, dd, th, c->d_ginfo, c->xs.as<real>(), m.lbx, m.sx, c->d_Ast.as<real>(),
                     c->d_dAp.as<real>(), c->d_lossp.as<real>(), c->d_lamp.as<real>(), c->part.as<real>(), c->R);
  if (ev4) HIPCHK(hipEventRecord(ev4[2], c->stream));
  HIPCHK(hipGetLastError());
  return launch_reduce<real>(c, dd.n_groups, af);
}

template <int DK>
static int disc_eval_kind(pinn_ctx* c, hipEvent_t* ev4, const AdamFuse* af) {
  if (c->dtype == PINN_F64) return disc_eval<double, 4, DK>(c, ev4, af);
  if constexpr (DK == DISC_ADRD) return disc_eval<float, 4, DK>(c, ev4, af);     // widths above 64 are refused at create
  else return c->dd.wp == 64 ? disc_eval<float, 4, DK>(c, ev4, af) : disc_eval<float, 8, DK>(c, ev4, af);
}
static int disc_eval_any(pinn_ctx* c, hipEvent_t* ev4, const AdamFuse* af) {
  switch (disc_dk(c)) {
    case DISC_ADRD: return disc_eval_kind<DISC_ADRD>(c, ev4, af);
    case DISC_ADR_IDE: return disc_eval_kind<DISC_ADR_IDE>(c, ev4, af);
    case DISC_ADR: return disc_eval_kind<DISC_ADR>(c, ev4, af);
    default: return disc_eval_kind<DISC_BURGERS>(c, ev4, af);
  }
}

static int eval_loss_grad(pinn_ctx* c, const AdamFuse* af = nullptr) {
  int rc = src_fresh(c, "evaluation");          // (the entry points refuse by their own name before they get here)
  if (rc) return rc;
  rc = is_disc(c) ? disc_ensure(c) : ensure_sets(c);
  if (rc) return rc;
  c->n_evals += 1;
  hipEvent_t* ev4 = nullptr;
  if (c->timing && c->ev_used < c->ev_cap_evals && (c->ev_seen++ % c->ev_every) == 0)
    ev4 = &c->ev[(size_t)4 * c->ev_used];
  if (is_disc(c)) rc = disc_eval_any(c, ev4, af);
  else
    rc = by_kind(c, pde_kind(c, AT_TRAINING), [&](auto r, auto kind) {
      return launch_sweeps<decltype(r), decltype(kind)::value>(c, ev4, af);
    });
  if (rc) return rc;
  if (c->comm && !c->xg.on)
    NCCLCHK(ncclAllReduce(c->gl, c->gl, (size_t)c->R, ncclDouble, ncclSum, c->comm, c->stream));
  if (ev4) { HIPCHK(hipEventRecord(ev4[3], c->stream)); c->ev_used++; }
  return 0;
}

// discrete-time models: network outputs (mode 0) or U + N(U) M^T with the table of `set` (mode 1) at n points
template <typename real, int NT, int DK>
static int disc_predict_impl(pinn_ctx* c, int mode, int set, const double* x, int64_t n, double* out) {
  const int NO = c->nd.n_out;
  const int G = (int)((n + 15) / 16);
  DiscDesc dd{};
  disc_layout(c, dd, G, mode == 1 && c->dset[set].has_M ? c->dset[set].q : 0);
  std::vector<double> hx(dd.n_pad, c->lb[0]);
  for (int64_t i = 0; i < n; ++i) hx[i] = x[i];
  std::vector<int> gi(G, disc_ginfo(set, 16));
  DevBuf<void> xe, U3, Nn, Rb;                   // the call's own: freed on every return
  DevBuf<int> ge;
  const size_t rs = sizeof(real);
  HIPCHK(xe.reserve_bytes(dd.n_pad * rs));
  HIPCHK(ge.reserve(G));
  if (disc_alloc_scratch(c, dd, nullptr, nullptr, U3, Nn, Rb)) return PINN_EHIP;
  if (upload_real(c, xe, hx.data(), dd.n_pad)) return PINN_EHIP;
  if (hipMemcpy(ge, gi.data(), G * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) return PINN_EHIP;
  const InMap<real> m(c->lb, c->ub);
  const size_t lds_f = disc_fwd_lds<NT, DK>(rs);
  if (int rc = disc_set_lds<real, NT, DK>()) return rc;
  const dim3 grid(dd.n_groups, dd.n_chunks), block(256);
  hipLaunchKernelGGL((k_disc_fwd<real, NT, DK>), grid, block, lds_f, c->stream, c->nd, dd, c->theta_r.as<real>(),
                     xe.as<real>(), m.lbx, m.sx, disc_coef<real, DK>(c, nullptr), (real*)nullptr, (real*)nullptr,
                     U3.as<real>(), Nn.as<real>(), 0);
  if (mode == 1)
    hipLaunchKernelGGL((k_disc_irk<real, DK>), grid, block, 0, c->stream, dd, NO, ge.get(), c->d_MT[0].as<real>(),
                       c->d_MT[1].as<real>(), Nn.as<real>(), U3.as<real>(), (const real*)nullptr, Rb.as<real>(),
                       (real*)nullptr, 1);
  std::vector<real> ho((size_t)dd.n_pad * dd.ldo);
  if (hipMemcpyAsync(ho.data(), mode == 1 ? Rb.get() : U3.get(), ho.size() * rs, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
      hipStreamSynchronize(c->stream) != hipSuccess)
    return fail(PINN_EHIP, "discrete-time predict failed: %s", hipGetErrorString(hipGetLastError()));
  for (int64_t i = 0; i < n; ++i)
    for (int j = 0; j < NO; ++j) out[(size_t)i * NO + j] = (double)ho[(size_t)i * dd.ldo + j];
  return 0;
}

template <int DK>
static int disc_predict_kind(pinn_ctx* c, int mode, int set, const double* x, int64_t n, double* out) {
  if (c->dtype == PINN_F64) return disc_predict_impl<double, 4, DK>(c, mode, set, x, n, out);
  if constexpr (DK == DISC_ADRD) return disc_predict_impl<float, 4, DK>(c, mode, set, x, n, out);
  else return c->nd.width <= 64 ? disc_predict_impl<float, 4, DK>(c, mode, set, x, n, out)
                           : disc_predict_impl<float, 8, DK>(c, mode, set, x, n, out);
}
static int disc_predict_any(pinn_ctx* c, int mode, int set, const double* x, int64_t n, double* out) {
  switch (disc_dk(c)) {
    case DISC_ADRD: return disc_predict_kind<DISC_ADRD>(c, mode, set, x, n, out);
    case DISC_ADR_IDE: return disc_predict_kind<DISC_ADR_IDE>(c, mode, set, x, n, out);
    case DISC_ADR: return disc_predict_kind<DISC_ADR>(c, mode, set, x, n, out);
    default: return disc_predict_kind<DISC_BURGERS>(c, mode, set, x, n, out);
  }
}

// ------------------------------------------------------------------------------------------
// mailbox all-reduce: set-up, self-test, tear-down (kernels_xgmi.h)
// ------------------------------------------------------------------------------------------
static void xg_release(pinn_ctx* c) {
  for (int r = 0; r < XG_MAX_RANKS; ++r)
    if (c->xg.opened[r]) { (void)hipIpcCloseMemHandle(c->xg.opened[r]); c->xg.opened[r] = nullptr; }
  if (c->xg.box) { (void)hipFree(c->xg.box); c->xg.box = nullptr; }
  c->xg.err.reset();
  c->xg.attached = c->xg.on = false;
  c->xg.seq = 0;
  c->xg.sharing = 1;
  c->xg.grid_cap = 0;
}

// k_t16_fused's in-kernel boundary hand-over waits (bounded) for the other boundary workgroups of the launch; when one of
// them was not resident in time (a GPU shared with another process, masked CUs) the kernel raises bsync[1] and poisons
// the loss.  Seen at the next host synchronisation: the context switches to the forward pre-pass for good (no
// co-residency assumption) and the call fails with an explicit error instead of handing back a NaN.
static int t16_handover_check(pinn_ctx* c) {
  if (!c->t16_bsync || c->t16_prepass) return 0;
  unsigned int flag = 0;
  HIPCHK(hipMemcpyAsync(&flag, c->t16_bsync + 1, sizeof(flag), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (!flag) return 0;
  HIPCHK(hipMemsetAsync(c->t16_bsync + 1, 0, sizeof(flag), c->stream));
  c->t16_prepass = true;
  return fail(PINN_ESTATE, "k_t16_fused: the periodic-boundary workgroups of one launch were not resident together within "
                           "the time limit (is the GPU shared or are CUs masked?); the losses since the last "
                           "synchronisation are not valid.  This context now runs the boundary forward pre-pass instead: "
                           "restore the weights (pinn_set_weights) and repeat the call");
}

// One rank of a data-parallel job: a hand-over time-out would be seen by THIS rank only -- it would fail with PINN_ESTATE and move
// to the pre-pass while its peers, whose all-reduced loss is poisoned all the same, keep stepping -- and "restore the weights and
// repeat" cannot be done rank-locally.  So with peers attached the boundary outputs come from the pre-pass from the start (no
// co-residency assumption at all; one small forward launch per evaluation), unless PINN_T16_PREPASS says otherwise.
static void t16_prepass_for_ranks(pinn_ctx* c, int n_ranks) {
  if (n_ranks > 1 && !c->t16_prepass_pinned) c->t16_prepass = true;
}

// an error raised inside a mailbox kernel (a peer that never delivered) surfaces at the next host sync
static int xg_check(pinn_ctx* c) {
  if (int rc = t16_handover_check(c)) return rc;
  if (!c->xg.on) return 0;
  int e = 0;
  HIPCHK(hipMemcpyAsync(&e, c->xg.err, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (e) {
    c->xg.poisoned = true;
    return fail(PINN_ECOMM, "mailbox all-reduce: a peer did not deliver its vector within the time limit; the weights "
                            "are undefined until pinn_set_weights");
  }
  return 0;
}

// T rounds on integer-valued vectors (exact in float64, so the expected sum is known in closed form)
static int xg_self_test(pinn_ctx* c, int* ok) {
  *ok = 0;
  const int R = c->R, n = c->xg.peers.n_ranks, me = c->xg.peers.rank;
  DevBuf<double> vec, out;
  HIPCHK(vec.reserve(R));
  HIPCHK(out.reserve(R));
  std::vector<double> h(R), got(R);
  bool good = true;
  for (int round = 0; round < 6 && good; ++round) {
    for (int i = 0; i < R; ++i) h[i] = (double)((me + 1) * 1000 + (i % 97) + round);
    HIPCHK(hipMemcpyAsync(vec, h.data(), (size_t)R * 8, hipMemcpyHostToDevice, c->stream));
    if (++c->xg.seq == 0) c->xg.seq = 2;
    const unsigned int seq = c->xg.seq;
    hipLaunchKernelGGL((k_reduce_xgmi<double, false>), xg_grid(c, R), dim3(RED_THREADS), 0,
                       c->stream, (const double*)vec, 1, R, out.get(), c->xg.peers, seq, XG_TEST_TIMEOUT_TICKS, c->xg.err.get(), 0,
                       (double*)nullptr, (double*)nullptr, (double*)nullptr, (double*)nullptr, 0.0, 0.0, 0.0, 0.0,
                       (double*)nullptr, c->nd, (float*)nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(got.data(), out, (size_t)R * 8, hipMemcpyDeviceToHost, c->stream));
    int e = 0;
    HIPCHK(hipMemcpyAsync(&e, c->xg.err, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (e) good = false;
    for (int i = 0; i < R && good; ++i) {
      const double want = 1000.0 * n * (n + 1) / 2.0 + (double)n * ((i % 97) + round);
      if (got[i] != want) good = false;
    }
  }
  if (!good) HIPCHK(hipMemsetAsync(c->xg.err, 0, sizeof(int), c->stream));
  *ok = good ? 1 : 0;
  return 0;
}

static int cast_weights(pinn_ctx* c) {
  const int n = c->nd.n_theta;
  by_real(c, [&](auto r) {
    using real = decltype(r);
    hipLaunchKernelGGL((k_cast_weights<real>), dim3((n + 255) / 256), dim3(256), 0, c->stream, n, c->theta,
                       c->theta_r.as<real>(), c->nd, c->img);
  });
  HIPCHK(hipGetLastError());
  return 0;
}

// n caller-supplied points -> c->xe / c->te (compute dtype, padded to 64 with inert points).  The last point set stays
// on the device and on the host: a repeat with identical contents (the scripts evaluate the same X_star grid at every
// logged error and again at the end, utils/logger.py:56-60, inf_cont_burgers.py:114-123) uploads nothing.
static int eval_points(pinn_ctx* c, const double* X, int64_t n, int* n_pad_out) {
  const size_t rs = real_size(c);
  const int NO = c->nd.n_out;
  const int n_pad = (int)((n + 63) / 64 * 64);
  *n_pad_out = n_pad;
  if ((size_t)n * 2 == c->ev_X.size() && c->ev_n_pad == n_pad && memcmp(c->ev_X.data(), X, (size_t)n * 16) == 0) return 0;
  HIPCHK(c->xe.reserve_bytes(n_pad * rs));
  HIPCHK(c->te.reserve_bytes(n_pad * rs));
  HIPCHK(c->Oe.reserve_bytes((size_t)NO * n_pad * 4 * rs));
  c->ev_X.clear();
  std::vector<double> hx(n_pad, c->lb[0]), ht(n_pad, c->lb[1]);
  for (int64_t i = 0; i < n; ++i) { hx[i] = X[2 * i]; ht[i] = X[2 * i + 1]; }
  if (upload_real(c, c->xe, hx.data(), n_pad) || upload_real(c, c->te, ht.data(), n_pad)) return PINN_EHIP;
  c->ev_X.assign(X, X + 2 * n);
  c->ev_n_pad = n_pad;
  return 0;
}

// width-20 nets: the MFMA forward sweeps of kernels_predict20.h.  NCH = 4 -> O4 ([n_pad] vec4 (u, u_x, u_t, u_xx)),
// NCH = 1 -> out1 ([n_pad] float64 u)
template <int NCH>
static int predict20_launch(pinn_ctx* c, const void* xs, const void* ts, int n_pad, void* O4, double* out1) {
  const int n_tiles = n_pad / 64;
  if (c->dtype == PINN_F64) {
    const InMap<double> m(c->lb, c->ub);
    const size_t lds = predict20_lds_bytes(c->nd, 8);
    const int wg = n_tiles < 4 * c->n_cu ? n_tiles : 4 * c->n_cu;
    hipLaunchKernelGGL((k_fwd20d<NCH>), dim3(wg), dim3(256), lds, c->stream, c->nd, c->theta_r.as<double>(),
                       (const double*)xs, (const double*)ts, n_tiles, m.lbx, m.lbt, m.sx, m.st,
                       (vec4<double>*)O4, out1);
  } else {
    const InMap<float> m(c->lb, c->ub);                 // sx, st: (float) of the float64 quotient
    const size_t lds = predict20_lds_bytes(c->nd, 4);
    const int wg = n_tiles < 8 * c->n_cu ? n_tiles : 8 * c->n_cu;
    hipLaunchKernelGGL((k_fwd20f<NCH>), dim3(wg), dim3(64), lds, c->stream, c->nd, c->theta_r.as<float>(),
                       (const float*)xs, (const float*)ts, n_tiles, m.lbx, m.lbt, m.sx, m.st,
                       (vec4<float>*)O4, out1);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

// Taylor-channel forward sweep of the points in xs/ts -> O ([n_out][n_pad] vec4 (u, u_x, u_t, u_xx))
static int forward_taylor(pinn_ctx* c, const void* xs, const void* ts, int n_pad, int chunk, void* O) {
  if (predict20_ok(c->nd) && !is_disc(c) && !is_adr2(c)) return predict20_launch<4>(c, xs, ts, n_pad, O, nullptr);
  const size_t need_S = (size_t)c->nd.n_hidden * c->nd.width * (size_t)chunk * 4 * real_size(c);
  HIPCHK(c->S.reserve_bytes(need_S));
  for (int base = 0; base < n_pad; base += chunk) {
    const int pts = (n_pad - base < chunk) ? n_pad - base : chunk;
    const int rc = by_real(c, [&](auto r) { return forward_chunk<decltype(r)>(c, xs, ts, n_pad, chunk, O, base, pts); });
    if (rc) return rc;
  }
  HIPCHK(hipGetLastError());
  return 0;
}

// network outputs at the current evaluation points -> c->pred ([n][n_out] float64, device)
static int predict_values(pinn_ctx* c, int64_t n, int n_pad) {
  const int NO = c->nd.n_out;
  HIPCHK(c->pred.reserve((size_t)n_pad * NO));
  if (predict20_ok(c->nd) && !is_disc(c)) return predict20_launch<1>(c, c->xe, c->te, n_pad, nullptr, c->pred);
  const int chunk = n_pad < CHUNK_POINTS ? n_pad : CHUNK_POINTS;
  if (int rc = forward_taylor(c, c->xe, c->te, n_pad, chunk, c->Oe)) return rc;
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  by_real(c, [&](auto r) {
    using real = decltype(r);
    hipLaunchKernelGGL((k_pick_values<real>), grid, block, 0, c->stream, c->Oe.as<vec4<real>>(), (int)n, n_pad, NO,
                       c->pred);
  });
  HIPCHK(hipGetLastError());
  return 0;
}

// PDE residuals from Taylor outputs: points first .. first + count - 1 of O ([n_out][n_pad] vec4, forward_taylor) -> dst
// ([count][n_out] float64, device), in the kind the place calls for (adr_kind).  Enqueues only.
static int launch_residual(pinn_ctx* c, Where w, const void* O, int first, int count, int n_pad, double* dst) {
  const dim3 grid((unsigned)((count + 255) / 256)), block(256);
  const int rc = by_kind(c, pde_kind(c, w), [&](auto r, auto kind) {
    using real = decltype(r);
    constexpr int PDE = decltype(kind)::value;
    if constexpr (PDE == PDE_ADR_ROBIN) {           // no such k_residual, and adr_kind answers it for training alone
      return fail(PINN_EINVAL, "a residual has no Robin form");
    } else {
      pde_coef_t<real, PDE> coef = pde_coef<real, PDE>(c);
      if constexpr (PDE == PDE_ADR_SRC || PDE == PDE_ADR2) {   // s is not known at foreign points: the null form, N[u] alone
        if (w == AT_FOREIGN) coef.src = nullptr;
      }
      hipLaunchKernelGGL((k_residual<real, PDE>), grid, block, 0, c->stream, first, count, n_pad, (const vec4<real>*)O,
                         c->theta_r.as<real>(), c->nd.n_net, coef, dst, c->nd.n_out);
      return 0;
    }
  });
  if (rc) return rc;
  HIPCHK(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------------------------
// residual-based adaptive collocation (kernels_rad.h)
// ------------------------------------------------------------------------------------------
// the buffers of pinn_rad_collocation: grown only (a grow synchronises; a repeat at the same sizes only enqueues)
static int rad_alloc(pinn_ctx* c, int64_t count, int64_t M) {
  if (count > 0) {                               // (an empty draw allocates nothing)
    HIPCHK(c->rad.cx.reserve((size_t)count));
    HIPCHK(c->rad.ct.reserve((size_t)count));
  }
  HIPCHK(c->rad.tot.reserve(1));
  const size_t n_pad = (size_t)((M + 63) / 64 * 64), rs = real_size(c), NO = (size_t)c->nd.n_out;
  const size_t nb = (n_pad + RAD_BLOCK - 1) / RAD_BLOCK;
  const bool grown = n_pad * rs > c->rad.px.capacity_bytes() || n_pad * rs > c->rad.pt.capacity_bytes();
  HIPCHK(c->rad.px.reserve_bytes(n_pad * rs));
  HIPCHK(c->rad.pt.reserve_bytes(n_pad * rs));
  HIPCHK(c->rad.O.reserve_bytes(NO * n_pad * 4 * rs));
  HIPCHK(c->rad.f.reserve(NO * n_pad));
  HIPCHK(c->rad.w.reserve(n_pad));
  HIPCHK(c->rad.bsum.reserve(nb));
  if (grown) {                                   // pad points of a new pool: finite, inert, never drawn
    HIPCHK(hipMemsetAsync(c->rad.px, 0, n_pad * rs, c->stream));
    HIPCHK(hipMemsetAsync(c->rad.pt, 0, n_pad * rs, c->stream));
  }
  return 0;
}

// pool -> residuals -> integer weights -> CDF -> the col.count samples from col.first, into the collocation slots and the
// float64 copy.  Enqueues only.
static int rad_draw(pinn_ctx* c, int64_t M, uint64_t seed, int k, double c_add) {
  const int64_t cnt = c->col.count;
  if (cnt <= 0) return 0;
  const int NO = c->nd.n_out;
  const InMap<double> m(c->lb, c->ub);
  const int n_pad = (int)((M + 63) / 64 * 64);
  const uint32_t lo = (uint32_t)seed, hi = (uint32_t)(seed >> 32);
  const uint64_t n = (uint64_t)M;
  const dim3 grid_m((unsigned)((M + RAD_BLOCK - 1) / RAD_BLOCK)), block(RAD_BLOCK);
  // 1. the pool: points [0, M) of the M-point design, in the compute dtype (k_lhs_fill, as pinn_lhs_collocation draws it)
  by_real(c, [&](auto r) {
    using real = decltype(r);
    hipLaunchKernelGGL((k_lhs_fill<real>), grid_m, block, 0, c->stream, c->rad.px.as<real>(), c->rad.pt.as<real>(), M,
                       (uint64_t)0, n, lhs_half_bits(n), lo, hi, m.lbx, m.lbt, m.ex, m.et);
  });
  HIPCHK(hipGetLastError());
  // 2. residuals at the current weights: pinn_residual_at's forward sweep and k_residual
  const int chunk = n_pad < CHUNK_POINTS ? n_pad : CHUNK_POINTS;
  if (int rc = forward_taylor(c, c->rad.px, c->rad.pt, n_pad, chunk, c->rad.O)) return rc;
  if (int rc = launch_residual(c, AT_FOREIGN, c->rad.O, 0, (int)M, n_pad, c->rad.f)) return rc;
  // 3.-4. weights and their CDF
  HIPCHK(hipMemsetAsync(c->rad.tot, 0, sizeof(RadTotals), c->stream));
  hipLaunchKernelGGL(k_rad_mag, grid_m, block, 0, c->stream, (const double*)c->rad.f, NO, M, k, c->rad.w, c->rad.tot);
  hipLaunchKernelGGL(k_rad_q, grid_m, block, 0, c->stream, c->rad.w, M, (const RadTotals*)c->rad.tot, c->rad.bsum);
  hipLaunchKernelGGL(k_rad_scan, dim3(1), dim3(RAD_SCAN), 0, c->stream, c->rad.bsum, (int)grid_m.x, M, c_add, c->rad.tot);
  HIPCHK(hipGetLastError());
  // 5. the draw
  const size_t off = (size_t)colloc_first(c->sd);
  const dim3 grid_s((unsigned)((cnt + 255) / 256)), block_s(256);
  by_real(c, [&](auto r) {
    using real = decltype(r);
    hipLaunchKernelGGL((k_rad_select<real>), grid_s, block_s, 0, c->stream, c->rad.px.as<real>(),
                       c->rad.pt.as<real>(), (const unsigned long long*)c->rad.w,
                       (const unsigned long long*)c->rad.bsum, (const RadTotals*)c->rad.tot, M, (uint64_t)c->col.first,
                       cnt, lo, hi, c->xs.as<real>() + off, c->ts.as<real>() + off, c->rad.cx, c->rad.ct);
  });
  HIPCHK(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------------------------
// The optional extras of a context, one row each: how to see that one is present, the phrases its refusals are built from
// (whole phrases: "are" / "is" and "them" / "it" are the row's, no grammar is derived) and how the caller removes it.  The two
// weight kinds belong to one kind of problem in float64 on kernel path 7 (weights_supported); the three extras of the adr
// kind run on both of its paths, in both dtypes (adr_extra_gate).  Every extra is single-device.
// ------------------------------------------------------------------------------------------
enum { X_SA, X_PW, X_ROBIN, X_SRC, X_KF, X_COUNT };
struct Extra {
  bool (*present)(const pinn_ctx*);
  const char* is;        // subject and verb
  const char* runs;
  const char* remove;    // the call that removes it
  int home_pde;          // the one kind of problem it is for, and its name
  const char* home;
  const char* needs;     // the weight kinds only
  const char* pron;      // the adr extras only: the object form, and point weights' refusal to stand beside it
  const char* pw_clash;
};
static const Extra EXTRAS[X_COUNT] = {
    {[](const pinn_ctx* c) { return c->sa.on; }, "self-adaptive weights are", "self-adaptive weights run",
     "pinn_sa_disable", PINN_PDE_BURGERS, "Burgers inference (pde 0)", "self-adaptive weights need", nullptr, nullptr},
    {[](const pinn_ctx* c) { return c->pw.on; }, "point weights are", "point weights run", "pinn_pw_disable", PINN_PDE_ADR,
     "the adr kind (pde 5)", "point weights need", nullptr, nullptr},
    {[](const pinn_ctx* c) { return !c->robin.X.empty(); }, "Robin points are", "Robin points run",
     "pinn_set_robin with n = 0", PINN_PDE_ADR, "the adr kind (pde 5)", nullptr, "them",
     "point weights do not cover Robin points"},
    {[](const pinn_ctx* c) { return c->src.on; }, "a source term is", "a source term runs", "pinn_set_source with n = 0",
     PINN_PDE_ADR, "the adr kind (pde 5)", nullptr, "it", "point weights are not combined with a source term"},
    {[](const pinn_ctx* c) { return c->kf.on; }, "coefficient fields are", "coefficient fields run",
     "pinn_set_coef_fields with n = 0", PINN_PDE_ADR, "the adr kind (pde 5)", nullptr, "them",
     "point weights are not combined with coefficient fields"},
};

// a communicator is refused while any extra is present, and for the adr_ide kind.  That kind comes last: it can hold none of
// the five (adr_extra_gate and weights_supported refuse them), so its place among them cannot be observed
static int single_device_only(const pinn_ctx* c, const char* who) {
  for (const Extra& x : EXTRAS)
    if (x.present(c)) return fail(PINN_EUNSUPPORTED, "%s: %s single-device (%s first)", who, x.is, x.remove);
  if (is_adr_ide(c))
    return fail(PINN_EUNSUPPORTED, "%s: the adr_ide kind (pde 6) is single-device; it has no data-parallel launch", who);
  if (is_adr2(c))
    return fail(PINN_EUNSUPPORTED, "%s: the adr2 kind (pde 10) is single-device; it has no data-parallel launch", who);
  return 0;
}

// what a weighted kernel serves: its kind of problem in float64 on kernel path 7, one device; checked before any device work
static int weights_supported(const pinn_ctx* c, const Extra& x, const char* who) {
  if (c->pde != x.home_pde) return fail(PINN_EUNSUPPORTED, "%s: %s for %s only", who, x.is, x.home);
  if (c->dtype != PINN_F64) return fail(PINN_EUNSUPPORTED, "%s: %s float64", who, x.needs);
  if (c->path != KP_FUSED20D)
    return fail(PINN_EUNSUPPORTED, "%s: %s kernel path 7 (this context runs path %d)", who, x.needs, (int)c->path);
  if (c->comm || c->xg.box)
    return fail(PINN_EUNSUPPORTED, "%s: %s single-device; this context has a communicator", who, x.is);
  return 0;
}

// what the setter of an adr extra asks of the context, behind its own checks of the arrays (they need no context) and in
// front of everything else: the adr kind, no point weights, one of its two paths, one device
static int adr_extra_gate(const pinn_ctx* c, const Extra& x, const char* who) {
  REQUIRE(c, "%s: null context", who);
  if (c->pde == PINN_PDE_ADR_IDE)
    return fail(PINN_EUNSUPPORTED, "%s: %s for %s only; the adr_ide kind (pde 6) has no variant for %s", who, x.is, x.home,
                x.pron);
  // the adr2 kind (pde 10) takes wall points and a source as the adr kind does, and neither fields nor point weights
  const bool adr2_has = is_adr2(c) && (&x == &EXTRAS[X_ROBIN] || &x == &EXTRAS[X_SRC]);
  if (c->pde != x.home_pde && !adr2_has) return fail(PINN_EUNSUPPORTED, "%s: %s for %s only", who, x.is, x.home);
  if (EXTRAS[X_PW].present(c))
    return fail(PINN_EUNSUPPORTED, "%s: %s (%s first)", who, x.pw_clash, EXTRAS[X_PW].remove);
  if (!adr_has_path(c->path))
    return fail(PINN_EUNSUPPORTED, "%s: %s on kernel paths 0 and 7 only (this context runs path %d)", who, x.runs,
                (int)c->path);
  if (c->comm || c->xg.box)
    return fail(PINN_EUNSUPPORTED, "%s: %s single-device; this context has a communicator", who, x.is);
  return 0;
}

// the collocation points were replaced: a source's values and the fields' rows belonged to the old points (nothing evaluates
// until their setters are called again, src_fresh), and both weight stores start that class over
static void colloc_replaced(pinn_ctx* c) {
  if (c->src.on) c->src.stale = true;
  if (c->kf.on) c->kf.stale = true;
  c->sa.arr.reset[LAM_COL] = c->pw.arr.reset[LAM_COL] = true;
}

// what the three calls that take points first .. first + count - 1 of an n_design-point design ask of those numbers
static int design_check(int64_t n_design, int64_t first, int64_t count) {
  REQUIRE(n_design >= 1 && first >= 0 && count >= 0 && first + count <= n_design && count <= (1 << 30),
          "bad design geometry (n_design %lld, first %lld, count %lld)", (long long)n_design, (long long)first,
          (long long)count);
  return 0;
}

// the collocation block now comes from a design on the device: no host points, the design's size as the global total
static void colloc_from_design(pinn_ctx* c, pinn_ctx::ColFrom from, int64_t n_design, int64_t first, int64_t count) {
  c->col = pinn_ctx::ColOrigin{from, n_design, first, count};
  c->sets.Xf.clear();
  c->nf_total = n_design;
  c->sd.inv_nf = 1.0 / (double)n_design;
  colloc_replaced(c);
}

// ------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------
extern "C" {

const char* pinn_last_error(void) { return g_err.c_str(); }
int pinn_abi_version(void) { return 6; }

int pinn_device_count(int* n) {
  REQUIRE(n, "null");
  HIPCHK(hipGetDeviceCount(n));
  return 0;
}

// which HIP runtime / driver / RCCL build this process actually bound (a process that imported torch first resolves the
// sonames to torch's bundled ROCm; a plain process to /opt/rocm): recorded in every bench line
int pinn_runtime_versions(int* hip_runtime, int* hip_driver, int* rccl) {
  if (hip_runtime) HIPCHK(hipRuntimeGetVersion(hip_runtime));
  if (hip_driver) HIPCHK(hipDriverGetVersion(hip_driver));
  if (rccl) {
    const ncclResult_t r = ncclGetVersion(rccl);
    if (r != ncclSuccess) return fail(PINN_ECOMM, "ncclGetVersion: %s", ncclGetErrorString(r));
  }
  return 0;
}

int pinn_device_info(int device, char* name, int cap, int* n_cu, int64_t* hbm_bytes) {
  hipDeviceProp_t p;
  HIPCHK(hipGetDeviceProperties(&p, device));
  if (name && cap > 0) snprintf(name, cap, "%s (%s)", p.name, p.gcnArchName);
  if (n_cu) *n_cu = p.multiProcessorCount;
  if (hbm_bytes) *hbm_bytes = (int64_t)p.totalGlobalMem;
  return 0;
}

// PINN_PDE_ADR_IDE, PINN_PDE_ADR_DISC_IDE: raw [a0, a1, nu, r1, r2, r3] -> the tail of theta (log nu in the nu slot) and its compute-dtype mirror.
// PINN_PDE_ADRD_DISC: seven, d3 raw behind them; nu == 0 raises c->nu_off and leaves 0.0 in the nu slot, nu > 0 lowers it
static int adr_ide_write_tail(pinn_ctx* c, const double* p) {
  const int nt = tail_len(c->pde);
  double tail[7];
  for (int i = 0; i < nt; ++i) tail[i] = i == 2 ? std::log(p[i]) : p[i];
  if (is_adrd_disc(c)) {
    c->nu_off = p[2] == 0.0;
    if (c->nu_off) tail[2] = 0.0;
  }
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpyAsync(c->theta + c->nd.n_net, tail, (size_t)nt * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));       // tail lives on this stack
  if (int rc = cast_weights(c)) return rc;
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

// pinn_create behind its checks: the stream, the environment's knobs, the buffers every context has and the kernel path.
// pinn_create destroys the context on any failure, so every return here is plain
static int ctx_device_init(pinn_ctx* c) {
  NetDesc& nd = c->nd;
  hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
  if (e != hipSuccess) { c->stream = nullptr; return fail(PINN_EHIP, "hipStreamCreate: %s", hipGetErrorString(e)); }
  // debug knobs of k_t16_fused's boundary hand-over (tests/test_gpu_parity.py): force the pre-pass / shorten the wait
  // (a value that does not parse is an error, not a silent 0: zero ticks would make every hand-over expire at once)
  // the split one-tile launch of path 7 (split_plan): auto (default), 0 = never, 1 = required where the kernel exists
  if (const char* v = getenv("PINN_F64_SPLIT")) {
    if (!strcmp(v, "0")) c->f64_split = 0;
    else if (!strcmp(v, "1")) c->f64_split = 1;
    else if (strcmp(v, "auto")) return fail(PINN_EINVAL, "PINN_F64_SPLIT must be auto, 0 or 1 (got \"%s\")", v);
  }
  if (const char* v = getenv("PINN_T16_PREPASS")) {
    if (!(v[0] == '0' || v[0] == '1') || v[1]) return fail(PINN_EINVAL, "PINN_T16_PREPASS must be 0 or 1 (got \"%s\")", v);
    c->t16_prepass = v[0] == '1';
    c->t16_prepass_pinned = true;
  }
  if (const char* v = getenv("PINN_T16_HANDOVER_TICKS")) {
    char* end = nullptr;
    const long long t = strtoll(v, &end, 10);
    if (end == v || *end || t <= 0) return fail(PINN_EINVAL, "PINN_T16_HANDOVER_TICKS must be a positive integer of 100 MHz ticks (got \"%s\")", v);
    c->t16_handover_ticks = t;
  }
  if (const char* v = getenv("PINN_T16_COSTS")) {
    double a = 0, b = 0;
    char tail = 0;
    if (sscanf(v, "%lf,%lf%c", &a, &b, &tail) != 2 || !(a > 0 && b > 0)) return fail(PINN_EINVAL, "PINN_T16_COSTS must be two positive numbers \"full,strip\" (got \"%s\")", v);
    c->t16_cost_full = a; c->t16_cost_strip = b;
  }
  const size_t n = nd.n_theta;
  HIPCHK(c->theta.reserve(n));
  HIPCHK(c->gl.reserve((size_t)c->R));
  HIPCHK(c->adam_m.reserve(n));
  HIPCHK(c->adam_v.reserve(n));
  HIPCHK(c->theta_r.reserve_bytes(n * real_size(c) + 1024));   // + one LDS-DMA piece of slack
  HIPCHK(hipMemsetAsync(c->theta, 0, n * 8, c->stream));
  HIPCHK(hipMemsetAsync(c->theta_r, 0, n * real_size(c), c->stream));
  HIPCHK(hipMemsetAsync(c->gl, 0, (size_t)c->R * 8, c->stream));
  HIPCHK(c->d_nonfinite.reserve(1));
  HIPCHK(hipMemsetAsync(c->d_nonfinite, 0, 8, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, c->device) == hipSuccess && prop.multiProcessorCount > 0)
      c->n_cu = prop.multiProcessorCount;
  }
  if (fused_regs_ok(c)) {
    const size_t nimg = fused20m_image_floats(nd.n_hidden);
    HIPCHK(c->img.reserve(nimg));
    HIPCHK(hipMemsetAsync(c->img, 0, nimg * 4, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  if (fused_regs_ok(c)) nd.img_kind = 1;
  if (fused_f64_ok(c)) {
    std::vector<int> ri((size_t)fused20d_blocks(nd.n_hidden) * 16);
    fused20d_row_index(nd, nd.n_hidden, ri.data());
    HIPCHK(c->row_index.reserve(ri.size()));
    HIPCHK(hipMemcpy(c->row_index, ri.data(), ri.size() * sizeof(int), hipMemcpyHostToDevice));
  }
  if (wide_ok(c)) {
    const size_t nimg = wide_image_floats<100>(nd.n_hidden);
    HIPCHK(c->img.reserve(nimg));
    HIPCHK(hipMemsetAsync(c->img, 0, nimg * 4, c->stream));   // the zero padding is never rewritten
    HIPCHK(hipStreamSynchronize(c->stream));
    nd.img_kind = 2;
  }
  for (KernelPath p : PATH_PREFERENCE)      // (KP_GENERIC, the last, takes every net)
    if (path_ok(c, p)) { c->path = p; break; }
  if (has_adr_tail(c)) return adr_ide_write_tail(c, c->adr);    // starts as Burgers too, every coefficient frozen
  return 0;
}

int pinn_create(pinn_ctx** out, const int* layers, int n_layers, const double* lb,
                const double* ub, int pde_kind, int dtype, int device) {
  REQUIRE(out && layers && lb && ub, "null argument");
  REQUIRE(n_layers >= 3 && n_layers <= MAX_DENSE + 1, "need 3..%d layer sizes, got %d", MAX_DENSE + 1, n_layers);
  REQUIRE(dtype == PINN_F32 || dtype == PINN_F64, "dtype must be PINN_F32 or PINN_F64");
  REQUIRE(pde_kind >= 0 && pde_kind <= PINN_PDE_ADR2, "unknown pde kind %d", pde_kind);
  const bool disc = disc_kind(pde_kind);
  if (disc) REQUIRE(layers[0] == 1, "discrete-time models take one input (x), got %d", layers[0]);
  else REQUIRE(layers[0] == 2, "input dimension must be 2 (x, t), got %d", layers[0]);
  const int W = layers[1], NO = layers[n_layers - 1];
  for (int i = 1; i < n_layers - 1; ++i)
    REQUIRE(layers[i] == W, "all hidden widths must be equal (the reference's sizes_w assumes it, "
                            "utils/neuralnetwork.py:40-45); got %d vs %d", layers[i], W);
  REQUIRE(W >= 1 && W <= MAX_WIDTH, "hidden width %d outside 1..%d", W, MAX_WIDTH);
  if (disc) {
    REQUIRE(NO >= 1 && NO <= 65536, "output size %d outside 1..65536", NO);
    // four Taylor channels: k_disc_bwd_hidden at NT = 8 would need 169 024 B of LDS, a CU has 163 840 B
    if (pde_kind == PINN_PDE_ADRD_DISC && W > 64)
      return fail(PINN_EUNSUPPORTED, "the adrd_disc kind: hidden width %d exceeds 64, what the four-channel kernels hold in LDS "
                  "(float32 too)", W);
    REQUIRE(W <= (dtype == PINN_F64 ? 64 : 128), "discrete-time models: hidden width %d exceeds what the LDS-resident "
            "kernels hold (64 in float64, 128 in float32)", W);
  }
  else REQUIRE(NO == (pde_kind == PINN_PDE_SCHRODINGER ? 2 : 1), "output size %d does not match the PDE kind", NO);
  REQUIRE(ub[0] > lb[0] && (disc || ub[1] > lb[1]), "ub must exceed lb");
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  REQUIRE(device >= 0 && device < ndev, "device %d not present (%d devices)", device, ndev);
  HIPCHK(hipSetDevice(device));

  pinn_ctx* c = new pinn_ctx();
  c->device = device; c->dtype = dtype; c->pde = pde_kind; c->n_layers = n_layers;
  for (int i = 0; i < n_layers; ++i) c->layers[i] = layers[i];
  c->lb[0] = lb[0]; c->ub[0] = ub[0];
  if (disc) { c->lb[1] = 0.0; c->ub[1] = 1.0; } else { c->lb[1] = lb[1]; c->ub[1] = ub[1]; }
  c->nu = 0.01 / M_PI;
  c->adr[1] = 1.0; c->adr[2] = c->nu;              // PINN_PDE_ADR and PINN_PDE_ADR_DISC start as Burgers: [0, 1, nu, 0, 0, 0]
  if (pde_kind == PINN_PDE_ADR2) c->adr[6] = 1.0;  // ... and PINN_PDE_ADR2 with b = 1, kappa = 0
  NetDesc& nd = c->nd;
  nd.n_hidden = n_layers - 2; nd.width = W; nd.n_out = NO;
  int off = 0;
  for (int d = 0; d < n_layers - 1; ++d) {
    nd.off_w[d] = off; off += layers[d] * layers[d + 1];
    nd.off_b[d] = off; off += layers[d + 1];
  }
  nd.n_net = off;
  nd.n_theta = off + tail_len(pde_kind);
  c->R = nd.n_theta + LOSS_SLOTS;
  if (int rc = ctx_device_init(c)) { (void)pinn_destroy(c); return rc; }
  *out = c;
  return 0;
}

// The buffers go with `delete c` (devbuf.h): the device is current and the stream idle by then
int pinn_destroy(pinn_ctx* c) {
  if (!c) return 0;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  if (c->comm) ncclCommDestroy(c->comm);
  xg_release(c);
  for (auto& p : c->tk.pend) if (p.ev) (void)hipEventDestroy(p.ev);
  for (hipEvent_t e : c->ev) (void)hipEventDestroy(e);
  if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
  return 0;
}

int pinn_num_params(pinn_ctx* c, int64_t* n) {
  REQUIRE(c && n, "null");
  *n = c->nd.n_theta;
  return 0;
}

int pinn_set_collocation(pinn_ctx* c, const double* X_f, int64_t n, int64_t n_total) {
  if (c && is_disc(c)) return fail(PINN_EINVAL, "pinn_set_collocation: discrete-time models take stage sets (pinn_disc_set_stage)");
  REQUIRE(c && (X_f || n == 0) && n >= 0 && n_total >= n, "bad collocation arguments");
  c->sets.Xf.assign(X_f, X_f + 2 * n);
  c->nf_total = n_total;
  c->col = pinn_ctx::ColOrigin{};
  colloc_replaced(c);
  c->sets_dirty = true;
  return 0;
}

int pinn_lhs_collocation(pinn_ctx* c, int64_t n_design, int64_t first, int64_t count, uint64_t seed) {
  REQUIRE(c, "null");
  REQUIRE(!is_disc(c) && c->pde != PINN_PDE_BURGERS_IDE, "pinn_lhs_collocation: this model has no collocation set");
  if (int rc = design_check(n_design, first, count)) return rc;
  HIPCHK(hipSetDevice(c->device));
  const bool same_shape = c->col.from == pinn_ctx::COL_LHS && !c->sets_dirty && c->col.count == count;
  colloc_from_design(c, pinn_ctx::COL_LHS, n_design, first, count);   // (the fill writes xs and ts only)
  c->lhs.seed = seed;
  if (same_shape) return lhs_fill(c);            // re-draw in place: one launch, nothing reallocated
  c->sets_dirty = true;
  return 0;
}

int pinn_rad_collocation(pinn_ctx* c, int64_t n_design, int64_t first, int64_t count, int64_t n_pool, uint64_t seed,
                         int k, double c_add) {
  REQUIRE(c, "null");
  if (is_disc(c) || c->pde == PINN_PDE_BURGERS_IDE)
    return fail(PINN_EUNSUPPORTED, "pinn_rad_collocation: this model has no collocation set");
  if (is_adr2(c))
    return fail(PINN_EUNSUPPORTED, "pinn_rad_collocation: the adr2 kind (pde 10) has no adaptive draw");
  if (int rc = design_check(n_design, first, count)) return rc;
  REQUIRE(n_pool >= 1 && n_pool <= RAD_POOL_MAX, "pinn_rad_collocation: n_pool %lld is outside 1..2^24", (long long)n_pool);
  if (c->src.on)                                  // refused first: the source is not made stale, the context stays usable
    return fail(PINN_EUNSUPPORTED, "pinn_rad_collocation: the adaptive draw is not combined with a source term -- the pool's "
                "residuals would lack s (pinn_set_source with n = 0 first)");
  if (c->kf.on)                                   // the same: the pool's points have no rows
    return fail(PINN_EUNSUPPORTED, "pinn_rad_collocation: the adaptive draw is not combined with coefficient fields -- the "
                "coefficients are not known at the pool's points (pinn_set_coef_fields with n = 0 first)");
  REQUIRE(k >= 1 && k <= 4, "pinn_rad_collocation: k %d is outside 1..4", k);
  REQUIRE(std::isfinite(c_add) && c_add >= 0.0 && c_add <= 64.0, "pinn_rad_collocation: c %g is outside [0, 64]", c_add);
  HIPCHK(hipSetDevice(c->device));
  // the slots stay where they are (same count, set assembled): the draw only enqueues, as an in-place LHS redraw does
  const bool in_place = !c->sets_dirty && c->sd.n_f == count;
  if (int rc = rad_alloc(c, count, n_pool)) return rc;          // may fail before anything changes
  colloc_from_design(c, pinn_ctx::COL_RAD, n_design, first, count);   // (no source and no fields here: refused above)
  if (!in_place) {
    c->rad.filled = false;
    c->sets_dirty = true;
    if (int rc = ensure_sets(c)) return rc;
  }
  if (int rc = rad_draw(c, n_pool, seed, k, c_add)) return rc;
  c->rad.filled = true;
  return 0;
}

int pinn_get_collocation(pinn_ctx* c, double* X, int64_t n) {
  REQUIRE(c && (X || n == 0), "null");
  REQUIRE(!is_disc(c), "pinn_get_collocation: discrete-time models have stage sets");
  HIPCHK(hipSetDevice(c->device));
  int rc = ensure_sets(c);
  if (rc) return rc;
  REQUIRE(n == c->sd.n_f, "buffer holds %lld points, the collocation set has %d", (long long)n, c->sd.n_f);
  if (n == 0) return 0;
  const size_t off = (size_t)colloc_first(c->sd), rs = real_size(c);
  std::vector<char> hx((size_t)n * rs), ht((size_t)n * rs);
  HIPCHK(hipMemcpyAsync(hx.data(), c->xs.as<char>() + off * rs, hx.size(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(ht.data(), c->ts.as<char>() + off * rs, ht.size(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  for (int64_t i = 0; i < n; ++i) {
    X[2 * i] = c->dtype == PINN_F64 ? ((const double*)hx.data())[i] : (double)((const float*)hx.data())[i];
    X[2 * i + 1] = c->dtype == PINN_F64 ? ((const double*)ht.data())[i] : (double)((const float*)ht.data())[i];
  }
  return 0;
}

int pinn_set_data(pinn_ctx* c, const double* X_u, const double* u, int64_t n, int64_t n_total) {
  if (c && is_disc(c)) return fail(PINN_EINVAL, "pinn_set_data: discrete-time models take stage sets (pinn_disc_set_stage)");
  REQUIRE(c && ((X_u && u) || n == 0) && n >= 0 && n_total >= n, "bad data arguments");
  c->sets.Xu.assign(X_u, X_u + 2 * n);
  c->sets.U.assign(u, u + (size_t)c->nd.n_out * n);
  c->nu_total = n_total;
  c->sa.arr.reset[LAM_DATA] = c->pw.arr.reset[LAM_DATA] = true;
  c->sets_dirty = true;
  return 0;
}

int pinn_set_boundary(pinn_ctx* c, const double* X_lb, const double* X_ub, int64_t n, int64_t n_total) {
  if (c && is_disc(c)) return fail(PINN_EINVAL, "pinn_set_boundary: discrete-time models take stage sets (pinn_disc_set_stage)");
  REQUIRE(c && ((X_lb && X_ub) || n == 0) && n >= 0 && n_total >= n, "bad boundary arguments");
  REQUIRE(c->pde == PINN_PDE_SCHRODINGER || adr_family(c) || n == 0, "boundary pairs are Schrodinger-only");
  c->sets.Xlo.assign(X_lb, X_lb + 2 * n);
  c->sets.Xhi.assign(X_ub, X_ub + 2 * n);
  c->nb_total = n_total;
  c->pw.arr.reset[LAM_PAIRS] = true;
  c->sets_dirty = true;
  return 0;
}

// Robin points of the adr kind: alpha u + beta u_x = g at (x_j, t_j).  Every refusal stands in front of any device work and
// leaves the context as it was (the arrays are looked at first: they need no context); n = 0 removes the class.
int pinn_set_robin(pinn_ctx* c, const double* X_w, const double* alpha, const double* beta, const double* g, int64_t n,
                   int64_t n_total) {
  REQUIRE(n >= 0 && n_total >= n, "pinn_set_robin: bad counts (n %lld, n_total %lld)", (long long)n, (long long)n_total);
  REQUIRE(n <= (1 << 30), "pinn_set_robin: too many points (%lld)", (long long)n);
  REQUIRE(n == 0 || (X_w && alpha && beta && g), "pinn_set_robin: null array");
  for (int64_t j = 0; j < n; ++j) {
    REQUIRE(std::isfinite(X_w[2 * j]) && std::isfinite(X_w[2 * j + 1]), "pinn_set_robin: point %lld is not finite",
            (long long)j);
    REQUIRE(std::isfinite(alpha[j]) && std::isfinite(beta[j]) && std::isfinite(g[j]),
            "pinn_set_robin: alpha, beta or g of point %lld is not finite", (long long)j);
    REQUIRE(alpha[j] != 0.0 || beta[j] != 0.0, "pinn_set_robin: point %lld has alpha = beta = 0: it constrains nothing",
            (long long)j);
  }
  if (int rc = adr_extra_gate(c, EXTRAS[X_ROBIN], "pinn_set_robin")) return rc;
  c->robin.X.assign(X_w, X_w + 2 * n);
  c->robin.alpha.assign(alpha, alpha + n);
  c->robin.beta.assign(beta, beta + n);
  c->robin.gamma.assign((size_t)n, 0.0);           // (read by the adr2 kind alone: there this call means gamma = 0)
  c->robin.g.assign(g, g + n);
  c->robin.n_total = n_total;
  if (n == 0) c->robin.n = 0;
  c->sets_dirty = true;
  return 0;
}

// Three-term wall points of the adr2 kind: alpha u + beta u_x + gamma u_t = g at (x_j, t_j).  pinn_set_robin's order of
// refusals (the arrays first, then the context; nothing touched on a refusal) and its storage; n = 0 removes the class.
int pinn_set_robin3(pinn_ctx* c, const double* X_w, const double* alpha, const double* beta, const double* gamma,
                    const double* g, int64_t n, int64_t n_total) {
  REQUIRE(n >= 0 && n_total >= n, "pinn_set_robin3: bad counts (n %lld, n_total %lld)", (long long)n, (long long)n_total);
  REQUIRE(n <= (1 << 30), "pinn_set_robin3: too many points (%lld)", (long long)n);
  REQUIRE(n == 0 || (X_w && alpha && beta && gamma && g), "pinn_set_robin3: null array");
  for (int64_t j = 0; j < n; ++j) {
    REQUIRE(std::isfinite(X_w[2 * j]) && std::isfinite(X_w[2 * j + 1]), "pinn_set_robin3: point %lld is not finite",
            (long long)j);
    REQUIRE(std::isfinite(alpha[j]) && std::isfinite(beta[j]) && std::isfinite(gamma[j]) && std::isfinite(g[j]),
            "pinn_set_robin3: alpha, beta, gamma or g of point %lld is not finite", (long long)j);
    REQUIRE(alpha[j] != 0.0 || beta[j] != 0.0 || gamma[j] != 0.0,
            "pinn_set_robin3: point %lld has alpha = beta = gamma = 0: it constrains nothing", (long long)j);
  }
  REQUIRE(c, "pinn_set_robin3: null context");
  if (!is_adr2(c))
    return fail(PINN_EUNSUPPORTED, "pinn_set_robin3: three-term wall points are for the adr2 kind (pde 10) only");
  if (int rc = adr_extra_gate(c, EXTRAS[X_ROBIN], "pinn_set_robin3")) return rc;
  c->robin.X.assign(X_w, X_w + 2 * n);
  c->robin.alpha.assign(alpha, alpha + n);
  c->robin.beta.assign(beta, beta + n);
  c->robin.gamma.assign(gamma, gamma + n);
  c->robin.g.assign(g, g + n);
  c->robin.n_total = n_total;
  if (n == 0) c->robin.n = 0;
  c->sets_dirty = true;
  return 0;
}

// r_j = alpha_j u + beta_j u_x - g_j at the current weights: the generic forward sweep over the set, then k_robin_residual
int pinn_robin_residual(pinn_ctx* c, double* out, int64_t n) {
  REQUIRE(c, "null");
  if (!has_walls(c))
    return fail(PINN_EUNSUPPORTED, "pinn_robin_residual: Robin points are for the adr kind (pde 5) and the adr2 kind (pde 10) only");
  REQUIRE(n == (int64_t)(c->robin.X.size() / 2),
          "pinn_robin_residual: buffer holds %lld values, the context has %lld Robin points", (long long)n,
          (long long)(c->robin.X.size() / 2));
  if (n == 0) return 0;
  REQUIRE(out, "null");
  HIPCHK(hipSetDevice(c->device));
  if (int rc = ensure_sets(c)) return rc;
  HIPCHK(c->robin.out.reserve((size_t)n));
  if (int rc = forward_taylor(c, c->xs, c->ts, c->sd.n_pad, c->chunk, c->O)) return rc;
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  by_real(c, [&](auto r) {
    using real = decltype(r);
    if (is_adr2(c))                            // + gamma_j u_t
      hipLaunchKernelGGL((k_robin3_residual<real>), grid, block, 0, c->stream, pde_coef<real, PDE_ADR2>(c),
                         c->O.as<vec4<real>>(), c->tgt.as<real>(), c->robin.out);
    else
      hipLaunchKernelGGL((k_robin_residual<real>), grid, block, 0, c->stream, pde_coef<real, PDE_ADR_ROBIN>(c),
                         c->O.as<vec4<real>>(), c->tgt.as<real>(), c->robin.out);
  });
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, c->robin.out, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

// Source term of the adr kind: f_i = N[u](x_i, t_i) - s_i at local collocation point i.  Every refusal stands in front of any
// device work and leaves the context as it was (the array is looked at first: it needs no context); n = 0 removes the source.
int pinn_set_source(pinn_ctx* c, const double* s, int64_t n) {
  REQUIRE(n >= 0, "pinn_set_source: bad count (n %lld)", (long long)n);
  REQUIRE(n <= (1 << 30), "pinn_set_source: too many values (%lld)", (long long)n);
  REQUIRE(n == 0 || s, "pinn_set_source: null array");
  for (int64_t i = 0; i < n; ++i) REQUIRE(std::isfinite(s[i]), "pinn_set_source: value %lld is not finite", (long long)i);
  if (int rc = adr_extra_gate(c, EXTRAS[X_SRC], "pinn_set_source")) return rc;
  REQUIRE(n == 0 || n == n_colloc(c), "pinn_set_source: %lld values for %lld local collocation points", (long long)n,
          (long long)n_colloc(c));
  HIPCHK(hipSetDevice(c->device));
  // the set is assembled and the block has this length: one copy into the collocation block of tgt (zeros on removal), no
  // re-assembly; an in-place LHS redraw leaves the set in this state too
  const bool in_place = !c->sets_dirty && c->tgt && (n == 0 || c->sd.n_f == n);
  if (in_place && c->sd.n_f > 0) {
    const size_t off = (size_t)colloc_first(c->sd), rs = real_size(c);
    if (n == 0) {
      HIPCHK(hipMemsetAsync(c->tgt.as<char>() + off * rs, 0, (size_t)c->sd.n_f * rs, c->stream));
      HIPCHK(hipStreamSynchronize(c->stream));
    } else if (upload_real(c, c->tgt.as<char>() + off * rs, s, (size_t)n)) return PINN_EHIP;
  }
  if (n == 0) { c->src.s.clear(); c->src.s.shrink_to_fit(); }
  else c->src.s.assign(s, s + n);
  c->src.on = n > 0;
  c->src.stale = false;
  if (!in_place) c->sets_dirty = true;
  return 0;
}

// Coefficient fields of the adr kind: row i of K holds (a0, a1, nu, r1, r2, r3) of local collocation point i.  pinn_set_source's
// order of refusals and its placement: the array first, then the context, nothing touched on a refusal; n = 0 removes them.
int pinn_set_coef_fields(pinn_ctx* c, const double* K, int64_t n) {
  REQUIRE(n >= 0, "pinn_set_coef_fields: bad count (n %lld)", (long long)n);
  REQUIRE(n <= (1 << 28), "pinn_set_coef_fields: too many rows (%lld)", (long long)n);
  REQUIRE(n == 0 || K, "pinn_set_coef_fields: null array");
  // a row is refused where pinn_set_pde_params refuses a constant set of the adr kind: a coefficient that is not finite
  for (int64_t i = 0; i < 6 * n; ++i)
    REQUIRE(std::isfinite(K[i]), "pinn_set_coef_fields: coefficient %d of row %lld is not finite", (int)(i % 6),
            (long long)(i / 6));
  if (int rc = adr_extra_gate(c, EXTRAS[X_KF], "pinn_set_coef_fields")) return rc;
  REQUIRE(n == 0 || n == n_colloc(c), "pinn_set_coef_fields: %lld rows for %lld local collocation points", (long long)n,
          (long long)n_colloc(c));
  HIPCHK(hipSetDevice(c->device));
  // the set is assembled and the block has this length: one copy into the device table, no re-assembly (an in-place LHS redraw
  // leaves the set in this state too).  Removal needs no device work: the table is not read without fields
  const bool in_place = !c->sets_dirty && c->tgt &&
                        (n == 0 || (c->sd.n_f == n && c->kf.dev.capacity_bytes() >= (size_t)6 * n * real_size(c)));
  if (in_place && n > 0) {
    if (upload_real(c, c->kf.dev, K, (size_t)6 * n)) return PINN_EHIP;
  }
  if (n == 0) { c->kf.K.clear(); c->kf.K.shrink_to_fit(); }
  else c->kf.K.assign(K, K + 6 * n);
  c->kf.on = n > 0;
  c->kf.stale = false;
  if (!in_place) c->sets_dirty = true;
  return 0;
}

int pinn_set_pde_params(pinn_ctx* c, const double* p, int n) {
  REQUIRE(c && p && n >= 1, "bad pde params");
  if (is_adr2(c)) {                       // a0, a1, nu, r1, r2, r3, b, kappa: any sign; nothing changes on a refusal
    REQUIRE(n == 8, "pinn_set_pde_params: the adr2 kind takes 8 coefficients (a0, a1, nu, r1, r2, r3, b, kappa), got %d", n);
    for (int i = 0; i < 8; ++i) REQUIRE(std::isfinite(p[i]), "pinn_set_pde_params: coefficient %d is not finite", i);
    for (int i = 0; i < 8; ++i) c->adr[i] = p[i];
    c->nu = p[2];
    return 0;
  }
  if (is_adr(c) || is_adr_disc(c)) {      // a0, a1, nu, r1, r2, r3; nothing changes on a refusal
    REQUIRE(n == 6, "pinn_set_pde_params: the adr kind takes 6 coefficients (a0, a1, nu, r1, r2, r3), got %d", n);
    for (int i = 0; i < 6; ++i) REQUIRE(std::isfinite(p[i]), "pinn_set_pde_params: coefficient %d is not finite", i);
    for (int i = 0; i < 6; ++i) c->adr[i] = p[i];
    c->nu = p[2];
    return 0;
  }
  if (is_adrd_disc(c)) {  // raw a0, a1, nu, r1, r2, r3, d3 -> the tail of theta; nu == 0 is allowed (the flag); nothing changes on a refusal
    REQUIRE(n == 7, "pinn_set_pde_params: the adrd_disc kind takes 7 coefficients (a0, a1, nu, r1, r2, r3, d3), got %d", n);
    for (int i = 0; i < 7; ++i) REQUIRE(std::isfinite(p[i]), "pinn_set_pde_params: coefficient %d is not finite", i);
    REQUIRE(p[2] >= 0.0, "pinn_set_pde_params: the adrd_disc kind stores log nu, so nu must be positive or exactly 0 (got %g)", p[2]);
    REQUIRE(p[2] > 0.0 || !(c->adr_mask & 4), "pinn_set_pde_params: nu must be positive to be trained (the nu bit of the "
            "trainable mask is set)");
    return adr_ide_write_tail(c, p);
  }
  if (has_adr_tail(c)) {  // raw a0, a1, nu, r1, r2, r3 -> the tail of theta; nothing changes on a refusal
    const char* kind = is_adr_ide(c) ? "adr_ide" : "adr_disc_ide";
    REQUIRE(n == 6, "pinn_set_pde_params: the %s kind takes 6 coefficients (a0, a1, nu, r1, r2, r3), got %d", kind, n);
    for (int i = 0; i < 6; ++i) REQUIRE(std::isfinite(p[i]), "pinn_set_pde_params: coefficient %d is not finite", i);
    REQUIRE(p[2] > 0.0, "pinn_set_pde_params: the %s kind stores log nu, so nu must be positive (got %g)", kind, p[2]);
    return adr_ide_write_tail(c, p);
  }
  c->nu = p[0];
  return 0;
}

int pinn_get_pde_params(pinn_ctx* c, double* p, int n) {
  REQUIRE(c && p, "null");
  if (is_adr2(c)) {
    REQUIRE(n == 8, "pinn_get_pde_params: this kind has 8 coefficients (a0, a1, nu, r1, r2, r3, b, kappa), got %d", n);
    for (int i = 0; i < 8; ++i) p[i] = c->adr[i];
    return 0;
  }
  if (is_adrd_disc(c)) REQUIRE(n == 7, "pinn_get_pde_params: this kind has 7 coefficients (a0, a1, nu, r1, r2, r3, d3), got %d", n);
  else if (is_adr(c) || has_adr_tail(c) || is_adr_disc(c)) REQUIRE(n == 6, "pinn_get_pde_params: this kind has 6 coefficients (a0, a1, nu, r1, r2, r3), got %d", n);
  else REQUIRE(n == 1, "pinn_get_pde_params: this kind has 1 parameter (nu), got %d", n);
  if (has_adr_tail(c)) {
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(p, c->theta + c->nd.n_net, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    p[2] = c->nu_off ? 0.0 : std::exp(p[2]);
  } else if (is_adr(c) || is_adr_disc(c)) {
    for (int i = 0; i < 6; ++i) p[i] = c->adr[i];
  } else {
    p[0] = c->nu;
  }
  return 0;
}

int pinn_set_pde_trainable(pinn_ctx* c, int mask) {
  REQUIRE(c, "null");
  if (!has_adr_tail(c))
    return fail(PINN_EUNSUPPORTED, "pinn_set_pde_trainable: only the adr_ide kind (pde 6) and its discrete-time form, the "
                "adr_disc_ide kind (pde 8), have trainable coefficients to choose from");
  if (is_adrd_disc(c)) {
    REQUIRE(mask >= 0 && mask <= 127, "pinn_set_pde_trainable: mask %d is outside 0..127 (bit k = coefficient k of a0, a1, nu, r1, r2, r3, d3)", mask);
    REQUIRE(!(mask & 4) || !c->nu_off, "pinn_set_pde_trainable: nu must be positive to be trained (it is 0: pinn_set_pde_params)");
    c->adr_mask = mask;
    return 0;
  }
  REQUIRE(mask >= 0 && mask <= 63, "pinn_set_pde_trainable: mask %d is outside 0..63 (bit k = coefficient k of a0, a1, nu, r1, r2, r3)", mask);
  c->adr_mask = mask;
  return 0;
}

int pinn_set_weights(pinn_ctx* c, const double* w, int64_t n) {
  REQUIRE(c && w, "null");
  REQUIRE(n == c->nd.n_theta, "weight vector has %lld entries, expected %d", (long long)n, c->nd.n_theta);
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpyAsync(c->theta, w, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
  int rc = cast_weights(c);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(c->stream));
  c->xg.poisoned = false;
  return 0;
}

// Device-side copies of the weight vector, in stream order: what the restart guard of NeuralNetwork.nt_optimization goes back
// to.  Nothing crosses the bus and nothing synchronises, so a snapshot can be taken behind every chunk of iterations that is
// still in flight.
int pinn_weights_snapshot(pinn_ctx* c, int slot) {
  REQUIRE(c && slot >= 0 && slot < pinn_ctx::N_SNAP, "snapshot slot %d outside 0..%d", slot, pinn_ctx::N_SNAP - 1);
  HIPCHK(hipSetDevice(c->device));
  const size_t bytes = (size_t)c->nd.n_theta * 8;
  HIPCHK(c->snap.reserve_bytes(bytes * pinn_ctx::N_SNAP));
  HIPCHK(hipMemcpyAsync(c->snap + (size_t)slot * c->nd.n_theta, c->theta, bytes, hipMemcpyDeviceToDevice, c->stream));
  c->snap_valid |= 1u << slot;
  return 0;
}

int pinn_weights_restore(pinn_ctx* c, int slot) {
  REQUIRE(c && slot >= 0 && slot < pinn_ctx::N_SNAP, "snapshot slot %d outside 0..%d", slot, pinn_ctx::N_SNAP - 1);
  REQUIRE(c->snap && (c->snap_valid >> slot & 1u), "no snapshot in slot %d", slot);
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpyAsync(c->theta, c->snap + (size_t)slot * c->nd.n_theta, (size_t)c->nd.n_theta * 8, hipMemcpyDeviceToDevice, c->stream));
  if (int rc = cast_weights(c)) return rc;           // the compute-dtype mirror and the LDS image follow, as in pinn_set_weights
  c->xg.poisoned = false;
  return 0;
}

int pinn_get_weights(pinn_ctx* c, double* w, int64_t n) {
  REQUIRE(c && w, "null");
  REQUIRE(n == c->nd.n_theta, "weight vector has %lld entries, expected %d", (long long)n, c->nd.n_theta);
  if (c->xg.poisoned)
    return fail(PINN_ESTATE, "the weights are undefined: a mailbox peer was lost in the middle of an optimiser step "
                             "(PINN_ECOMM was returned); restore them with pinn_set_weights");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpyAsync(w, c->theta, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

int pinn_loss_grad(pinn_ctx* c, double* loss, double* grad, double* terms) {
  REQUIRE(c, "null");
  if (int rc0 = src_fresh(c, "pinn_loss_grad")) return rc0;
  HIPCHK(hipSetDevice(c->device));
  const Range rg("pinn_loss_grad");
  int rc = eval_loss_grad(c);
  if (rc) return rc;
  std::vector<double> h(c->R);
  HIPCHK(hipMemcpyAsync(h.data(), c->gl, (size_t)c->R * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if ((rc = xg_check(c))) return rc;
  const int P = c->nd.n_theta;
  if (loss) *loss = h[P] + h[P + 1] + h[P + 2];
  if (terms) { terms[0] = h[P]; terms[1] = h[P + 1]; terms[2] = h[P + 2]; }
  if (grad) memcpy(grad, h.data(), (size_t)P * 8);
  return 0;
}

int pinn_adam_init(pinn_ctx* c, double lr, double beta1, double beta2, double eps) {
  REQUIRE(c, "null");
  REQUIRE(lr > 0 && beta1 >= 0 && beta1 < 1 && beta2 >= 0 && beta2 < 1 && eps >= 0, "bad Adam hyper-parameters");
  HIPCHK(hipSetDevice(c->device));
  c->adam.lr = lr; c->adam.b1 = beta1; c->adam.b2 = beta2; c->adam.eps = eps; c->adam.t = 0;
  HIPCHK(hipMemsetAsync(c->adam_m, 0, (size_t)c->nd.n_theta * 8, c->stream));
  HIPCHK(hipMemsetAsync(c->adam_v, 0, (size_t)c->nd.n_theta * 8, c->stream));
  c->adam.ready = true;
  return 0;
}

// ---- chunks in flight (see pinn_ctx::Pending) ----------------------------------------------------------------------
// the slot of the next ticket, with pinned room for n_loss doubles / n_iter ints (+ an L-BFGS state when asked)
static int pend_reserve(pinn_ctx* c, int kind, size_t n_loss, size_t n_iter, bool want_state, pinn_ctx::Pending** out) {
  REQUIRE(c->tk.room(), "%d chunks are in flight already: collect the oldest ticket first", N_PENDING);
  pinn_ctx::Pending& p = c->tk.pend[c->tk.next_slot()];
  if (!p.ev) HIPCHK(hipEventCreateWithFlags(&p.ev, hipEventDisableTiming));
  if (n_loss > 0) HIPCHK(p.h_loss.reserve(n_loss < 64 ? 64 : n_loss));      // at least 64 entries; nothing for none
  if (n_iter > 0) HIPCHK(p.h_iter.reserve(n_iter < 64 ? 64 : n_iter));
  if (want_state) HIPCHK(p.h_state.reserve(1));
  p.kind = kind;
  *out = &p;
  return 0;
}

// the chunk in slot p is complete in the stream: its event, its number, the counter
static int ticket_issue(pinn_ctx* c, pinn_ctx::Pending* p, int* ticket) {
  HIPCHK(hipEventRecord(p->ev, c->stream));
  if (ticket) *ticket = c->tk.next_number();
  c->tk.issued += 1;
  return 0;
}

// *pp = the chunk of `ticket`, which must be the oldest in flight and of `kind`, waited for and counted as collected
static int ticket_oldest(pinn_ctx* c, int ticket, int kind, pinn_ctx::Pending** pp) {
  REQUIRE(c, "null");
  REQUIRE(c->tk.is_oldest(ticket),
          "ticket %d is not the oldest chunk in flight (tickets are collected in the order they were issued)", ticket);
  pinn_ctx::Pending& p = c->tk.pend[c->tk.oldest_slot()];
  REQUIRE(p.kind == kind, kind == 1 ? "ticket %d belongs to an L-BFGS chunk" : "ticket %d belongs to an Adam chunk", ticket);
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipEventSynchronize(p.ev));
  c->tk.collected += 1;
  *pp = &p;
  return 0;
}

// the next Adam step of c: its counter, and the bias correction every step size of that step is formed from
static AdamFactors adam_step_factors(pinn_ctx* c) {
  c->adam.t += 1;
  return AdamFactors(c->adam.b1, c->adam.b2, (double)c->adam.t);
}

// n_steps Adam iterations into the stream.  record = false: nothing is kept (pinn_adam_run with losses == NULL).
static int adam_issue(pinn_ctx* c, int n_steps, bool record, int* ticket) {
  REQUIRE(c && n_steps >= 0, "bad arguments");
  if (int rc0 = src_fresh(c, "pinn_adam_run / pinn_adam_enqueue")) return rc0;
  REQUIRE(c->adam.ready, "pinn_adam_init has not been called");
  HIPCHK(hipSetDevice(c->device));
  const Range rg("pinn_adam_run");
  pinn_ctx::Pending* p = nullptr;
  double* region = nullptr;
  if (record) {
    if (int rc = pend_reserve(c, 1, (size_t)3 * (n_steps > 0 ? n_steps : 1), 0, false, &p)) return rc;
    const size_t steps = ring_steps(n_steps);
    if (ring_must_grow(steps, c->adam.loss_hist.capacity_bytes())) {
      // a larger ring: the chunks in flight finish first (their copies into the pinned buffers are then complete and the
      // tickets stay collectable), only then is the device ring replaced
      if (c->tk.outstanding() > 0) HIPCHK(hipStreamSynchronize(c->stream));
      HIPCHK(c->adam.loss_hist.reserve(ring_doubles(steps)));
      c->adam.hist_stride = steps;
    }
    region = c->adam.loss_hist + ring_region(c->tk, c->adam.hist_stride);
    p->n = n_steps; p->want_terms = c->adam.want_terms;
  }
  const int n = c->nd.n_theta;
  for (int s = 0; s < n_steps; ++s) {
    const AdamFactors bc = adam_step_factors(c);
    const double alpha = bc.alpha(c->adam.lr);
    double* slot = region ? region + (size_t)3 * s : nullptr;
    if (!c->comm || c->xg.on) {                   // reduction (+ mailbox all-reduce) + update in one kernel
      AdamFuse af{alpha, slot};
      if (c->sa.on && c->sa.lr > 0.0)             // self-adaptive weights: the ascent, same counter, same form
        af.alpha_sa = bc.alpha(c->sa.lr);
      if (c->pw.on && (c->pw.rate[0] > 0.0 || c->pw.rate[1] > 0.0 || c->pw.rate[2] > 0.0))   // adr point weights, likewise
        af.bc_pw = bc.bc_pw();
      if (int rc = eval_loss_grad(c, &af)) return rc;
      continue;
    }
    if (int rc = eval_loss_grad(c)) return rc;    // reduce -> RCCL all-reduce -> update
    by_real(c, [&](auto r) {
      using real = decltype(r);
      hipLaunchKernelGGL((k_adam<real>), dim3((n + 255) / 256), dim3(256), 0, c->stream, n, c->gl, c->theta,
                         c->theta_r.as<real>(), c->adam_m, c->adam_v, alpha, c->adam.b1, c->adam.b2, c->adam.eps, slot, n, c->nd,
                         c->img);
    });
  }
  HIPCHK(hipGetLastError());
  if (!record) return 0;
  if (n_steps > 0) HIPCHK(hipMemcpyAsync(p->h_loss, region, (size_t)3 * n_steps * 8, hipMemcpyDeviceToHost, c->stream));
  return ticket_issue(c, p, ticket);
}

int pinn_adam_collect(pinn_ctx* c, int ticket, double* losses) {
  pinn_ctx::Pending* pp = nullptr;
  if (int rc = ticket_oldest(c, ticket, 1, &pp)) return rc;
  const pinn_ctx::Pending& p = *pp;
  if (int rc = xg_check(c)) return rc;          // a lost mailbox peer: the steps after it were not applied
  if (losses) {
    if (p.want_terms) memcpy(losses, p.h_loss, (size_t)3 * p.n * 8);
    else for (int s = 0; s < p.n; ++s) losses[s] = p.h_loss[3 * s] + p.h_loss[3 * s + 1] + p.h_loss[3 * s + 2];
  }
  return 0;
}

int pinn_adam_run(pinn_ctx* c, int n_steps, double* losses) {
  REQUIRE(c && n_steps >= 0, "bad arguments");
  if (n_steps == 0) return 0;
  if (!losses) return adam_issue(c, n_steps, false, nullptr);
  REQUIRE(c->tk.outstanding() == 0, "pinn_adam_run: %d chunk(s) are in flight; collect them first", c->tk.outstanding());
  int ticket = 0;
  if (int rc = adam_issue(c, n_steps, true, &ticket)) return rc;
  return pinn_adam_collect(c, ticket, losses);
}

int pinn_adam_enqueue(pinn_ctx* c, int n_steps, int* ticket) {
  REQUIRE(c && ticket && n_steps >= 1, "bad arguments");
  return adam_issue(c, n_steps, true, ticket);
}

// the chunk of pinn_adam_run_terms: pinn_adam_collect hands back 3 n values, (residual, data, boundary) before every update
int pinn_adam_enqueue_terms(pinn_ctx* c, int n_steps, int* ticket) {
  REQUIRE(c && ticket && n_steps >= 1, "bad arguments");
  c->adam.want_terms = true;
  const int rc = adam_issue(c, n_steps, true, ticket);
  c->adam.want_terms = false;
  return rc;
}

int pinn_adam_run_terms(pinn_ctx* c, int n_steps, double* terms3) {
  REQUIRE(c && terms3, "null");
  c->adam.want_terms = true;
  const int rc = pinn_adam_run(c, n_steps, terms3);
  c->adam.want_terms = false;
  return rc;
}

// pinn_lbfgs_begin up to the initial evaluation; *eval = 0: nothing follows (max_iter == 0)
static int lbfgs_begin_setup(pinn_ctx* c, int max_iter, double lr, int n_corr, double tol_fun, double tol_x,
                             double max_eval, bool* eval) {
  *eval = false;
  REQUIRE(c && max_iter >= 0 && n_corr >= 1 && lr > 0, "bad L-BFGS arguments");
  if (int rc0 = src_fresh(c, "pinn_lbfgs_begin")) return rc0;
  HIPCHK(hipSetDevice(c->device));
  const size_t n = c->nd.n_theta;
  auto& lb = c->lbfgs;
  lb.max_iter = max_iter; lb.lr = lr; lb.ncorr = n_corr; lb.tol_fun = tol_fun; lb.tol_x = tol_x;
  lb.max_eval = max_eval > 0 ? max_eval : 1.25 * max_iter;        // custom_lbfgs.py:50
  if (c->tk.outstanding() > 0) {                                   // a restart: chunks still in flight are waited for and
    HIPCHK(hipStreamSynchronize(c->stream));                       // forgotten (their results are dropped)
    c->tk.drop_all();
  }
  lb.iters_issued = 0; lb.logged_read = 0; lb.issued_at_read = 0; lb.post_pending = false; lb.ready = false;
  if (max_iter == 0) { lb.ready = true; return 0; }                // custom_lbfgs.py:43-44
  const int M1 = lb.M1 = n_corr + 1;                               // ring slots (compact mode)
  // compact mode needs the two padded Gram matrices in LDS (<= 64 KiB) and one lane per slot
  lb.mode_active = (lb.mode == 1 && M1 <= LBC_MAXSLOTS) ? 1 : 0;
  if (lb.mode_active && lbc_coef_apply_lds_bytes(M1) > 64 * 1024) {
    const int lds = (int)lbc_coef_apply_lds_bytes(M1);
    HIPCHK(hipFuncSetAttribute((const void*)k_lbc_coef_apply<float>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    HIPCHK(hipFuncSetAttribute((const void*)k_lbc_coef_apply<double>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  }
  // (sizes of a context's lifetime: allocated once.)  zero: unused ring slots must read as finite; Gram matrices,
  // coefficients, dots and the extra record start at zero
  const size_t m1 = M1, ring = m1 * ring_ld((int)n), gram = 2 * m1 * m1, dots = 2 * (5 * m1 + LBC_NSCAL);
  const struct { DevBuf<double>* buf; size_t count; bool zero; } bufs[] = {
      {&lb.x, n, false},    {&lb.d, n, false},    {&lb.gold, n, false},  {&lb.q, n, false},     {&lb.al, m1, false},
      {&lb.S, ring, true},  {&lb.Y, ring, true},  {&lb.cs, m1, true},    {&lb.cy, m1, true},    {&lb.SY, gram, true},
      {&lb.YY, gram, true}, {&lb.ro, 2 * m1, true}, {&lb.dots, dots, true}};
  static_assert(sizeof(LbcExtra) % 8 == 0, "LbcExtra is cleared as doubles");
  ZeroList zl{};
  auto add = [&](void* p, size_t doubles) { zl.p[zl.count] = (double*)p; zl.n[zl.count] = doubles; zl.count++; };
  for (const auto& b : bufs) {
    HIPCHK(b.buf->reserve(b.count));
    if (b.zero) add(b.buf->get(), b.count);
  }
  HIPCHK(lb.state.reserve(2));
  HIPCHK(lb.ex.reserve(1));
  add(lb.ex, sizeof(LbcExtra) / 8);
  // the optimiser state starts as {0..., Hdiag = 1}: written by the same launch (no host buffer in flight)
  static_assert(sizeof(LbfgsState) % 8 == 0 && offsetof(LbfgsState, Hdiag) % 8 == 0, "LbfgsState is initialised as doubles");
  zl.state = (double*)lb.state.get(); zl.state_doubles = (int)(sizeof(LbfgsState) / 8);
  zl.hdiag_index = (int)(offsetof(LbfgsState, Hdiag) / 8);
  hipLaunchKernelGGL(k_zero_list, dim3(256), dim3(256), 0, c->stream, zl);
  HIPCHK(hipGetLastError());
  lb.flip = 0;
  HIPCHK(lb.log_loss.reserve((size_t)max_iter + 1));
  HIPCHK(lb.log_iter.reserve((size_t)max_iter + 1));
  HIPCHK(hipMemcpyAsync(lb.x, c->theta, n * 8, hipMemcpyDeviceToDevice, c->stream));
  *eval = true;
  return 0;
}

// what follows an evaluation: its bookkeeping, break tests and log entry (initial = 1: pinn_lbfgs_begin's, :65-76)
static void lbfgs_post(pinn_ctx* c, int initial) {
  const auto& lb = c->lbfgs;
  const int n = c->nd.n_theta;
  hipLaunchKernelGGL(k_lbfgs_post, dim3(1), dim3(LB_THREADS), 0, c->stream, n, n, lb.max_iter, lb.max_eval, lb.tol_fun,
                     lb.tol_x, lb.state + lb.flip, c->gl, lb.d, lb.log_iter, lb.log_loss, initial);
}

// pinn_lbfgs_begin behind the initial evaluation
static int lbfgs_begin_post(pinn_ctx* c) {
  lbfgs_post(c, 1);
  HIPCHK(hipGetLastError());
  if (c->xg.on) {                                 // a lost mailbox peer in the first evaluation surfaces here
    HIPCHK(hipStreamSynchronize(c->stream));
    if (int rc2 = xg_check(c)) return rc2;
  }                                               // otherwise nothing is read back: pinn_lbfgs_run synchronises
  c->lbfgs.ready = true;
  return 0;
}

int pinn_lbfgs_begin(pinn_ctx* c, int max_iter, double lr, int n_corr, double tol_fun,
                     double tol_x, double max_eval) {
  bool eval = false;
  if (int rc = lbfgs_begin_setup(c, max_iter, lr, n_corr, tol_fun, tol_x, max_eval, &eval)) return rc;
  if (!eval) return 0;
  if (int rc = eval_loss_grad(c)) return rc;                       // :65
  return lbfgs_begin_post(c);
}

// ---- one chunk of L-BFGS iterations (pinn_lbfgs_run / _enqueue, pinn_ens_lbfgs_run) ----------------------------------------
// a context's share of a chunk: its pending slot (nullptr: max_iter == 0, the ticket is issued already), its log window
struct LbfgsMember { pinn_ctx* c; pinn_ctx::Pending* p; int window, ticket; };

// the chunk's pending slot, with pinned room for the window of log entries the chunk can have added
static int lbfgs_open(LbfgsMember& m, int n_iters) {
  pinn_ctx* c = m.c;
  REQUIRE(c && n_iters >= 0, "bad arguments");
  if (int rc0 = src_fresh(c, "pinn_lbfgs_run / pinn_lbfgs_enqueue")) return rc0;
  const auto& lb = c->lbfgs;
  REQUIRE(lb.ready, "pinn_lbfgs_begin has not been called");
  HIPCHK(hipSetDevice(c->device));
  pinn_ctx::Pending* p = nullptr;
  const int log_room = (int)(lb.log_iter.capacity_bytes() / sizeof(int));   // entries the two log arrays hold
  const int window = lbfgs_window(lb.iters_issued, lb.issued_at_read, n_iters, log_room, lb.logged_read, lb.max_iter);
  if (int rc = pend_reserve(c, 2, (size_t)window + 1, (size_t)window + 1, true, &p)) return rc;
  if (lb.max_iter == 0) { p->n = -1; return ticket_issue(c, p, &m.ticket); }   // custom_lbfgs.py:43-44: done at once
  m.p = p; m.window = window;
  return 0;
}

// one iteration's step kernels; -> an evaluation follows (not behind the last iteration)
static bool lbfgs_iter(pinn_ctx* c) {
  auto& lb = c->lbfgs;
  const int n = c->nd.n_theta;
  lb.iters_issued += 1;
  if (lb.mode_active) {
    const int M1 = lb.M1;
    const size_t lsh = lbc_coef_apply_lds_bytes(M1), mm = (size_t)M1 * M1;
    LbfgsState *st_in = lb.state + lb.flip, *st_out = lb.state + (lb.flip ^ 1);
    // dot products of this iteration: already formed behind the evaluation's reduction (one partial set per
    // 64-column tile; opt-in), or by k_lbc_dots (two half sets, one when n > 4096) -- also N > 1 ranks, the first
    // iteration after pinn_lbfgs_begin, an evaluation issued by somebody else in between
    const int n_part = n <= 2 * 2 * LBD_THREADS ? 2 : 1;   // two workgroups per ring slot, one pair stride each
    if (n_part == 2)
      hipLaunchKernelGGL(k_lbc_dots<2>, dim3(M1, 2), dim3(LBD_THREADS), 0, c->stream, n, M1, st_in, c->gl, lb.gold, lb.d,
                         lb.S, lb.Y, lb.dots);
    else
      hipLaunchKernelGGL(k_lbc_dots<1>, dim3(M1), dim3(LBD_THREADS), 0, c->stream, n, M1, st_in, c->gl, lb.gold, lb.d,
                         lb.S, lb.Y, lb.dots);
    const double* pd = lb.dots;
    const dim3 agrid((n + 63) / 64);
    by_real(c, [&](auto r) {
      using real = decltype(r);
      hipLaunchKernelGGL((k_lbc_coef_apply<real>), agrid, dim3(LBC_THREADS), lsh, c->stream, n, M1, lb.ncorr, lb.max_iter,
                         lb.lr, lb.tol_x, lb.tol_fun, lb.max_eval, lb.post_pending ? 1 : 0, n, st_in, st_out, c->gl, pd,
                         n_part, lb.SY + lb.flip * mm, lb.YY + lb.flip * mm, lb.ro + lb.flip * M1,
                         lb.SY + (lb.flip ^ 1) * mm, lb.YY + (lb.flip ^ 1) * mm, lb.ro + (lb.flip ^ 1) * M1, lb.log_iter,
                         lb.log_loss, lb.S, lb.Y, lb.d, lb.gold, lb.x, c->theta, c->theta_r.as<real>(), c->nd, c->img);
    });
    lb.post_pending = false;
    lb.flip ^= 1;
  } else
    by_real(c, [&](auto r) {
      using real = decltype(r);
      hipLaunchKernelGGL((k_lbfgs_step<real>), dim3(1), dim3(LB_THREADS), 0, c->stream, n, lb.max_iter, lb.ncorr,
                         lb.lr, lb.tol_x, lb.state + lb.flip, c->gl, lb.x, c->theta, c->theta_r.as<real>(),
                         lb.d, lb.gold, lb.S, lb.Y, lb.ro, lb.al, lb.q, c->nd, c->img);
    });
  return lb.iters_issued != lb.max_iter;                           // last iteration: no re-evaluation
}

// the state and the log window to the chunk's pinned buffers, the ticket
static int lbfgs_close(LbfgsMember& m) {
  pinn_ctx* c = m.c;
  auto& lb = c->lbfgs;
  pinn_ctx::Pending* p = m.p;
  if (lb.post_pending) { lbfgs_post(c, 0); lb.post_pending = false; }   // the host is about to read the state: settle it
  HIPCHK(hipGetLastError());
  p->n = m.window; p->base = lb.logged_read; p->issued_upto = lb.iters_issued;
  HIPCHK(hipMemcpyAsync(p->h_state, lb.state + lb.flip, sizeof(LbfgsState), hipMemcpyDeviceToHost, c->stream));
  if (m.window > 0) {
    HIPCHK(hipMemcpyAsync(p->h_iter, lb.log_iter + p->base, (size_t)m.window * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(p->h_loss, lb.log_loss + p->base, (size_t)m.window * 8, hipMemcpyDeviceToHost, c->stream));
  }
  return ticket_issue(c, p, &m.ticket);
}

// Up to n_iters iterations of K >= 1 contexts into the stream -- a context that has issued its max_iter stops moving while
// the others go on -- then each one's state and log window on their way to its chunk's pinned buffers, and its ticket.
// eval(act) evaluates loss and gradient of the contexts with act[k] set (K = 1: eval_loss_grad; an ensemble: one launch for
// all its members).  Nothing is allocated here: m and act are the caller's.
extern "C++" {
template <typename Eval>
static int lbfgs_chunk(LbfgsMember* m, char* act, int K, int n_iters, Eval&& eval) {
  for (int k = 0; k < K; ++k)
    if (int rc = lbfgs_open(m[k], n_iters)) return rc;
  for (int s = 0; s < n_iters; ++s) {
    bool any = false;
    for (int k = 0; k < K; ++k) {
      pinn_ctx* c = m[k].c;
      act[k] = m[k].p && c->lbfgs.iters_issued < c->lbfgs.max_iter && lbfgs_iter(c);
      any = any || act[k];
    }
    if (!any) break;
    if (int rc = eval(act)) return rc;
    for (int k = 0; k < K; ++k) {
      if (!act[k]) continue;
      if (m[k].c->lbfgs.mode_active) m[k].c->lbfgs.post_pending = true;   // folded into the next k_lbc_coef_apply
      else lbfgs_post(m[k].c, 0);
    }
  }
  for (int k = 0; k < K; ++k)
    if (m[k].p) { if (int rc = lbfgs_close(m[k])) return rc; }
  return 0;
}
}  // extern "C++" (a template inside the API's extern "C" block)

static int lbfgs_issue(pinn_ctx* c, int n_iters, int* ticket) {
  const Range rg("pinn_lbfgs_run");
  LbfgsMember m{c, nullptr, 0, 0};
  char act = 0;
  if (int rc = lbfgs_chunk(&m, &act, 1, n_iters, [c](const char*) { return eval_loss_grad(c); })) return rc;
  *ticket = m.ticket;
  return 0;
}

int pinn_lbfgs_collect(pinn_ctx* c, int ticket, int cap, int* iters, double* losses, int* n_logged, int* done) {
  REQUIRE(cap >= 0, "bad arguments");
  pinn_ctx::Pending* pp = nullptr;
  if (int rc = ticket_oldest(c, ticket, 2, &pp)) return rc;
  const pinn_ctx::Pending& p = *pp;
  auto& lb = c->lbfgs;
  if (n_logged) *n_logged = 0;
  if (p.n < 0) { if (done) *done = 1; return 0; }
  if (int rc2 = xg_check(c)) return rc2;
  const LbfgsState hs = *p.h_state;
  const LbfgsHandout h = lbfgs_handout(hs.n_logged, lb.logged_read, p.base, p.n);
  REQUIRE(!(iters && losses) || h.fresh <= cap, "pinn_lbfgs_collect: %d log entries are due, the arrays hold %d", h.fresh, cap);
  if (h.fresh > 0 && iters && losses) {
    if (!h.inside)    // (never, over every chunking: tests/host/optim_host_check.cpp -- an invariant, so no device call here)
      return fail(PINN_ESTATE, "pinn_lbfgs_collect: log entries from %d on lie outside the chunk's window of %d", h.off, p.n);
    memcpy(iters, p.h_iter + h.off, (size_t)h.fresh * 4);
    memcpy(losses, p.h_loss + h.off, (size_t)h.fresh * 8);
  }
  lb.logged_read = hs.n_logged;
  lb.issued_at_read = p.issued_upto;
  if (n_logged) *n_logged = (iters && losses) ? h.fresh : 0;
  if (done) *done = hs.done;
  return 0;
}

// (the arrays hold n_iters entries: the tight bound with nothing in flight, include/pinn_hip.h)
int pinn_lbfgs_run(pinn_ctx* c, int n_iters, int* iters, double* losses, int* n_logged, int* done) {
  REQUIRE(c && n_iters >= 0, "bad arguments");
  REQUIRE(c->tk.outstanding() == 0, "pinn_lbfgs_run: %d chunk(s) are in flight; collect them first", c->tk.outstanding());
  int ticket = 0;
  if (int rc = lbfgs_issue(c, n_iters, &ticket)) return rc;
  return pinn_lbfgs_collect(c, ticket, n_iters, iters, losses, n_logged, done);
}

int pinn_lbfgs_enqueue(pinn_ctx* c, int n_iters, int* ticket) {
  REQUIRE(c && ticket && n_iters >= 1, "bad arguments");
  return lbfgs_issue(c, n_iters, ticket);
}

int pinn_lbfgs_set_mode(pinn_ctx* c, int mode) {
  REQUIRE(c && (mode == 0 || mode == 1), "mode must be 0 (reference operation order) or 1 (compact)");
  c->lbfgs.mode = mode;
  return 0;
}

int pinn_lbfgs_get_x(pinn_ctx* c, double* x, int64_t n) {
  REQUIRE(c && x && n == c->nd.n_theta, "bad arguments");
  REQUIRE(c->lbfgs.x, "no L-BFGS run yet");
  HIPCHK(hipSetDevice(c->device));
  // in stream order, as pinn_get_weights: the context's stream is non-blocking, so a copy on the null stream would not wait
  // for what pinn_lbfgs_begin or an enqueued chunk has still in flight (the copy of the start into lbfgs.x, a step kernel)
  HIPCHK(hipMemcpyAsync(x, c->lbfgs.x, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

int pinn_predict(pinn_ctx* c, const double* X, int64_t n, double* out) {
  REQUIRE(c && X && out && n >= 0, "bad arguments");
  HIPCHK(hipSetDevice(c->device));
  if (n == 0) return 0;
  if (is_disc(c))
    return disc_predict_any(c, 0, 0, X, n, out);
  const Range rg("pinn_predict");
  int n_pad = 0;
  if (int rc = eval_points(c, X, n, &n_pad)) return rc;
  if (int rc = predict_values(c, n, n_pad)) return rc;
  HIPCHK(hipMemcpyAsync(out, c->pred, (size_t)n * c->nd.n_out * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

int pinn_error_l2(pinn_ctx* c, const double* X, const double* ref, int64_t n, int kind, double* err) {
  REQUIRE(c && X && ref && err && n >= 1, "bad arguments");
  REQUIRE(kind == 0 || kind == 1, "kind must be 0 (element-wise over [n][n_out]) or 1 (modulus of the outputs against ref [n])");
  REQUIRE(!is_disc(c), "pinn_error_l2: not defined for discrete-time models");
  HIPCHK(hipSetDevice(c->device));
  const Range rg("pinn_error_l2");
  const int NO = c->nd.n_out;
  const size_t n_ref = kind == 1 ? (size_t)n : (size_t)n * NO;
  int n_pad = 0;
  if (int rc = eval_points(c, X, n, &n_pad)) return rc;
  if (c->ev_ref.size() != n_ref || memcmp(c->ev_ref.data(), ref, n_ref * 8) != 0) {
    c->ev_ref.clear();
    HIPCHK(c->d_ref.reserve(n_ref));
    HIPCHK(hipMemcpyAsync(c->d_ref, ref, n_ref * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->ev_ref.assign(ref, ref + n_ref);
  }
  if (int rc = predict_values(c, n, n_pad)) return rc;
  const int nb = (int)((n_ref + ERR_SPAN - 1) / ERR_SPAN);
  HIPCHK(c->err_partial.reserve((size_t)nb * 2));
  HIPCHK(c->err_res.reserve(3));
  HIPCHK(c->h_err.reserve(3));
  hipLaunchKernelGGL(k_err_partial, dim3(nb), dim3(ERR_THREADS), 0, c->stream, (const double*)c->pred,
                     (const double*)c->d_ref, (long long)n_ref, NO, kind, c->err_partial);
  hipLaunchKernelGGL(k_err_final, dim3(1), dim3(64), 0, c->stream, (const double*)c->err_partial, nb, c->err_res);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(c->h_err, c->err_res, 3 * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  *err = c->h_err[0];
  return 0;
}

int pinn_get_status(pinn_ctx* c, int64_t* n_evals, int64_t* first_nonfinite_eval) {
  REQUIRE(c, "null");
  HIPCHK(hipSetDevice(c->device));
  unsigned long long nf = 0;
  HIPCHK(hipMemcpyAsync(&nf, c->d_nonfinite, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (n_evals) *n_evals = (int64_t)c->n_evals;
  if (first_nonfinite_eval) *first_nonfinite_eval = (int64_t)nf;
  if (nf) fail(PINN_OK, "loss became non-finite at evaluation %llu of %llu", nf, c->n_evals);   // message only
  return 0;
}

int pinn_disc_set_stage(pinn_ctx* c, int set, const double* x, const double* target, int64_t n,
                        const double* M, int q) {
  REQUIRE(c, "null");
  REQUIRE(is_disc(c), "pinn_disc_set_stage: the context is not a discrete-time model");
  REQUIRE(set == 0 || set == 1, "stage set %d outside 0..1", set);
  REQUIRE(n >= 0 && n <= (1 << 24), "bad point count");
  REQUIRE(n == 0 || (x && target), "null argument");
  if (M) REQUIRE(q >= 1 && q <= c->nd.n_out, "q = %d outside 1..n_out (%d)", q, c->nd.n_out);
  pinn_ctx::DiscSet& ds = c->dset[set];
  ds.x.assign(x, x + n);
  ds.t.assign(target, target + n);
  ds.has_M = M != nullptr && n > 0;
  ds.q = ds.has_M ? q : 0;
  if (ds.has_M) ds.M.assign(M, M + (size_t)c->nd.n_out * q); else ds.M.clear();
  c->sets_dirty = true;
  return 0;
}

int pinn_disc_set_periodic(pinn_ctx* c, const double* x_lb, const double* x_ub, int64_t n, int order) {
  REQUIRE(c, "null");
  if (!has_pairs(c))
    return fail(PINN_EUNSUPPORTED, "pinn_disc_set_periodic: periodic pairs are for the adr_disc kind (pde 7) and the "
                "adr_disc_ide kind (pde 8) only");      // (and adrd_disc, pde 9; the wording is pinned by the earlier kinds' tests)
  REQUIRE(order == 0 || order == 1, "pinn_disc_set_periodic: order %d outside 0..1 (0: values, 1: values and slopes)", order);
  REQUIRE(n >= 0 && n <= (1 << 24), "pinn_disc_set_periodic: bad pair count");
  REQUIRE(n == 0 || (x_lb && x_ub), "pinn_disc_set_periodic: null argument");
  for (int64_t i = 0; i < n; ++i)
    REQUIRE(std::isfinite(x_lb[i]) && std::isfinite(x_ub[i]), "pinn_disc_set_periodic: pair %lld is not finite", (long long)i);
  c->dper.lb.assign(x_lb, x_lb + n);
  c->dper.ub.assign(x_ub, x_ub + n);
  c->dper.order = order;
  c->sets_dirty = true;
  return 0;
}

int pinn_disc_predict(pinn_ctx* c, int set, const double* x, int64_t n, double* out) {
  REQUIRE(c && x && out && n >= 0, "bad arguments");
  REQUIRE(is_disc(c), "pinn_disc_predict: the context is not a discrete-time model");
  REQUIRE(set == 0 || set == 1, "stage set %d outside 0..1", set);
  HIPCHK(hipSetDevice(c->device));
  if (n == 0) return 0;
  int rc = disc_ensure(c);      // uploads the tables
  if (rc) return rc;
  return disc_predict_any(c, 1, set, x, n, out);
}

int pinn_residual(pinn_ctx* c, double* f, int64_t n) {
  if (c && is_disc(c)) return fail(PINN_EUNSUPPORTED, "pinn_residual: not defined for discrete-time models");
  REQUIRE(c && f, "null");
  if (int rc0 = src_fresh(c, "pinn_residual")) return rc0;
  HIPCHK(hipSetDevice(c->device));
  int rc = ensure_sets(c);
  if (rc) return rc;
  const SetDesc sd = c->sd;
  const bool ide = c->pde == PINN_PDE_BURGERS_IDE;
  const int first = ide ? data_first(sd) : colloc_first(sd);
  const int cnt = ide ? sd.n_u : sd.n_f;
  REQUIRE(n == cnt, "residual buffer holds %lld points, the set has %d", (long long)n, cnt);
  if (cnt == 0) return 0;
  const int NO = c->nd.n_out;
  HIPCHK(c->f_out.reserve((size_t)cnt * NO));
  if (int rc2 = forward_taylor(c, c->xs, c->ts, sd.n_pad, c->chunk, c->O)) return rc2;
  if (int rc2 = launch_residual(c, AT_SET, c->O, first, cnt, sd.n_pad, c->f_out)) return rc2;
  HIPCHK(hipMemcpyAsync(f, c->f_out, (size_t)cnt * NO * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

int pinn_residual_at(pinn_ctx* c, const double* X, int64_t n, double* f) {
  if (c && is_disc(c)) return fail(PINN_EUNSUPPORTED, "pinn_residual_at: not defined for discrete-time models");
  REQUIRE(c && X && f && n >= 0, "bad arguments");
  if (c->kf.on)
    return fail(PINN_EUNSUPPORTED, "pinn_residual_at: this context holds coefficient fields, and the coefficients are not known at "
                "foreign points (pinn_residual gives f over the set; pinn_set_coef_fields with n = 0 removes the fields)");
  HIPCHK(hipSetDevice(c->device));
  if (n == 0) return 0;
  const int NO = c->nd.n_out;
  int n_pad = 0;
  if (int rc = eval_points(c, X, n, &n_pad)) return rc;
  const int chunk = n_pad < CHUNK_POINTS ? n_pad : CHUNK_POINTS;
  if (int rc = forward_taylor(c, c->xe, c->te, n_pad, chunk, c->Oe)) return rc;
  HIPCHK(c->f_out.reserve((size_t)n * NO));
  // (a context with a source: s is not known at foreign points, launch_residual leaves it out)
  if (int rc = launch_residual(c, AT_FOREIGN, c->Oe, 0, (int)n, n_pad, c->f_out)) return rc;
  HIPCHK(hipMemcpyAsync(f, c->f_out, (size_t)n * NO * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

int pinn_comm_unique_id(char* id128) {
  REQUIRE(id128, "null");
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is expected to be 128 bytes");
  ncclUniqueId id;
  NCCLCHK(ncclGetUniqueId(&id));
  memcpy(id128, &id, 128);
  return 0;
}

int pinn_comm_init(pinn_ctx* c, const char* id128, int n_ranks, int rank) {
  REQUIRE(c && id128 && n_ranks >= 1 && rank >= 0 && rank < n_ranks, "bad communicator arguments");
  if (int rc = single_device_only(c, "pinn_comm_init")) return rc;
  HIPCHK(hipSetDevice(c->device));
  if (c->comm) { ncclCommDestroy(c->comm); c->comm = nullptr; }
  xg_release(c);
  ncclUniqueId id;
  memcpy(&id, id128, 128);
  NCCLCHK(ncclCommInitRank(&c->comm, n_ranks, id, rank));
  c->n_ranks = n_ranks; c->rank = rank;
  t16_prepass_for_ranks(c, n_ranks);
  return 0;
}

int pinn_comm_xgmi_export(pinn_ctx* c, int n_ranks, int rank, char* handle64) {
  REQUIRE(c && handle64 && n_ranks >= 1 && n_ranks <= XG_MAX_RANKS && rank >= 0 && rank < n_ranks,
          "bad arguments (at most %d ranks)", XG_MAX_RANKS);
  if (int rc = single_device_only(c, "pinn_comm_xgmi_export")) return rc;
  static_assert(sizeof(hipIpcMemHandle_t) == 64, "hipIpcMemHandle_t is expected to be 64 bytes");
  HIPCHK(hipSetDevice(c->device));
  xg_release(c);
  const int Rp = (c->R + 63) / 64 * 64;
  const size_t bytes = xg_box_bytes(n_ranks, Rp);
  hipError_t e = hipExtMallocWithFlags(&c->xg.box, bytes, hipDeviceMallocUncached);
  if (e != hipSuccess) { c->xg.box = nullptr; return fail(PINN_EHIP, "mailbox allocation: %s", hipGetErrorString(e)); }
  HIPCHK(hipMemset(c->xg.box, 0, bytes));
  HIPCHK(c->xg.err.reserve(1));
  HIPCHK(hipMemset(c->xg.err, 0, sizeof(int)));
  HIPCHK(hipDeviceSynchronize());
  c->xg.peers = XgPeers{};
  c->xg.peers.n_ranks = n_ranks; c->xg.peers.rank = rank; c->xg.peers.Rp = Rp;
  hipIpcMemHandle_t h;
  e = hipIpcGetMemHandle(&h, c->xg.box);
  if (e != hipSuccess) { xg_release(c); return fail(PINN_EHIP, "hipIpcGetMemHandle: %s", hipGetErrorString(e)); }
  memcpy(handle64, &h, 64);
  return 0;
}

int pinn_comm_xgmi_attach(pinn_ctx* c, const char* handles, int n_handles, int* mapped_ok) {
  REQUIRE(c && handles && mapped_ok, "null");
  REQUIRE(c->xg.box && n_handles == c->xg.peers.n_ranks, "pinn_comm_xgmi_export first; one handle per rank");
  HIPCHK(hipSetDevice(c->device));
  int* self_test_ok = mapped_ok;
  *self_test_ok = 0;
  const int n = c->xg.peers.n_ranks, me = c->xg.peers.rank;
  // (a workgroup of the reduction kernel waits only for remote stores, never for another local workgroup, so the
  //  grid needs no co-residency guarantee)
  for (int r = 0; r < n; ++r) {
    void* base = c->xg.box;
    if (r != me) {
      hipIpcMemHandle_t h;
      memcpy(&h, handles + (size_t)64 * r, 64);
      hipError_t e = hipIpcOpenMemHandle(&c->xg.opened[r], h, hipIpcMemLazyEnablePeerAccess);
      if (e != hipSuccess) { c->xg.opened[r] = nullptr; (void)hipGetLastError(); return 0; }   // stay on RCCL
      base = c->xg.opened[r];
    }
    c->xg.peers.box[r] = (xg_line_t*)base;
    if (r != me) {                               // does that peer's mailbox live on MY device?  (ranks sharing one GPU)
      hipPointerAttribute_t at;
      if (hipPointerGetAttributes(&at, base) == hipSuccess && at.device == c->device) ++c->xg.sharing;
      else (void)hipGetLastError();
    }
  }
  // ranks sharing the device: keep the polling workgroups of the reduction off most CUs (kernels_xgmi.h)
  c->xg.grid_cap = c->xg.sharing > 1 ? (c->n_cu / (4 * (c->xg.sharing - 1)) > 8 ? c->n_cu / (4 * (c->xg.sharing - 1)) : 8) : 0;
  if (const char* v = getenv("PINN_XGMI_GRID_CAP")) c->xg.grid_cap = atoi(v);
  c->xg.attached = true;
  t16_prepass_for_ranks(c, n_handles);
  *mapped_ok = 1;
  return 0;
}

int pinn_comm_xgmi_selftest(pinn_ctx* c, int* ok) {
  REQUIRE(c && ok, "null");
  REQUIRE(c->xg.attached, "pinn_comm_xgmi_attach first");
  HIPCHK(hipSetDevice(c->device));
  return xg_self_test(c, ok);
}

int pinn_comm_benchmark(pinn_ctx* c, int mode, int iters, double* us_per_iter) {
  REQUIRE(c && us_per_iter && iters >= 1 && (mode == 1 || mode == 2), "bad arguments");
  if (mode == 1) REQUIRE(c->comm, "no RCCL communicator");
  if (mode == 2) REQUIRE(c->xg.attached, "mailboxes are not attached");
  HIPCHK(hipSetDevice(c->device));
  const int R = c->R;
  DevBuf<double> vec, out;                       // the call's own: freed on every return
  HIPCHK(vec.reserve(R));
  HIPCHK(out.reserve(R));
  HIPCHK(hipMemsetAsync(vec, 0, (size_t)R * 8, c->stream));
  const dim3 grid((R + RED_COLS - 1) / RED_COLS), block(RED_THREADS);
  auto once = [&]() -> int {
    if (mode == 1) {
      hipLaunchKernelGGL((k_reduce_rows<double>), grid, block, 0, c->stream, (const double*)vec, 1, R, out, 0, 0ull,
                         (unsigned long long*)nullptr);
      NCCLCHK(ncclAllReduce(out, out, (size_t)R, ncclDouble, ncclSum, c->comm, c->stream));
    } else {
      if (++c->xg.seq == 0) c->xg.seq = 2;
      hipLaunchKernelGGL((k_reduce_xgmi<double, false>), xg_grid(c, R), block, 0, c->stream, (const double*)vec, 1, R, out,
                         c->xg.peers, c->xg.seq, XG_TEST_TIMEOUT_TICKS, c->xg.err, 0, (double*)nullptr,
                         (double*)nullptr, (double*)nullptr, (double*)nullptr, 0.0, 0.0, 0.0, 0.0, (double*)nullptr,
                         c->nd, (float*)nullptr);
    }
    return 0;
  };
  for (int i = 0; i < 10; ++i) if (int rc = once()) return rc;
  HIPCHK(hipStreamSynchronize(c->stream));
  const auto t0 = std::chrono::steady_clock::now();
  for (int i = 0; i < iters; ++i) if (int rc = once()) return rc;
  HIPCHK(hipStreamSynchronize(c->stream));
  *us_per_iter = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / iters;
  HIPCHK(hipGetLastError());
  if (mode == 2) {
    int e = 0;
    HIPCHK(hipMemcpy(&e, c->xg.err, sizeof(int), hipMemcpyDeviceToHost));
    if (e) { HIPCHK(hipMemset(c->xg.err, 0, sizeof(int))); return fail(PINN_ECOMM, "mailbox exchange timed out in the probe"); }
  }
  return 0;
}

int pinn_comm_set_mode(pinn_ctx* c, int mode) {
  REQUIRE(c && (mode == 1 || mode == 2), "mode must be 1 (RCCL) or 2 (mailboxes)");
  if (mode == 2) REQUIRE(c->xg.attached, "mailboxes are not attached (pinn_comm_xgmi_attach)");
  if (mode == 1) REQUIRE(c->comm, "mode 1 needs an RCCL communicator (pinn_comm_init)");
  c->xg.on = mode == 2;
  return 0;
}

int pinn_comm_get_mode(pinn_ctx* c, int* mode) {
  REQUIRE(c && mode, "null");
  *mode = c->xg.on ? 2 : c->comm ? 1 : 0;
  return 0;
}

int pinn_timing_enable(pinn_ctx* c, int max_evals, int every) {
  REQUIRE(c && max_evals >= 0 && every >= 1, "bad arguments");
  HIPCHK(hipSetDevice(c->device));
  while ((int)c->ev.size() < 4 * (max_evals > 8 ? max_evals : 8)) {
    hipEvent_t e;
    HIPCHK(hipEventCreate(&e));
    c->ev.push_back(e);
  }
  if (max_evals > 0) {
    // calibration: what an empty bracket (two records, nothing in between) reads on this stream
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int i = 0; i < 16; ++i) HIPCHK(hipEventRecord(c->ev[i], c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    double acc = 0;
    for (int i = 2; i < 16; i += 2) {             // skip the first (cold) pair
      float ms = 0;
      HIPCHK(hipEventElapsedTime(&ms, c->ev[i], c->ev[i + 1]));
      acc += ms;
    }
    c->ev_overhead_ms = acc / 7.0;
  }
  c->ev_cap_evals = max_evals; c->ev_used = 0; c->timing = max_evals > 0;
  c->ev_every = every; c->ev_seen = 0;
  return 0;
}

int pinn_timing_read(pinn_ctx* c, double* avg_ms, int* n) {
  REQUIRE(c && avg_ms && n, "null");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  double a = 0, b = 0, t = 0;
  for (int i = 0; i < c->ev_used; ++i) {
    float m01 = 0, m02 = 0, m03 = 0;
    HIPCHK(hipEventElapsedTime(&m01, c->ev[4 * i], c->ev[4 * i + 1]));
    HIPCHK(hipEventElapsedTime(&m02, c->ev[4 * i], c->ev[4 * i + 2]));
    HIPCHK(hipEventElapsedTime(&m03, c->ev[4 * i], c->ev[4 * i + 3]));
    a += m01; b += m02; t += m03;
  }
  *n = c->ev_used;
  const double k = c->ev_used ? 1.0 / c->ev_used : 0.0;
  avg_ms[0] = a * k; avg_ms[1] = b * k; avg_ms[2] = t * k; avg_ms[3] = c->ev_overhead_ms;
  avg_ms[4] = PATHS[c->path].one_launch ? 1.0 : 0.0;
  c->ev_used = 0;
  return 0;
}

int pinn_sync(pinn_ctx* c) {
  REQUIRE(c, "null");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  return xg_check(c);
}

int pinn_set_kernel_path(pinn_ctx* c, int path) {
  REQUIRE(c && (unsigned)path < (unsigned)KP_COUNT, "path must be 0 (generic), 1 (fused width-20), 2 (fused width-20, register stash), "
          "3 (wide MFMA sweeps), 4 (shape-generic MFMA sweeps), 5 / 6 (4's forward / reverse half with the generic other half), "
          "7 (fused width-20 float64, register stash), 8 (fused float64 MFMA sweep, widths 65..128, 2-4 hidden layers)");
  const KernelPath p = (KernelPath)path;
  for (const int k : {X_SA, X_PW})
    if (EXTRAS[k].present(c) && p != KP_FUSED20D)
      return fail(PINN_EUNSUPPORTED, "pinn_set_kernel_path: %s on kernel path 7 only (%s first)", EXTRAS[k].runs,
                  EXTRAS[k].remove);
  if (is_adr(c) && !adr_has_path(p))
    return fail(PINN_EUNSUPPORTED, "pinn_set_kernel_path: the adr kind (pde 5) runs on kernel paths 0 and 7 only; path %d "
                "(%s) has no variant for it", path, PATHS[p].name);
  if (is_adr2(c) && !adr_has_path(p))
    return fail(PINN_EUNSUPPORTED, "pinn_set_kernel_path: the adr2 kind (pde 10) runs on kernel paths 0 and 7 only; path %d "
                "(%s) has no variant for it", path, PATHS[p].name);
  if (is_adr_ide(c) && !adr_has_path(p))
    return fail(PINN_EUNSUPPORTED, "pinn_set_kernel_path: the adr_ide kind (pde 6) runs on kernel paths 0 and 7 only; path %d "
                "(%s) has no variant for it", path, PATHS[p].name);
  REQUIRE(PATHS[p].ok(c), "%s", PATHS[p].needs);
  c->path = p;
  c->sets_dirty = true;
  return 0;
}

int pinn_debug_stamps(pinn_ctx* c, long long* out, int64_t cap, int64_t* n_waves) {
#ifdef PINN_STAMPS
  REQUIRE(c && out && n_waves, "null");
  REQUIRE(c->path != KP_GENERIC, "stamps exist for the fused kernels only");
  HIPCHK(hipSetDevice(c->device));
  int rc = ensure_sets(c);
  if (rc) return rc;
  // (a split launch of path 7 has helper workgroups behind the rows' own: their stamps follow)
  const int n_wgs = split_plan(c) == 1 ? fused20d_split_grid(c->sd.n_pad / 64) : path_rows(c);
  const size_t n = (size_t)n_wgs * 4 * 32;
  REQUIRE((size_t)cap >= n, "stamp buffer too small: need %zu", n);
  c->stamps.reset();
  HIPCHK(c->stamps.reserve(n));
  HIPCHK(hipMemsetAsync(c->stamps, 0, n * 8, c->stream));
  rc = eval_loss_grad(c);
  hipError_t he = rc ? hipSuccess : hipMemcpyAsync(out, c->stamps, n * 8, hipMemcpyDeviceToHost, c->stream);
  if (he == hipSuccess) he = hipStreamSynchronize(c->stream);
  c->stamps.reset();                             // on every exit: the evaluations that follow take no stamps
  if (rc) return rc;
  HIPCHK(he);
  *n_waves = (int64_t)(n / 32);
  return 0;
#else
  (void)c; (void)out; (void)cap; (void)n_waves;
  return fail(PINN_EUNSUPPORTED, "built without -DPINN_STAMPS (profiling build only)");
#endif
}

int pinn_debug_coef_stamps(long long* out16) {
#ifdef PINN_STAMPS
  REQUIRE(out16, "null");
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_coef_stamps), 16 * sizeof(long long)));
  return 0;
#else
  (void)out16;
  return fail(PINN_EUNSUPPORTED, "built without -DPINN_STAMPS (profiling build only)");
#endif
}

int pinn_debug_t16_deal(int W, int* out49) {
  REQUIRE(out49 && W >= 1 && W <= 128, "width outside 1..128");
  const T16Deal d = t16_deal(W);
  for (int w = 0; w < 8; ++w) {
    out49[w] = d.f_lo[w]; out49[8 + w] = d.f_hi[w]; out49[16 + w] = d.e_lo[w]; out49[24 + w] = d.e_hi[w];
    out49[32 + w] = d.row0[w]; out49[40 + w] = d.ns[w];
  }
  out49[48] = d.edge;
  return 0;
}

int pinn_debug_t16f_stamps(long long* out512) {
#ifdef PINN_STAMPS
  REQUIRE(out512, "null");
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpyFromSymbol(out512, HIP_SYMBOL(g_t16f_stamps), 8 * 64 * sizeof(long long)));
  return 0;
#else
  (void)out512;
  return fail(PINN_EUNSUPPORTED, "built without -DPINN_STAMPS (profiling build only)");
#endif
}

int pinn_debug_live_buffers(int64_t* n, int64_t* bytes) {
  if (n) *n = devbuf::live_blocks.load();
  if (bytes) *bytes = devbuf::live_bytes.load();
  return 0;
}

int pinn_get_kernel_path(pinn_ctx* c, int* path) {
  REQUIRE(c && path, "null");
  *path = c->path;
  return 0;
}

int pinn_get_f64_split(pinn_ctx* c, int* split) {
  REQUIRE(c && split, "null");
  HIPCHK(hipSetDevice(c->device));
  if (int rc = ensure_sets(c)) return rc;
  const int sp = split_plan(c);
  if (sp < 0)
    return fail(PINN_EUNSUPPORTED, "PINN_F64_SPLIT=1: %d tiles need %d workgroups, this device has %d compute units",
                c->sd.n_pad / 64, fused20d_split_grid(c->sd.n_pad / 64), c->n_cu);
  *split = sp;
  return 0;
}

// ------------------------------------------------------------------------------------------
// self-adaptive point weights (include/pinn_hip.h pinn_sa_*; the SAW variants of k_fused20d, fused20d_api.h)
// ------------------------------------------------------------------------------------------
// the local set sizes as ensure_sets will assemble them
static void sa_counts(const pinn_ctx* c, int64_t* n_u, int64_t* n_f) {
  *n_u = (int64_t)(c->sets.Xu.size() / 2);
  *n_f = n_colloc(c);
}

int pinn_sa_set_weights(pinn_ctx* c, const double* lam_u, int64_t n_u, const double* lam_f, int64_t n_f) {
  REQUIRE(c, "null");
  if (int rc = weights_supported(c, EXTRAS[X_SA], "pinn_sa_set_weights")) return rc;
  int64_t cu, cf;
  sa_counts(c, &cu, &cf);
  REQUIRE((lam_u || n_u == 0) && (lam_f || n_f == 0), "pinn_sa_set_weights: null weight array");
  REQUIRE(n_u == cu && n_f == cf, "pinn_sa_set_weights: %lld / %lld weights for %lld data and %lld collocation points",
          (long long)n_u, (long long)n_f, (long long)cu, (long long)cf);
  for (int64_t j = 0; j < n_u; ++j) REQUIRE(std::isfinite(lam_u[j]), "pinn_sa_set_weights: lam_u[%lld] is not finite", (long long)j);
  for (int64_t i = 0; i < n_f; ++i) REQUIRE(std::isfinite(lam_f[i]), "pinn_sa_set_weights: lam_f[%lld] is not finite", (long long)i);
  HIPCHK(hipSetDevice(c->device));
  if (int rc = ensure_sets(c)) return rc;
  const LamLayout L = sa_layout(c);
  std::vector<double> h(L.doubles(), 0.0);
  for (int64_t j = 0; j < n_u; ++j) h[L.at(LAM_DATA) + 3 * j] = lam_u[j];
  for (int64_t i = 0; i < n_f; ++i) h[L.at(LAM_COL) + 3 * i] = lam_f[i];
  if (int rc = lam_upload(c, c->sa.arr, L, h)) return rc;
  c->sa.on = true;
  return 0;
}

int pinn_sa_get_weights(pinn_ctx* c, double* lam_u, int64_t n_u, double* lam_f, int64_t n_f) {
  REQUIRE(c, "null");
  REQUIRE(c->sa.on, "pinn_sa_get_weights: self-adaptive weights are off (pinn_sa_set_weights)");
  int64_t cu, cf;
  sa_counts(c, &cu, &cf);
  REQUIRE((lam_u || n_u == 0) && (lam_f || n_f == 0), "pinn_sa_get_weights: null weight array");
  REQUIRE(n_u == cu && n_f == cf, "pinn_sa_get_weights: %lld / %lld weights for %lld data and %lld collocation points",
          (long long)n_u, (long long)n_f, (long long)cu, (long long)cf);
  HIPCHK(hipSetDevice(c->device));
  if (int rc = ensure_sets(c)) return rc;
  const LamLayout L = sa_layout(c);
  if (int rc = lam_prepare(c, c->sa.arr, L)) return rc;            // a replaced set reads back as ones
  std::vector<double> h;
  if (int rc = lam_download(c, c->sa.arr, h)) return rc;
  for (int64_t j = 0; j < n_u; ++j) lam_u[j] = h[L.at(LAM_DATA) + 3 * j];
  for (int64_t i = 0; i < n_f; ++i) lam_f[i] = h[L.at(LAM_COL) + 3 * i];
  return 0;
}

int pinn_sa_adam_init(pinn_ctx* c, double lr) {
  REQUIRE(c, "null");
  if (int rc = weights_supported(c, EXTRAS[X_SA], "pinn_sa_adam_init")) return rc;
  REQUIRE(std::isfinite(lr) && lr >= 0.0, "pinn_sa_adam_init: lr %g must be finite and >= 0", lr);
  c->sa.lr = lr;
  return 0;
}

int pinn_sa_disable(pinn_ctx* c) {
  REQUIRE(c, "null");
  c->sa.on = false;
  return 0;
}

// ------------------------------------------------------------------------------------------
// per-point loss weights of the adr kind (include/pinn_hip.h pinn_pw_*; k_fused20d<PDE_ADR, ..> with SAW, fused20d_api.h)
// ------------------------------------------------------------------------------------------
// counts against the local set sizes as ensure_sets will assemble them; a NULL array is allowed with the right count
static int pw_check_counts(const pinn_ctx* c, const char* who, int64_t n_u, int64_t n_f, int64_t n_b) {
  int64_t cu, cf;
  sa_counts(c, &cu, &cf);
  const int64_t cb = (int64_t)(c->sets.Xlo.size() / 2);
  REQUIRE(n_u == cu && n_f == cf && n_b == cb,
          "%s: %lld / %lld / %lld weights for %lld data points, %lld collocation points and %lld boundary pairs", who,
          (long long)n_u, (long long)n_f, (long long)n_b, (long long)cu, (long long)cf, (long long)cb);
  return 0;
}

int pinn_pw_set(pinn_ctx* c, const double* lam_u, int64_t n_u, const double* lam_f, int64_t n_f, const double* lam_b,
                int64_t n_b) {
  REQUIRE(c, "null");
  if (int rc = weights_supported(c, EXTRAS[X_PW], "pinn_pw_set")) return rc;
  for (const int k : {X_ROBIN, X_SRC, X_KF}) {
    const Extra& x = EXTRAS[k];
    if (x.present(c)) return fail(PINN_EUNSUPPORTED, "pinn_pw_set: %s; remove %s first (%s)", x.pw_clash, x.pron, x.remove);
  }
  if (int rc = pw_check_counts(c, "pinn_pw_set", n_u, n_f, n_b)) return rc;
  for (int64_t j = 0; lam_u && j < n_u; ++j) REQUIRE(std::isfinite(lam_u[j]), "pinn_pw_set: lam_u[%lld] is not finite", (long long)j);
  for (int64_t i = 0; lam_f && i < n_f; ++i) REQUIRE(std::isfinite(lam_f[i]), "pinn_pw_set: lam_f[%lld] is not finite", (long long)i);
  for (int64_t p = 0; lam_b && p < n_b; ++p) REQUIRE(std::isfinite(lam_b[p]), "pinn_pw_set: lam_b[%lld] is not finite", (long long)p);
  HIPCHK(hipSetDevice(c->device));
  if (int rc = ensure_sets(c)) return rc;
  const LamLayout L = pw_layout(c);
  std::vector<double> h(L.doubles(), 0.0);
  // a pair's weight lives in the lo point's entry: both lanes read it, the lo lane steps it, pinn_pw_get returns it.  The hi
  // point's entry is never read; it gets the same start value on purpose, as lam_prepare's class-wide reset writes both, so
  // that a dump of the array shows no stray value
  for (int64_t p = 0; p < 2 * n_b; ++p) h[L.at(LAM_PAIRS) + 3 * p] = lam_b ? lam_b[p / 2] : 1.0;
  for (int64_t j = 0; j < n_u; ++j) h[L.at(LAM_DATA) + 3 * j] = lam_u ? lam_u[j] : 1.0;
  for (int64_t i = 0; i < n_f; ++i) h[L.at(LAM_COL) + 3 * i] = lam_f ? lam_f[i] : 1.0;
  if (int rc = lam_upload(c, c->pw.arr, L, h)) return rc;
  c->pw.on = true;
  return 0;
}

int pinn_pw_get(pinn_ctx* c, double* lam_u, int64_t n_u, double* lam_f, int64_t n_f, double* lam_b, int64_t n_b) {
  REQUIRE(c, "null");
  REQUIRE(c->pw.on, "pinn_pw_get: point weights are off (pinn_pw_set)");
  if (int rc = pw_check_counts(c, "pinn_pw_get", n_u, n_f, n_b)) return rc;
  HIPCHK(hipSetDevice(c->device));
  if (int rc = ensure_sets(c)) return rc;
  const LamLayout L = pw_layout(c);
  if (int rc = lam_prepare(c, c->pw.arr, L)) return rc;            // a replaced set reads back as ones
  std::vector<double> h;
  if (int rc = lam_download(c, c->pw.arr, h)) return rc;
  for (int64_t p = 0; lam_b && p < n_b; ++p) lam_b[p] = h[L.at(LAM_PAIRS) + 3 * (2 * p)];
  for (int64_t j = 0; lam_u && j < n_u; ++j) lam_u[j] = h[L.at(LAM_DATA) + 3 * j];
  for (int64_t i = 0; lam_f && i < n_f; ++i) lam_f[i] = h[L.at(LAM_COL) + 3 * i];
  return 0;
}

int pinn_pw_adam_init(pinn_ctx* c, double rate_u, double rate_f, double rate_b) {
  REQUIRE(c, "null");
  if (int rc = weights_supported(c, EXTRAS[X_PW], "pinn_pw_adam_init")) return rc;
  const double r[3] = {rate_u, rate_f, rate_b};
  for (int i = 0; i < 3; ++i)
    REQUIRE(std::isfinite(r[i]) && r[i] >= 0.0, "pinn_pw_adam_init: rate %d (%g) must be finite and >= 0", i, r[i]);
  for (int i = 0; i < 3; ++i) c->pw.rate[i] = r[i];
  return 0;
}

int pinn_pw_disable(pinn_ctx* c) {
  REQUIRE(c, "null");
  c->pw.on = false;
  return 0;
}

// ------------------------------------------------------------------------------------------
// ensembles: K members of one float64 Burgers net (kernel path 7) trained side by side on one point set
// ------------------------------------------------------------------------------------------
// A base context holds the point sets, the PDE parameters, the launch plan and the stream; every member is a context of
// its own (Adam moments, L-BFGS state, rings and log, status) whose weight, mirror, gradient, moment and status buffers are
// slices of the ensemble's blocks below and whose stream is the base's.  One evaluation = ONE k_fused20d<.., ENS> launch
// for all members (grid (n_wg, K)) + ONE member-batched reduction (k_reduce_rows_ens / k_reduce_adam_ens); the L-BFGS
// step kernels run per member between them, exactly as pinn_lbfgs_run issues them.  Member k is bit-identical to a solo
// context trained from the same weights: same launch plan, same row order, same per-column arithmetic.
struct pinn_ens {
  pinn_ctx* base = nullptr;
  int K = 0, P = 0, sw = 0;                    // members, parameters, weight-mirror stride (fused20d_weight_doubles(P))
  std::vector<pinn_ctx*> mem;
  // the blocks the members' buffers are views of (ens_build); ens_free keeps the order members -> blocks -> base
  DevBuf<double> theta, theta_r, gl, m, v;     // [K][P] / [K][sw] / [K][R]
  DevBuf<unsigned long long> nonfinite;        // [K]
  DevBuf<double> part;                         // [K][n_wg][R]
  DevBuf<double> loss_hist;                    // Adam: [steps][K][3]
  // per-member point sets and viscosities (pinn_ensk_*).  Off (shared mode) until the first per-member call; then `sets`
  // holds every member's sets as handed over (the adr kind: its periodic pairs too, one common n) WHILE THE BASE KEEPS
  // MEMBER 0'S, so that ensure_sets(base) still gives the SetDesc and the launch plan (every member has the same counts).
  // Hence every setter of this mode goes through the base's setter first -- a shared one with its argument, which it then
  // broadcasts; a per-member one with its [K][n][..] argument, whose head is member 0's, which it then slices.
  bool k_mode = false, k_dirty = true, k_nu_dirty = true;
  std::vector<PointSets> sets;                 // [K]
  std::vector<uint64_t> k_seeds;               // [K] device LHS seeds (the design geometry is the base's col)
  std::vector<double> k_nu;                    // [K]
  DevBuf<double> k_xs, k_ts, k_tgt, k_nud;     // [K][n_pad] x 3, [K]
  // an ensemble of the adr kind (pinn_adr_ens_create): every member has its own six coefficients in BOTH modes -- the host
  // rows [K][6] and the device table [K][ADR_ENS_ROW] k_fused20d<PDE_ADR_ENS> reads, there from creation and re-uploaded when dirty
  bool adr = false, coef_dirty = true;
  std::vector<double> coef;                    // [K][6]
  DevBuf<double> coef_d;                       // [K][ADR_ENS_ROW]
};

// The order is the point: the members first (their views of the blocks die with them), then the blocks (`delete e`, on the
// base's device with its stream idle), then the base, whose stream everything above ran on
static void ens_free(pinn_ens* e) {
  for (pinn_ctx* c : e->mem) (void)pinn_destroy(c);
  pinn_ctx* const base = e->base;
  if (base) { (void)hipSetDevice(base->device); (void)hipStreamSynchronize(base->stream); }
  delete e;
  (void)pinn_destroy(base);
}

// shared -> per-member mode: every member starts from the shared sets and viscosity
static void ens_to_k(pinn_ens* e) {
  if (e->k_mode) return;
  pinn_ctx* b = e->base;
  const size_t K = e->K;
  e->sets.assign(K, b->sets);
  e->k_seeds.assign(K, b->lhs.seed);
  e->k_nu.assign(K, b->nu);
  e->k_mode = true; e->k_dirty = true; e->k_nu_dirty = true;
}

// the device LHS of every member in one launch: member k's collocation slots <- points [first, first + count) of the
// design with seed k_seeds[k], each bit-identical to lhs_fill of a solo context with that seed
static int ens_lhs_fill(pinn_ens* e) {
  pinn_ctx* b = e->base;
  const int64_t cnt = b->col.count;
  if (cnt <= 0) return 0;
  const size_t off = (size_t)colloc_first(b->sd);             // off + cnt <= n_pad: inside member k's slice
  const uint64_t n = (uint64_t)b->col.n_design;
  const InMap<double> m(b->lb, b->ub);
  LhsSeeds sd{};
  for (int k = 0; k < e->K; ++k) { sd.lo[k] = (uint32_t)e->k_seeds[k]; sd.hi[k] = (uint32_t)(e->k_seeds[k] >> 32); }
  const dim3 grid((unsigned)((cnt + 255) / 256), (unsigned)e->K), block(256);
  hipLaunchKernelGGL(k_lhs_fill_ens, grid, block, 0, b->stream, e->k_xs + off, e->k_ts + off, (int64_t)b->sd.n_pad, cnt,
                     (uint64_t)b->col.first, n, lhs_half_bits(n), sd, m.lbx, m.lbt, m.ex, m.et);
  HIPCHK(hipGetLastError());
  return 0;
}

// ensure_sets for the ensemble: the base's SetDesc and plan, then (per-member mode) the [K][n_pad] sets, each member's slice
// by the assembler that ensure_sets calls (one output: ens_check_shape); the adr kind's coefficient table in both modes
static int ens_ensure_sets(pinn_ens* e) {
  pinn_ctx* b = e->base;
  if (b->sets_dirty) e->k_dirty = true;
  if (int rc = ensure_sets(b)) return rc;
  const size_t K = e->K;
  if (e->adr && e->coef_dirty) {               // both modes: the members' rows, padded to ADR_ENS_ROW doubles
    std::vector<double> rows(K * ADR_ENS_ROW, 0.0);
    for (size_t k = 0; k < K; ++k)
      for (int j = 0; j < 6; ++j) rows[k * ADR_ENS_ROW + j] = e->coef[k * 6 + j];
    if (upload_real(b, e->coef_d, rows.data(), rows.size())) return PINN_EHIP;
    e->coef_dirty = false;
  }
  if (!e->k_mode) return 0;
  if (!e->adr) {
    if (!e->k_nud) {
      HIPCHK(e->k_nud.reserve(K));
      e->k_nu_dirty = true;
    }
    if (e->k_nu_dirty) {
      if (upload_real(b, e->k_nud, e->k_nu.data(), K)) return PINN_EHIP;
      e->k_nu_dirty = false;
    }
  }
  if (!e->k_dirty) return 0;
  const SetDesc& sd = b->sd;
  const size_t n_pad = sd.n_pad;
  const bool lhs = b->col.from == pinn_ctx::COL_LHS;            // the members' slots are filled below
  std::vector<double> hx(K * n_pad), ht(K * n_pad), htg(K * n_pad);
  for (size_t k = 0; k < K; ++k) {
    REQUIRE(has_counts(e->sets[k], sd, 1, lhs),
            "the members' point sets do not have the base's counts (%d pairs, %d data, %d collocation points)", sd.n_b, sd.n_u,
            sd.n_f);
    assemble_set(e->sets[k], sd, 1, adr_family(b), lhs, b->lb, hx.data() + k * n_pad, ht.data() + k * n_pad,
                 htg.data() + k * n_pad);
  }
  HIPCHK(e->k_xs.reserve(K * n_pad));
  HIPCHK(e->k_ts.reserve(K * n_pad));
  HIPCHK(e->k_tgt.reserve(K * n_pad));
  if (upload_real(b, e->k_xs, hx.data(), K * n_pad) || upload_real(b, e->k_ts, ht.data(), K * n_pad) ||
      upload_real(b, e->k_tgt, htg.data(), K * n_pad)) return PINN_EHIP;
  if (lhs) { if (int rc = ens_lhs_fill(e)) return rc; }
  e->k_dirty = false;
  return 0;
}

// one evaluation of every member at its current weights.  active[k] = false: member k's rows are computed but not reduced
// (its gradient, status and evaluation count stay as they are).  alpha != nullptr: the Adam step behind the reduction,
// loss3 <- [K][3] loss parts.
static int ens_eval(pinn_ens* e, const bool* active, const double* alpha, double* loss3) {
  pinn_ctx* b = e->base;
  if (int rc = ens_ensure_sets(e)) return rc;
  const int n_rows = path_rows(b);
  const size_t need = (size_t)e->K * n_rows * b->R;
  HIPCHK(e->part.reserve(need));
  F20dLaunch a = fused20d_args(b, nullptr);
  a.th = e->theta_r; a.part = e->part; a.n_members = e->K;
  if (e->k_mode) { a.xs = e->k_xs; a.ts = e->k_ts; a.tgt = e->k_tgt; }
  const int rc = e->adr    ? fused20d_ens_launch_any(a, AdrEnsArg{e->coef_d}, e->k_mode)
                 : e->k_mode ? fused20d_ens_launch_any(b->pde, a, (const double*)e->k_nud)
                             : fused20d_ens_launch_any(b->pde, a, b->nu);
  if (rc) return fail(PINN_EHIP, "ensemble fused20d launch failed: %s", hipGetErrorString((hipError_t)rc));
  EnsStep es{};
  for (int k = 0; k < e->K; ++k) {
    if (!active[k]) continue;
    pinn_ctx* c = e->mem[k];
    c->n_evals += 1;
    es.eval_no[k] = c->n_evals;
    if (alpha) es.alpha[k] = alpha[k];
  }
  const dim3 grid((b->R + RED_COLS - 1) / RED_COLS, e->K);
  pinn_ctx* c0 = e->mem[0];
  if (alpha)
    hipLaunchKernelGGL(k_reduce_adam_ens, grid, dim3(RED_THREADS), 0, b->stream, (const double*)e->part, n_rows, b->R,
                       e->gl, e->P, e->sw, e->theta, e->theta_r, e->m, e->v, c0->adam.b1, c0->adam.b2, c0->adam.eps, loss3, e->nonfinite,
                       es);
  else
    hipLaunchKernelGGL(k_reduce_rows_ens, grid, dim3(RED_THREADS), 0, b->stream, (const double*)e->part, n_rows, b->R,
                       e->gl, e->P, e->nonfinite, es);
  HIPCHK(hipGetLastError());
  return 0;
}

// what both constructors refuse before any device work: a null argument and K outside 1..ENS_MAX (PINN_EINVAL), ...
static int ens_check_args(pinn_ens** out, const int* layers, const double* lb, const double* ub, int n_members) {
  REQUIRE(out && layers && lb && ub, "null argument");
  REQUIRE(n_members >= 1 && n_members <= ENS_MAX, "ensemble size %d outside 1..%d", n_members, ENS_MAX);
  return 0;
}
// ... and a net other than 2-20-...-20-1 with 4, 6 or 8 hidden layers (PINN_EUNSUPPORTED)
static int ens_check_shape(const int* layers, int n_layers) {
  const int H = n_layers - 2;
  bool shape_ok = n_layers >= 3 && fused20d_depth_ok(H) && layers[0] == 2 && layers[n_layers - 1] == 1;
  for (int i = 1; shape_ok && i <= H; ++i) shape_ok = layers[i] == FW;
  if (!shape_ok)
    return fail(PINN_EUNSUPPORTED, "ensembles need the 2-%d-1 net with 4, 6 or 8 hidden layers of width %d", FW, FW);
  return 0;
}

// the base, the blocks and the members of an ensemble of float64 contexts of pde_kind (the arguments are checked), into a
// fresh e.  ens_build frees whatever stands on any failure, so every return here is plain
static int ens_build_into(pinn_ens* e, const int* layers, int n_layers, const double* lb, const double* ub, int pde_kind,
                          int device) {
  const int dtype = PINN_F64;
  if (int rc = pinn_create(&e->base, layers, n_layers, lb, ub, pde_kind, dtype, device)) return rc;
  pinn_ctx* b = e->base;
  if (b->path != KP_FUSED20D) return fail(PINN_EUNSUPPORTED, "ensembles need kernel path 7 (got %d)", (int)b->path);
  e->P = b->nd.n_theta;
  e->sw = (int)fused20d_weight_doubles(e->P);
  const size_t K = e->K, P = e->P;
  if (pde_kind == PINN_PDE_ADR) {              // every row starts as a new adr context's coefficients
    e->adr = true;
    for (size_t k = 0; k < K; ++k) e->coef.insert(e->coef.end(), b->adr, b->adr + 6);
    HIPCHK(e->coef_d.reserve(K * ADR_ENS_ROW));
    e->coef_dirty = true;
  }
  HIPCHK(e->theta.reserve(K * P));
  HIPCHK(e->m.reserve(K * P));
  HIPCHK(e->v.reserve(K * P));
  HIPCHK(e->theta_r.reserve_bytes(K * e->sw * 8 + 1024));
  HIPCHK(e->gl.reserve(K * b->R));
  HIPCHK(e->nonfinite.reserve(K));
  HIPCHK(hipMemsetAsync(e->theta, 0, K * P * 8, b->stream));
  HIPCHK(hipMemsetAsync(e->theta_r, 0, K * e->sw * 8 + 1024, b->stream));
  HIPCHK(hipMemsetAsync(e->gl, 0, K * b->R * 8, b->stream));
  HIPCHK(hipMemsetAsync(e->nonfinite, 0, K * 8, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  for (size_t k = 0; k < K; ++k) {
    pinn_ctx* c = nullptr;
    if (int rc = pinn_create(&c, layers, n_layers, lb, ub, pde_kind, dtype, device)) return rc;
    e->mem.push_back(c);
    // the member's own six buffers are freed, in this order, and become views of its slices of the blocks
    c->theta.borrow(e->theta + k * P); c->theta_r.borrow(e->theta_r + k * e->sw); c->gl.borrow(e->gl + k * b->R);
    c->adam_m.borrow(e->m + k * P); c->adam_v.borrow(e->v + k * P); c->d_nonfinite.borrow(e->nonfinite + k);
    (void)hipStreamDestroy(c->stream);
    c->stream = b->stream;
    c->own_stream = false;
  }
  return 0;
}

static int ens_build(pinn_ens** out, const int* layers, int n_layers, const double* lb, const double* ub, int pde_kind,
                     int device, int n_members) {
  *out = nullptr;
  pinn_ens* e = new pinn_ens();
  e->K = n_members;
  if (int rc = ens_build_into(e, layers, n_layers, lb, ub, pde_kind, device)) { ens_free(e); return rc; }
  *out = e;
  return 0;
}

int pinn_ens_create(pinn_ens** out, const int* layers, int n_layers, const double* lb, const double* ub, int pde_kind,
                    int dtype, int device, int n_members) {
  // every refusal comes before any device work
  if (int rc = ens_check_args(out, layers, lb, ub, n_members)) return rc;
  if (dtype != PINN_F64)
    return fail(PINN_EUNSUPPORTED, "ensembles are float64 only (kernel path 7); float32 is not supported");
  if (pde_kind != PINN_PDE_BURGERS && pde_kind != PINN_PDE_BURGERS_IDE)
    return fail(PINN_EUNSUPPORTED, "ensembles support Burgers inference and identification (pde 0, 1) only; "
                                   "Schrodinger and discrete-time models are not supported");
  if (int rc = ens_check_shape(layers, n_layers)) return rc;
  return ens_build(out, layers, n_layers, lb, ub, pde_kind, device, n_members);
}

// K members of the adr kind (float64, kernel path 7): pinn_ens_create's handle, refusals and blocks; every member has its
// own six coefficients (pinn_ens_set_pde_params / pinn_adr_ensk_set_params), whether the point sets are shared or not
int pinn_adr_ens_create(pinn_ens** out, const int* layers, int n_layers, const double* lb, const double* ub, int device,
                        int n_members) {
  if (int rc = ens_check_args(out, layers, lb, ub, n_members)) return rc;
  if (int rc = ens_check_shape(layers, n_layers)) return rc;
  return ens_build(out, layers, n_layers, lb, ub, PINN_PDE_ADR, device, n_members);
}

int pinn_ens_destroy(pinn_ens* e) {
  if (e) ens_free(e);
  return 0;
}

int pinn_ens_size(pinn_ens* e, int* n_members, int64_t* n_params) {
  REQUIRE(e, "null");
  if (n_members) *n_members = e->K;
  if (n_params) *n_params = e->P;
  return 0;
}

// (per-member mode: the shared setters broadcast -- the same set or viscosity in every member's slots)
int pinn_ens_set_collocation(pinn_ens* e, const double* X_f, int64_t n, int64_t n_total) {
  REQUIRE(e, "null");
  if (int rc = pinn_set_collocation(e->base, X_f, n, n_total)) return rc;
  if (e->k_mode) { broadcast_field(e->sets, &PointSets::Xf, X_f, 2 * n); e->k_dirty = true; }
  return 0;
}

int pinn_ens_set_data(pinn_ens* e, const double* X_u, const double* u, int64_t n, int64_t n_total) {
  REQUIRE(e, "null");
  if (int rc = pinn_set_data(e->base, X_u, u, n, n_total)) return rc;
  if (e->k_mode) {
    broadcast_field(e->sets, &PointSets::Xu, X_u, 2 * n);
    broadcast_field(e->sets, &PointSets::U, u, n);
    e->k_dirty = true;
  }
  return 0;
}

int pinn_ens_set_pde_params(pinn_ens* e, const double* p, int n) {
  REQUIRE(e, "null");
  if (int rc = pinn_set_pde_params(e->base, p, n)) return rc;      // (the adr kind: n != 6 or a non-finite value is refused here)
  if (e->adr) {                                                    // one set for all members; the mode stays what it is
    for (int k = 0; k < e->K; ++k) memcpy(e->coef.data() + (size_t)k * 6, p, 6 * sizeof(double));
    e->coef_dirty = true;
    return 0;
  }
  if (e->k_mode) { e->k_nu.assign((size_t)e->K, p[0]); e->k_nu_dirty = true; }
  return 0;
}

// the adr kind: one coefficient set per member.  Nothing changes on a refusal, and the mode stays what it is
int pinn_adr_ensk_set_params(pinn_ens* e, const double* p, int n_members) {
  REQUIRE(e && p, "null argument");
  if (!e->adr) return fail(PINN_EUNSUPPORTED, "pinn_adr_ensk_set_params: this is not an ensemble of the adr kind (pinn_adr_ens_create)");
  REQUIRE(n_members == e->K, "pinn_adr_ensk_set_params: %d coefficient sets for %d members", n_members, e->K);
  for (int i = 0; i < 6 * e->K; ++i)
    REQUIRE(std::isfinite(p[i]), "pinn_adr_ensk_set_params: coefficient %d of member %d is not finite", i % 6, i / 6);
  if (int rc = pinn_set_pde_params(e->base, p, 6)) return rc;      // the base keeps member 0's
  e->coef.assign(p, p + (size_t)6 * e->K);
  e->coef_dirty = true;
  return 0;
}

int pinn_adr_ens_get_params(pinn_ens* e, double* p, int n_members) {
  REQUIRE(e && p, "null argument");
  if (!e->adr) return fail(PINN_EUNSUPPORTED, "pinn_adr_ens_get_params: this is not an ensemble of the adr kind (pinn_adr_ens_create)");
  REQUIRE(n_members == e->K, "pinn_adr_ens_get_params: room for %d coefficient sets, the ensemble has %d members", n_members, e->K);
  memcpy(p, e->coef.data(), (size_t)6 * e->K * sizeof(double));
  return 0;
}

// the adr kind's periodic pairs: one set for all members (per-member mode: the same pairs in every member's slots) ...
int pinn_adr_ens_set_boundary(pinn_ens* e, const double* X_lb, const double* X_ub, int64_t n, int64_t n_total) {
  REQUIRE(e, "null");
  if (!e->adr) return fail(PINN_EUNSUPPORTED, "pinn_adr_ens_set_boundary: boundary pairs are for ensembles of the adr kind (pinn_adr_ens_create)");
  if (int rc = pinn_set_boundary(e->base, X_lb, X_ub, n, n_total)) return rc;
  if (e->k_mode) {
    broadcast_field(e->sets, &PointSets::Xlo, X_lb, 2 * n);
    broadcast_field(e->sets, &PointSets::Xhi, X_ub, 2 * n);
    e->k_dirty = true;
  }
  return 0;
}

// per-member sets (every refusal before anything changes)
static constexpr int64_t ENSK_MAX_POINTS = (int64_t)1 << 30;

int pinn_ensk_set_collocation(pinn_ens* e, const double* X_f, int64_t n, int64_t n_total) {
  REQUIRE(e && X_f, "null argument");
  REQUIRE(n >= 0 && n <= ENSK_MAX_POINTS && n_total >= n, "bad collocation arguments (n %lld, n_total %lld)",
          (long long)n, (long long)n_total);
  REQUIRE(e->base->pde != PINN_PDE_BURGERS_IDE || n == 0,
          "identification evaluates the residual at the data points; no collocation set");
  ens_to_k(e);
  if (int rc = pinn_set_collocation(e->base, X_f, n, n_total)) return rc;
  slice_field(e->sets, &PointSets::Xf, X_f, 2 * n);
  e->k_dirty = true;
  return 0;
}

int pinn_ensk_set_data(pinn_ens* e, const double* X_u, const double* u, int64_t n, int64_t n_total) {
  REQUIRE(e && X_u && u, "null argument");
  REQUIRE(n >= 0 && n <= ENSK_MAX_POINTS && n_total >= n, "bad data arguments (n %lld, n_total %lld)", (long long)n,
          (long long)n_total);
  ens_to_k(e);
  if (int rc = pinn_set_data(e->base, X_u, u, n, n_total)) return rc;
  slice_field(e->sets, &PointSets::Xu, X_u, 2 * n);
  slice_field(e->sets, &PointSets::U, u, n);
  e->k_dirty = true;
  return 0;
}

// ... or one set per member, [K][n][2] each, one common n (CHUNK_POINTS / 4 pairs at the most, as ensure_sets asks)
int pinn_adr_ensk_set_boundary(pinn_ens* e, const double* X_lb, const double* X_ub, int64_t n, int64_t n_total) {
  REQUIRE(e && ((X_lb && X_ub) || n == 0), "null argument");
  if (!e->adr) return fail(PINN_EUNSUPPORTED, "pinn_adr_ensk_set_boundary: boundary pairs are for ensembles of the adr kind (pinn_adr_ens_create)");
  REQUIRE(n >= 0 && 2 * n <= CHUNK_POINTS / 2 && n_total >= n, "bad boundary arguments (n %lld, n_total %lld)", (long long)n,
          (long long)n_total);
  ens_to_k(e);
  if (int rc = pinn_set_boundary(e->base, X_lb, X_ub, n, n_total)) return rc;
  slice_field(e->sets, &PointSets::Xlo, X_lb, 2 * n);
  slice_field(e->sets, &PointSets::Xhi, X_ub, 2 * n);
  e->k_dirty = true;
  return 0;
}

int pinn_ensk_set_pde_params(pinn_ens* e, const double* nu, int n_members) {
  REQUIRE(e && nu, "null argument");
  if (e->adr) return fail(PINN_EUNSUPPORTED, "pinn_ensk_set_pde_params: a viscosity per member is the Burgers ensemble's call; "
                                             "an adr ensemble takes six coefficients per member (pinn_adr_ensk_set_params)");
  REQUIRE(n_members == e->K, "%d viscosities for %d members", n_members, e->K);
  ens_to_k(e);
  if (int rc = pinn_set_pde_params(e->base, nu, 1)) return rc;      // (identification: accepted and unused, as solo)
  e->k_nu.assign(nu, nu + e->K);
  e->k_nu_dirty = true;
  return 0;
}

int pinn_ensk_lhs_collocation(pinn_ens* e, int64_t n_design, int64_t first, int64_t count, const uint64_t* seeds) {
  REQUIRE(e && seeds, "null argument");
  pinn_ctx* b = e->base;
  REQUIRE(b->pde != PINN_PDE_BURGERS_IDE, "pinn_ensk_lhs_collocation: this model has no collocation set");
  if (int rc = design_check(n_design, first, count)) return rc;
  HIPCHK(hipSetDevice(b->device));
  // re-draw in place (one launch, nothing rebuilt) when only the seeds change, as pinn_lhs_collocation does
  const bool in_place = e->k_mode && !e->k_dirty && !b->sets_dirty && b->col.from == pinn_ctx::COL_LHS &&
                        b->col.count == count;
  ens_to_k(e);
  if (int rc = pinn_lhs_collocation(b, n_design, first, count, seeds[0])) return rc;
  e->k_seeds.assign(seeds, seeds + e->K);
  for (PointSets& ps : e->sets) ps.Xf.clear();
  if (in_place && !b->sets_dirty) return ens_lhs_fill(e);
  e->k_dirty = true;
  return 0;
}

int pinn_ens_set_weights(pinn_ens* e, const double* w, int64_t n) {
  REQUIRE(e && w, "null");
  REQUIRE(n == (int64_t)e->K * e->P, "weight array has %lld entries, expected K x P = %d x %d", (long long)n, e->K, e->P);
  pinn_ctx* b = e->base;
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipMemcpyAsync(e->theta, w, (size_t)n * 8, hipMemcpyHostToDevice, b->stream));
  for (pinn_ctx* c : e->mem) if (int rc = cast_weights(c)) return rc;
  HIPCHK(hipStreamSynchronize(b->stream));
  return 0;
}

int pinn_ens_get_weights(pinn_ens* e, double* w, int64_t n) {
  REQUIRE(e && w, "null");
  REQUIRE(n == (int64_t)e->K * e->P, "weight array has %lld entries, expected K x P = %d x %d", (long long)n, e->K, e->P);
  pinn_ctx* b = e->base;
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipMemcpyAsync(w, e->theta, (size_t)n * 8, hipMemcpyDeviceToHost, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  return 0;
}

int pinn_ens_loss_grad(pinn_ens* e, double* losses, double* grads, double* terms) {
  REQUIRE(e, "null");
  pinn_ctx* b = e->base;
  HIPCHK(hipSetDevice(b->device));
  std::vector<char> all((size_t)e->K, 1);
  if (int rc = ens_eval(e, (const bool*)all.data(), nullptr, nullptr)) return rc;
  const int R = b->R, P = e->P;
  std::vector<double> h((size_t)e->K * R);
  HIPCHK(hipMemcpyAsync(h.data(), e->gl, h.size() * 8, hipMemcpyDeviceToHost, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  for (int k = 0; k < e->K; ++k) {
    const double* g = h.data() + (size_t)k * R;
    if (losses) losses[k] = g[P] + g[P + 1] + g[P + 2];
    if (terms) { terms[3 * k] = g[P]; terms[3 * k + 1] = g[P + 1]; terms[3 * k + 2] = g[P + 2]; }
    if (grads) memcpy(grads + (size_t)k * P, g, (size_t)P * 8);
  }
  return 0;
}

int pinn_ens_adam_init(pinn_ens* e, double lr, double beta1, double beta2, double eps, const double* lr_k) {
  REQUIRE(e, "null");
  for (int k = 0; k < e->K; ++k)
    if (int rc = pinn_adam_init(e->mem[k], lr_k ? lr_k[k] : lr, beta1, beta2, eps)) return rc;
  return 0;
}

int pinn_ens_adam_run(pinn_ens* e, int n_steps, double* losses) {
  REQUIRE(e && n_steps >= 0, "bad arguments");
  for (pinn_ctx* c : e->mem) REQUIRE(c->adam.ready, "pinn_ens_adam_init has not been called");
  pinn_ctx* b = e->base;
  HIPCHK(hipSetDevice(b->device));
  if (n_steps == 0) return 0;
  const size_t K = e->K;
  HIPCHK(e->loss_hist.reserve((size_t)n_steps * K * 3));
  std::vector<char> all(K, 1);
  std::vector<double> alpha(K);
  for (int s = 0; s < n_steps; ++s) {
    for (size_t k = 0; k < K; ++k)               // the step size from where adam_issue takes it
      alpha[k] = adam_step_factors(e->mem[k]).alpha(e->mem[k]->adam.lr);
    if (int rc = ens_eval(e, (const bool*)all.data(), alpha.data(), e->loss_hist + (size_t)s * K * 3)) return rc;
  }
  std::vector<double> h((size_t)n_steps * K * 3);
  HIPCHK(hipMemcpyAsync(h.data(), e->loss_hist, h.size() * 8, hipMemcpyDeviceToHost, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  if (losses)
    for (size_t i = 0; i < (size_t)n_steps * K; ++i) losses[i] = h[3 * i] + h[3 * i + 1] + h[3 * i + 2];
  return 0;
}

int pinn_ens_lbfgs_begin(pinn_ens* e, int n_corr, double tol_fun, double tol_x, double max_eval, double lr,
                         const double* lr_k, int max_iter, const int* max_iter_k) {
  REQUIRE(e, "null");
  REQUIRE(n_corr >= 1, "bad L-BFGS arguments");
  for (int k = 0; k < e->K; ++k) {
    REQUIRE((lr_k ? lr_k[k] : lr) > 0 && (max_iter_k ? max_iter_k[k] : max_iter) >= 0,
            "bad L-BFGS arguments for member %d", k);
  }
  HIPCHK(hipSetDevice(e->base->device));
  std::vector<char> ev((size_t)e->K, 0);
  bool any = false;
  for (int k = 0; k < e->K; ++k) {
    bool eval = false;
    if (int rc = lbfgs_begin_setup(e->mem[k], max_iter_k ? max_iter_k[k] : max_iter, lr_k ? lr_k[k] : lr, n_corr,
                                   tol_fun, tol_x, max_eval, &eval)) return rc;
    ev[k] = eval;
    any = any || eval;
  }
  if (!any) return 0;
  if (int rc = ens_eval(e, (const bool*)ev.data(), nullptr, nullptr)) return rc;     // custom_lbfgs.py:65
  for (int k = 0; k < e->K; ++k)
    if (ev[k]) { if (int rc = lbfgs_begin_post(e->mem[k])) return rc; }
  return 0;
}

int pinn_ens_lbfgs_run(pinn_ens* e, int n_iters, int* iters, double* losses, int* n_logged, int* done) {
  REQUIRE(e && n_iters >= 0, "bad arguments");
  for (pinn_ctx* c : e->mem) {
    REQUIRE(c->lbfgs.ready, "pinn_ens_lbfgs_begin has not been called");
    REQUIRE(c->tk.outstanding() == 0, "chunks in flight");
  }
  HIPCHK(hipSetDevice(e->base->device));
  const Range rg("pinn_ens_lbfgs_run");
  const int K = e->K;
  std::vector<LbfgsMember> m(K);
  for (int k = 0; k < K; ++k) m[k].c = e->mem[k];
  std::vector<char> act(K, 0);
  if (int rc = lbfgs_chunk(m.data(), act.data(), K, n_iters,       // pinn_lbfgs_run's chunk, one evaluation for all members
                           [e](const char* a) { return ens_eval(e, (const bool*)a, nullptr, nullptr); })) return rc;
  const int ld = n_iters + 1;                  // the rows of iters / losses (the ABI's); n_iters entries suffice, as solo
  for (int k = 0; k < K; ++k) {
    int nl = 0, dn = 0;
    if (int rc = pinn_lbfgs_collect(m[k].c, m[k].ticket, n_iters, iters ? iters + (size_t)k * ld : nullptr,
                               losses ? losses + (size_t)k * ld : nullptr, &nl, &dn)) return rc;
    if (n_logged) n_logged[k] = nl;
    if (done) done[k] = dn;
  }
  return 0;
}

int pinn_ens_predict(pinn_ens* e, const double* X, int64_t n, double* out) {
  REQUIRE(e && X && out && n >= 0, "bad arguments");
  for (int k = 0; k < e->K; ++k)
    if (int rc = pinn_predict(e->mem[k], X, n, out + (size_t)k * n)) return rc;
  return 0;
}

int pinn_ens_error_l2(pinn_ens* e, const double* X, const double* ref, int64_t n, double* err) {
  REQUIRE(e && X && ref && err && n > 0, "bad arguments");
  for (int k = 0; k < e->K; ++k)
    if (int rc = pinn_error_l2(e->mem[k], X, ref, n, 0, err + k)) return rc;
  return 0;
}

int pinn_ens_get_status(pinn_ens* e, int64_t* n_evals, int64_t* first_nonfinite_eval) {
  REQUIRE(e, "null");
  for (int k = 0; k < e->K; ++k) {
    int64_t a = 0, b = 0;
    if (int rc = pinn_get_status(e->mem[k], &a, &b)) return rc;
    if (n_evals) n_evals[k] = a;
    if (first_nonfinite_eval) first_nonfinite_eval[k] = b;
  }
  return 0;
}

}  // extern "C"
