// fused20d_api.h -- host-side interface of the float64 register-stash kernel (kernels_fused20d.h).  The kernel lives in
// its own translation unit (fused20d_unit.hip) because it is compiled with -mllvm -amdgpu-mfma-vgpr-form=1: with 240
// AGPRs taken by the stash, hipcc's default (matrix results in AGPRs) costs two v_accvgpr_read per result, 1 900 of
// them per tile; the flag keeps the results in VGPRs.  The other kernels keep the default allocation they were tuned
// with.
#pragma once
#include <hip/hip_runtime.h>
#include "kernels_generic.h"

namespace pinn {

// 16-value gradient blocks of one wave: dense 0 (5), hidden layers 1..H-1 (30 each), dense H (6)
constexpr int fused20d_blocks(int H) { return 5 + (H - 1) * 30 + 6; }
// the flat weight vector is brought into LDS by LDS-DMA in whole 1-KiB pieces (128 doubles)
inline size_t fused20d_weight_doubles(int n_theta) { return ((size_t)n_theta + 127) / 128 * 128; }
// one-tile launches (workgroups >= tiles) keep no accumulators: every wave parks the blocks of one phase of the reverse sweep
// (<= 30) in a staging area, double buffered, and the workgroup sums them phase by phase.  PINN_ONETILE_SUM
// (kernels_fused20d.h) -- 0, the default: unfolded, all 64 lanes; 1: the blocks folded in registers, 16 totals per block and
// wave; 2: folded, no double buffer -- every block of the sweep has a place of its own, summed once behind the sweep
#ifndef PINN_ONETILE_SUM
#define PINN_ONETILE_SUM 0
#endif
constexpr int FUSED20D_STAGE_WAVE = PINN_ONETILE_SUM ? 30 * 16 : 30 * 64;   // doubles per wave and buffer
constexpr int FUSED20D_STAGE_BUF = 4 * FUSED20D_STAGE_WAVE;     // doubles per buffer (four waves)
constexpr int fused20d_stage_doubles(int n_hidden) {
  return PINN_ONETILE_SUM == 2 ? fused20d_blocks(n_hidden) * 64 : 2 * FUSED20D_STAGE_BUF;
}
inline size_t fused20d_lds_bytes(int n_hidden, int n_theta) {
  const size_t acc = (size_t)4 * fused20d_blocks(n_hidden) * 16, stage = (size_t)fused20d_stage_doubles(n_hidden);
  return (fused20d_weight_doubles(n_theta) + (acc > stage ? acc : stage) + 4 * 256) * sizeof(double);   // + loss-part slots
}

// entry e = 16 * block + 4 * i + j of a wave's block list -> flat parameter index (reference layout), -1 = padding;
// out holds fused20d_blocks(H) x 16 ints
void fused20d_row_index(const NetDesc& nd, int H, int* out);

inline bool fused20d_depth_ok(int n_hidden) { return n_hidden == 4 || n_hidden == 6 || n_hidden == 8; }

// The split one-tile launch (k_split20d, kernels_fused20d_kernel.h): beside the main workgroup of every tile, helper
// workgroups on compute units the launch would leave idle recompute a tile's forward sweep and seeds -- same inputs, same
// instructions, same bits -- and write the weight-gradient columns of the top of the reverse sweep into the tile's gradient
// row; the main workgroup leaves those blocks out.  A helper serves two tiles, one after the other.  No workgroup waits for
// another or reads what another wrote: rows, reduction and every bit downstream are those of the plain launch.
// Who writes column idx of a gradient row of n_theta + F20D_LOSS_SLOTS doubles: the helper owns the last hidden layer's
// kernel and bias and the output layer's, one contiguous range; the main workgroup owns the layers below, the equation's
// trailing parameters and the loss parts.  Both roles take their store predicates from here (PINN_ROLE_OWNS).
enum { F20D_MAIN = 0, F20D_HELPER = 1 };
constexpr int F20D_LOSS_SLOTS = 4;
constexpr int F20D_WIDTH = 20;         // == FW (kernels_fused20.h, checked in kernels_fused20d.h)
constexpr int f20d_layer_first(int d) { return d == 0 ? 0 : 3 * F20D_WIDTH + (d - 1) * (F20D_WIDTH + 1) * F20D_WIDTH; }   // layer d's kernel
constexpr int f20d_n_net(int H) { return f20d_layer_first(H) + F20D_WIDTH + 1; }
constexpr int f20d_split_owner(int idx, int H, int n_tail) {
  (void)n_tail;                        // (the trailing parameters stand behind the net: the main role's, like the loss parts)
  return idx >= f20d_layer_first(H - 1) && idx < f20d_n_net(H) ? F20D_HELPER : F20D_MAIN;
}
// every column has one owner (the function is total), the helper's columns are exactly layers H - 1 and H, and neither set
// is empty: what k_split20d static_asserts for every (PDE, H) it is instantiated with
constexpr bool f20d_split_ok(int H, int n_tail) {
  const int n = f20d_n_net(H) + n_tail + F20D_LOSS_SLOTS;
  int n_main = 0, n_helper = 0;
  for (int i = 0; i < n; ++i) {
    const int o = f20d_split_owner(i, H, n_tail);
    if (o != F20D_MAIN && o != F20D_HELPER) return false;
    const bool top = i >= f20d_layer_first(H - 1) && i < f20d_n_net(H);
    if ((o == F20D_HELPER) != top) return false;
    (o == F20D_HELPER ? n_helper : n_main) += 1;
  }
  return H >= 3 && n_main + n_helper == n && n_helper == (F20D_WIDTH + 1) * F20D_WIDTH + F20D_WIDTH + 1 && n_main > 0;
}
// workgroups of a split launch over n_tiles tiles: one main workgroup per tile, one helper per pair of tiles
constexpr int fused20d_split_grid(int n_tiles) { return n_tiles + (n_tiles + 1) / 2; }
// whether this build holds k_split20d (the folded phase sums of -DPINN_ONETILE_SUM=1, 2 are profiling builds without it)
constexpr bool fused20d_split_built() { return PINN_ONETILE_SUM == 0; }
// Launch plan of path 7: 64-point tiles, persistent over n_wg = min(tiles, CUs) workgroups = partial gradient rows.

// what every launch of k_fused20d takes besides its coefficient argument
struct F20dLaunch {
  const NetDesc& nd;
  const SetDesc& sd;
  const double* th;              // n_members weight vectors, fused20d_weight_doubles(n_theta) apart
  const double *xs, *ts, *tgt;   // the point set ([n_members][sd.n_pad] where every member has its own)
  double lbx, lbt, sx, st;       // the affine map of the inputs to [-1, 1]
  double* part;                  // member m's n_wg gradient rows of R doubles at part + m * n_wg * R
  int R, n_wg, n_members;        // n_members: 1 = solo
  const int* row_index;          // fused20d_row_index
  hipStream_t stream;
  long long* stamps;             // -DPINN_STAMPS builds: the waves' clock stamps (nullptr: none)
  hipEvent_t ev_start, ev_stop;  // both set: attached to the launch itself
  bool split = false;            // the split one-tile plan (pde 0 and 1, solo, n_wg >= tiles, fused20d_split_built() only)
};

// one loss+gradient evaluation, 4, 6 or 8 hidden layers; every entry point returns a hipError_t.  All of them launch the
// one kernel name, k_fused20d, with the template arguments of their variant (kernels_fused20d_kernel.h)
// pde 0: Burgers inference, 1: identification
int fused20d_launch_any(int pde, const F20dLaunch& a, double nu);

// the same for n_members weight vectors (an ensemble sharing the point set): each member's rows bit-identical to a solo
// launch's
int fused20d_ens_launch_any(int pde, const F20dLaunch& a, double nu);

// the same with a point set per member, all of one SetDesc, and nu_k [n_members] in device memory: member m's rows
// bit-identical to a solo launch on member m's set with viscosity nu_k[m]
int fused20d_ens_launch_any(int pde, const F20dLaunch& a, const double* nu_k);

// Self-adaptive point weights (k_fused20d<0, H, ., false, false, true>).  lam holds SA_CONST doubles (beta1, beta2, eps of
// the ascent), then (lambda, m, v) of every point of the assembled set, [n_all][3]: the data points, then the collocation
// points, each in the order they were handed over.  alpha = lr_lambda sqrt(1 - b2^t) / (1 - b1^t) as the host forms
// Adam's step size; 0 = the weights are only read (loss_grad, L-BFGS, lr_lambda = 0), otherwise one ascent step is
// written back.  (Three values and one interleaved array: with eight arguments, or per-class arrays, the tile-loop
// variants spilled SGPRs.)
constexpr int SA_CONST = 4;
struct SaArgs {
  double nu;
  double* lam;
  double alpha;
};

// one weighted evaluation of pde 0
int fused20d_launch_any(const F20dLaunch& a, const SaArgs& sa);

// one evaluation of the advection-diffusion-reaction kind (k_fused20d<PDE_ADR, H, .>): six run-time coefficients, boundary
// block pair-interleaved
int fused20d_launch_any(const F20dLaunch& a, const AdrCoef<double>& k);

// one evaluation of the same kind with trainable coefficients (k_fused20d<PDE_ADR_IDE, H, .>): the coefficients are the six
// entries behind the net's scalars in th, k.mask says which of their gradient entries are written (the others are 0.0)
int fused20d_launch_any(const F20dLaunch& a, const AdrIdeArg& k);

// Per-point loss weights of the adr kind (k_fused20d<PDE_ADR, H, ., false, false, true>, pinn_pw_*).  lam holds PW_CONST
// doubles -- beta1, beta2, eps of the ascent, then the ascent rate by point class at 3 + class (CLS_BLO: the pairs' rate,
// CLS_BHI: 0, CLS_DATA, CLS_COL, CLS_PAD: 0), so a lane picks its rate without a branch -- then (lambda, m, v) by POINT INDEX of
// the assembled set, [2 n_b pair-interleaved | n_u | n_f][3]: pair p's one entry stands at its lo point, 2 p (the entry at
// 2 p + 1 is unused).  bc = sqrt(1 - b2^t) / (1 - b1^t) of an Adam step, by value, so a queued step needs no copy; 0 = the
// weights are only read (loss_grad, L-BFGS, all rates 0).
constexpr int PW_CONST = 8;
struct AdrPwArgs {
  AdrCoef<double> k;
  double* lam;
  double bc;
};
int fused20d_launch_any(const F20dLaunch& a, const AdrPwArgs& k);

// one evaluation of the adr kind with Robin points (k_fused20d<PDE_ADR_ROBIN, H, .>, kernels_generic.h AdrRobinArg): the set
// is [pairs | data | collocation | robin | pad], a.sd counts the first three classes and a.sd.n_pad covers all four; k.ab is a
// device array of 2 k.n doubles, 16-byte aligned; g_j stands in tgt at the Robin point's own index.  Launch only with k.n > 0.
int fused20d_launch_any(const F20dLaunch& a, const AdrRobinArg<double>& k);

// one evaluation of the adr kind with a source term (k_fused20d<PDE_ADR_SRC, H, .>, kernels_generic.h AdrSrcArg): the same set,
// s_i in a.tgt at the collocation point's own index; the Robin part of k is as above, k.n may be 0 (k.ab is not read then);
// k.src is not read by this kernel.  Launch only while a source is present.
int fused20d_launch_any(const F20dLaunch& a, const AdrSrcArg<double>& k);

// one evaluation of the adr kind with per-point coefficient fields (k_fused20d<PDE_ADR_VAR, H, .>, kernels_generic.h
// AdrVarArg): the same set; k.kf is the table of a.sd.n_f rows of six doubles, 16-byte aligned, row i for collocation point
// 2 n_b + n_u + i; the collocation slots of a.tgt hold s_i or zeros; the Robin part of k is as above, k.n may be 0; k.k and
// k.src are not read by this kernel.  Launch only while fields are present.
int fused20d_launch_any(const F20dLaunch& a, const AdrVarArg<double>& k);
// one evaluation of the adr2 kind (k_adr2_20d<PDE_ADR2, H, .>, adr2_20d_unit.hip: the kernel text under a name and in a code
// object of its own; kernels_generic.h Adr2Arg): PDE_ADR_SRC's set -- the wall block's rows are (alpha, beta, gamma, 0), both
// counts may be 0 -- and launch plan
int adr2_20d_launch_any(const F20dLaunch& a, const Adr2Arg<double>& k);

// one evaluation of a.n_members members of the adr kind (k_fused20d<PDE_ADR_ENS, H, ., true, sets>, kernels_generic.h
// AdrEnsArg): k.coef is a device table of a.n_members rows of ADR_ENS_ROW doubles (a0, a1, nu, r1, r2, r3, two pads), member
// m reads row m; sets = false: one point set for all, true: [n_members][sd.n_pad], every slice pair-interleaved as a solo
// set.  Member m's rows are bit-identical to a solo PDE_ADR launch with row m's coefficients on member m's set.
int fused20d_ens_launch_any(const F20dLaunch& a, const AdrEnsArg& k, bool sets);

}  // namespace pinn
