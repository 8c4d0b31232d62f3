// kernels_fused20d.h -- float64 loss+gradient kernel for width-20 tanh MLPs (k_fused20d): the reference's own
// arithmetic (utils/neuralnetwork.py:24-26 is float64) with every contraction on v_mfma_f64_4x4x4_4b_f64 and no
// inter-wave exchange at all.
//
// Why this shape.  Measured on gfx950 (profiles/r02_ubench_mfma_f64_4x4x4.txt): the instruction retires 4 blocks x
// (4x4x4) = 256 MACs in 16.3 cycles = the FP64 rate of the SIMD (a v_fma_f64 costs 4-5 cycles for 64 MACs; the two
// share the pipe, their times add), dependent-accumulator latency 20 cycles, and its lane maps are
//     A[i][k] : lane 16k + 4b + i      B[k][j] : lane 16k + 4b + j      D[i][j] : lane 16i + 4b + j     (b = block)
// i.e. D and B have the SAME map with the output row i in the place of the contraction index k.  Put a point on the
// low four lane bits (q = 4b + j: 16 points per wave) and a feature slot s on the two high bits, five registers per
// Taylor channel for the five groups of four features (feature = 4n + s), and a layer is
//     out_c[n] += W-pattern[m][n] (A)  x  in_c[m] (B)            25 instructions per channel, 20 = 5 x 4: no padding
// whose result registers ARE the next layer's B operands: lane = (slot, point) in, lane = (slot, point) out, for the
// forward GEMV and (with the transposed pattern) for the reverse GEMV.  No LDS exchange tile and no
// cross-lane traffic in either sweep; tanh and the Taylor / adjoint algebra are lane-local.  The weight patterns
// are plain ds_read_b64 of the flat weight vector (copied into LDS once per workgroup): lane (s, i = lane & 3) reads
// W[4m+s][4n+i] (forward) or W[4m+i][4n+s] (reverse) -- conflict-free, no packed image needed.
//
// The weight gradient dW_d[k][j] = sum over (point, channel) IN_c[k] ZBAR_c[j] contracts over POINTS, so both
// operands need point bits where the instruction contracts (lane bits 4-5) and the feature slot on bits 0-1.  Since
// round 6 that move is ONE matrix instruction with the 4 x 4 identity as B -- it swaps the slot field with the two LOW
// point bits (PINN_TO_POINTS below; rounds 2-5: a ds_bpermute pair per value, 642 per tile on the LDS pipe), 40 values
// per layer.  The four blocks then hold partial sums over the points with the same HIGH point bits.
//   tile loop (more tiles than workgroups): the blocks are folded with a DPP row rotation and added (ds_add_f64) into a per-wave
//     accumulator in LDS (221 blocks x 16 values = 28 KB per wave, persistent over the workgroup's tiles; summed over the
//     four waves in fixed order at the end);
//   one tile per workgroup: nothing is accumulated -- every lane parks its partial in a double-buffered staging area and
//     the whole workgroup adds the 4 waves x 4 blocks of every entry once per reverse layer, straight into the gradient row.
// Either way one gradient row per workgroup, no atomics, bit-reproducible.  First and last dense layer run through the
// same block machinery (in-group (h_x, h_t, 1) / single output column), so there is no per-lane gradient bookkeeping.
//
// Stash: (a, z_x, z_t, z_xx) of the 5 own features x 6 middle layers = 240 registers parked in AGPRs; layer 0 keeps
// only a (its other channels are weight constants), the last hidden layer stays live in VGPRs.  One wave per SIMD,
// four waves = 64 points per workgroup, persistent over tiles (grid = min(tiles, CUs)).
//
// Work per 64-point tile and hidden layer: 100 (forward) + 100 (reverse GEMV) + 105 (dW) + 40 (operand moves) matrix
// instructions per wave = 5.6k cycles of matrix pipe (305 of them algorithmic); algorithmic FLOP and bytes as k_fused20m (68 640 FLOP and 16 B per collocation point).
//
// Math: SURVEY.md Appendix A.1-A.3 == nested GradientTapes of 1d-burgers/inf_cont_burgers.py:65-90 under the outer
// tape of utils/neuralnetwork.py:55-59; identification (PDE == 1): 1d-burgers/ide_cont_burgers.py:56-91.
#pragma once
#include <hip/hip_ext.h>
#include <type_traits>
#include "kernels_fused20.h"
#include "fused20d_api.h"

#ifndef PINN_FOLD_STAGES
#define PINN_FOLD_STAGES 1       // tile loop: DPP fold stages in front of the ds_add_f64.  1 = the blocks are folded once (b with
                                 // b ^ 2) and the lanes of blocks 0 and 1 add into the accumulator -- two lanes per address in one
                                 // LDS instruction (resolved in lane order: run-to-run bit equality is asserted by the tile-loop
                                 // tests).  2 = folded twice, the lanes of block 0 add: one adder per address, deterministic by
                                 // construction.  Same box, N_f = 10^6: 2 stages 1778 us, 1 stage 1738 us
                                 // (profiles/r06_ab_foldstages.txt)
#endif
#ifndef PINN_GACC_ATOMIC
#define PINN_GACC_ATOMIC 1       // tile loop: gradient accumulators updated by ds_add_f64 (0: read-add-write, the old value fetched by
                                 // grad_fetch ahead of the matrix instructions; profiles/r06_ab_gacc_atomic.txt).  Settled, and
                                 // kept whole all the same: without the `old` values handed to grad_store (zeros in this
                                 // setting) six one-tile kernels of the -DPINN_ONETILE_SUM=2 build, which a test compares bit
                                 // for bit, come out with another schedule (profiles/retire_switches_device_code.txt)
#endif
static_assert(PINN_FOLD_STAGES == 1 || PINN_FOLD_STAGES == 2, "PINN_FOLD_STAGES: 1 (product) or 2; the unfolded form is retired");
// Tried and dropped (one line each; the arms were in the sources up to 7a77e26, profiles/retire_switches_device_code.txt):
//   GEMV loops left to hipcc's placement (it sinks every ds_read next to its consumer) instead of pinned step by step with
//     the weight patterns requested two steps ahead: round 4 40.8 -> 40.5 us per Adam step at N_f = 10^4 for the pinned form;
//     in the tile-loop variants N_f = 10^6 1868 -> 1851 us since round 6 (profiles/r06_ab_loopvariants.txt; with the
//     ds_bpermute moves of rounds 2-5 it was a 1.6 % loss there)
//   a reverse layer's 40 operand moves and the whole one-tile phase sum in front of the GEMV (36.9 us), or the moves inside
//     the GEMV with barrier + reads in front of it and the adds behind it (35.6 us), against the order below (35.0 us)
//     (profiles/r06_ab_onetile_v3, _v4)
//   tile loop: no DPP fold in front of the ds_add_f64 (four lanes per address): 2110 us against 1738
//     (profiles/r06_ab_foldstages.txt)
//   the operand move as a ds_bpermute pair instead of the identity-B matrix instruction (rounds 2-5; profiles/r06_ab_rotmfma.txt)
//   the tile loop re-reading the lane index through an opaque asm once per tile (what stopped the address hoisting of
//     k_wide_bwd / k_t16_fused): 256 VGPRs + 6-11 AGPR spill slots -> 238-242 / 0 and 1 % SLOWER (same-box A/B, N_f = 10^6:
//     1991 / 2000 vs 1971 / 1978 us per Adam step, profiles/r04_opaque_lane_ab.txt)
//   the four waves of a workgroup started w x 640 cycles apart (s_sleep), so that they do not meet at the LDS pipe: with the
//     per-phase barriers 36.6 -> 37.0 us (profiles/r06_ab_stagger.txt)
// PINN_ONETILE_SUM (defined in fused20d_api.h: it sizes the staging area): how a one-tile launch adds the four blocks and the
// four waves of a gradient entry
//  0  (default) every lane parks its unfolded partial, 30 x 64 doubles per wave and phase; the workgroup adds 4 waves x 4
//     blocks per entry once per reverse layer, 16 ds_read_b128 per thread
//  1  the four blocks folded in registers first (two DPP row rotations), the 16 lanes that hold the total park it, entry-major
//     with the four waves adjacent: a quarter of the LDS bytes, 4 ds_read_b128 per thread and layer
//  2  the fold of 1, every phase in a region of its own, no per-layer barrier: one sum behind the sweep
// All three form (b0 + b1) + (b2 + b3) per wave and ((w0 + w1) + w2) + w3 over the waves: bit-identical rows
// (tests/test_gpu_onetile_fold.py builds 1 and 2 and compares).  Both folds LOST: + 1.8 and + 1.5 us per step on the headline
// (profiles/onetile_fold_ab.txt section 1) -- the 1 050 instructions they add cost more than the LDS traffic they save.
#ifndef PINN_ROW_STORE_WT
#define PINN_ROW_STORE_WT 1      // the one-tile row stores as write-through stores (agent-scope relaxed atomic store: sc1), spread
                                 // over the reverse sweep: the launch does not end with the rows dirty in the L2s, which the
                                 // reduction behind it otherwise waits for.  Same values; measured against the parent's plain
                                 // stores in profiles/onetile_fold_ab.txt section 2.  0: plain stores
#endif

// finer timeline inside reverse layer 4 and forward layer 4 (slots 20..30 of the wave's 32), profiling build -DPINN_STAMPS2 only
#if defined(PINN_STAMPS) && defined(PINN_STAMPS2)
#define STAMP2(cond, i) do { if (cond) STAMP(i); } while (0)
#else
#define STAMP2(cond, i) do { } while (0)
#endif

namespace pinn {

// (Ablation builds -- one ingredient compiled out at a time, wrong results by construction, only times are read -- are not part
// of the product sources since round 5.  profiles/ablation_scaffolding.patch holds the -DPINN_ABL / -DPINN_ABLD / -DT16_ABL
// switches of profiles/ablate_*.py; it is not kept up with these sources: it reverse-applies to the tree at ee3788e; check that
// commit out for the ablation builds.  Their results are under profiles/*ablate*.txt.)

// a double parked in the accumulation half of the register file (two 32-bit AGPRs)
struct agd { int lo, hi; };
__device__ __forceinline__ agd agd_put(const double x) {
  agd a;
  const int lo = __double2loint(x), hi = __double2hiint(x);
  asm("v_accvgpr_write_b32 %0, %1" : "=a"(a.lo) : "v"(lo));
  asm("v_accvgpr_write_b32 %0, %1" : "=a"(a.hi) : "v"(hi));
  return a;
}
// The same for a value that comes straight out of a matrix instruction.  hipcc's hazard recogniser does not look
// inside inline asm, so nothing would keep the v_accvgpr_write the required wait states behind the MFMA that
// produces x (observed: stale low words, 1e-8 relative errors).  `after` must be the result of a compiler-visible
// VALU instruction that reads x: the extra operand orders the asm behind that instruction, whose own hazard wait
// the compiler did insert.  tests/helpers/isa_lint.py checks the built code for exactly this (every accvgpr move of
// the library against every matrix instruction in front of it, along the control-flow graph).
__device__ __forceinline__ agd agd_put_after(const double x, const double after) {
  agd a;
  const int lo = __double2loint(x), hi = __double2hiint(x), dep = __double2hiint(after);
  asm("v_accvgpr_write_b32 %0, %1" : "=a"(a.lo) : "v"(lo), "v"(dep));
  asm("v_accvgpr_write_b32 %0, %1" : "=a"(a.hi) : "v"(hi), "v"(dep));
  return a;
}
__device__ __forceinline__ double agd_get(const agd a) {
  int lo, hi;
  asm("v_accvgpr_read_b32 %0, %1" : "=v"(lo) : "a"(a.lo));
  asm("v_accvgpr_read_b32 %0, %1" : "=v"(hi) : "a"(a.hi));
  return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double mfma444(const double a, const double b, const double c) {
  return __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, c, 0, 0, 0);
}

constexpr int DPP_ROW_ROR4 = 0x124, DPP_ROW_ROR8 = 0x128;

// a where m is all ones, b where m is 0: a select on the bit patterns, no condition mask
__device__ __forceinline__ double bit_pick(const int m, const double a, const double b) {
  const int lo = (__double2loint(a) & m) | (__double2loint(b) & ~m), hi = (__double2hiint(a) & m) | (__double2hiint(b) & ~m);
  return __hiloint2double(hi, lo);
}

// The weight-gradient blocks contract over POINTS, so both their operands need the point index where the matrix instruction
// contracts (lane bits 4-5) and the feature slot on bits 0-1.  Rounds 2-5 moved every value there with a ds_bpermute pair
// (a rotation of the lane index by two bits): 642 of them per tile, ~31 cycles of the LDS pipe each with four waves on the
// CU -- a quarter of the kernel's time (profiles/r06_stamps2_new.txt).  The matrix instruction itself can do the move: with
// the 4 x 4 identity as B (lane 16k + 4b + j holds [k == j]),
//     D[i][j] = sum_k A[i][k] [k == j] = A[i][j]:   lane 16i + 4b + j  <-  lane 16j + 4b + i,
// i.e. the slot field and the low two point bits of the lane index change places inside every block -- exactly a valid
// operand layout for the gradient blocks (contraction over the low point bits, one block per high-point-bit value; both
// operands and the "ones" / (hx, ht, 1) patterns of the bias and first-layer blocks use the same convention).  Products
// with 1.0 and sums with zeros are exact, so a FINITE moved value is bit-identical to the lane copy's, except that -0.0
// arrives as +0.0 (-0.0 + 0.0); an Inf or NaN in one lane becomes NaN in the other three lanes of its group (Inf x 0).  One
// instruction of the matrix pipe (16 cycles, no LDS round trip, no address register) instead of two of the LDS pipe.

// tanh(x) = sign(x) (1 - t) / (1 + t), t = e^{-2|x|}: the denominator lies in (1, 2], so the quotient needs none of
// the scaling / fix-up of an IEEE division: v_rcp_f64 seed + two Newton steps (relative error < 1e-30 before the
// final rounding), 5 instructions instead of 11.
__device__ __forceinline__ double tanh_d(const double x) {
  const double t = exp(-2.0 * fabs(x));
  const double y = 1.0 + t;
  double r = __builtin_amdgcn_rcp(y);
  r = __builtin_fma(__builtin_fma(-y, r, 1.0), r, r);
  r = __builtin_fma(__builtin_fma(-y, r, 1.0), r, r);
  const double num = 1.0 - t;
  double qv = num * r;
  qv = __builtin_fma(__builtin_fma(-y, qv, num), r, qv);      // one correction of the quotient itself
  return copysign(qv, x);
}

// layer-output channels (h, p, q, r) of a stash entry (a, zp, zq, zr)           (A.1)
__device__ __forceinline__ void channels_d(const double a, const double zp, const double zq, const double zr,
                                           double& h, double& p, double& q, double& r) {
  const double d1 = __builtin_fma(-a, a, 1.0);
  const double t = (-2.0 * a) * zp;
  h = a; p = d1 * zp; q = d1 * zq; r = d1 * __builtin_fma(t, zp, zr);
}

// adjoint of the pre-activation channels                                          (A.3)
__device__ __forceinline__ void preact_adjoint_d(const double a, const double zp, const double zq, const double zr,
                                                 const double oh, const double op, const double oq, const double orr,
                                                 double& bh, double& bp, double& bq, double& br) {
  const double a2 = a * a, d1 = 1.0 - a2;
  const double d2 = (-2.0 * a) * d1;
  const double d3 = (-2.0 * d1) * __builtin_fma(-3.0, a2, 1.0);
  const double zpw = zp * orr;
  const double dot = __builtin_fma(zr, orr, __builtin_fma(zq, oq, zp * op));
  bh = __builtin_fma(d3 * zp, zpw, __builtin_fma(d2, dot, d1 * oh));
  bp = __builtin_fma(d2 + d2, zpw, d1 * op);
  bq = d1 * oq;
  br = d1 * orr;
}

// The two functions above as traits of PDE, called from the forward sweep, the rotated-input macro, first_nat and dense 0: every
// kind gets them as they are; PDE_ADR2 (u_xx + kappa u_tt as the fourth channel, kernels_generic.h) adds its kappa terms as fmas
// whose multiplicand holds kappa, so kappa = 0 adds exact zeros and the values are PDE_ADR_SRC's
template <int PDE>
__device__ __forceinline__ void channels_pde_d(const double a, const double zp, const double zq, const double zr, const double kap,
                                               double& h, double& p, double& q, double& r) {
  if constexpr (PDE == PDE_ADR2) {
    const double d1 = __builtin_fma(-a, a, 1.0);
    const double t = (-2.0 * a) * zp, tq = (-2.0 * a) * zq;
    h = a; p = d1 * zp; q = d1 * zq; r = d1 * __builtin_fma(kap * tq, zq, __builtin_fma(t, zp, zr));
  } else {
    (void)kap;
    channels_d(a, zp, zq, zr, h, p, q, r);
  }
}
template <int PDE>
__device__ __forceinline__ void preact_adjoint_pde_d(const double a, const double zp, const double zq, const double zr,
                                                     const double kap, const double oh, const double op, const double oq,
                                                     const double orr, double& bh, double& bp, double& bq, double& br) {
  preact_adjoint_d(a, zp, zq, zr, oh, op, oq, orr, bh, bp, bq, br);
  if constexpr (PDE == PDE_ADR2) {
    const double a2 = a * a, d1 = 1.0 - a2;
    const double d2 = (-2.0 * a) * d1;
    const double d3 = (-2.0 * d1) * __builtin_fma(-3.0, a2, 1.0);
    const double zqw = zq * orr;
    bh = __builtin_fma((kap * d3) * zq, zqw, bh);
    bq = __builtin_fma(kap * (d2 + d2), zqw, bq);
  } else {
    (void)kap;
  }
}
// kappa of the kind's slot: PDE_ADR2's, 0 (and unused) everywhere else
template <typename Slot> __device__ __forceinline__ double f20d_kappa(const Slot&) { return 0.0; }
__device__ __forceinline__ double f20d_kappa(const Adr2Arg<double>& a) { return a.kappa; }

// ONE_TILE: the launch has at least as many workgroups as tiles: every gradient block is produced exactly once, so
// it is stored, not accumulated (no LDS read-modify-write), and there is no loop-carried coordinate prefetch.
// ENS: ensemble launch, grid (n_wg, members) over a shared point set: member m = blockIdx.y reads its weights at
// th + m * fused20d_weight_doubles(n_theta) and writes its gradient rows at part + m * gridDim.x * R; everything else is the
// solo kernel's, so a member's rows are bit-identical to those of a solo launch with the same n_wg.  (A template flag, not a
// wrapper around a shared body: the wrapper changed the schedule of the solo instantiations.)
// SETS (with ENS): every member has its own point set of the common SetDesc -- member m reads xs, ts and tgt at
// m * sd.n_pad -- and its own viscosity, nu[m] of a device array [members] passed in the slot of the scalar (a pointer
// has the size and alignment of a double, so the argument layout of every instantiation is the same).
// SAW: self-adaptive point weights (McClenny & Braga-Neto, arXiv:2009.04544), pde 0, solo launch: data point j and collocation
// point i count with m(lambda) = lambda^2, i.e. inv_nu * lambda_u,j^2 and inv_nf * lambda_f,i^2 stand where inv_nu and inv_nf
// stand in the plain kernel.  The SaArgs travel in the slot of the scalar nu (as SETS's pointer does), so the argument
// layout of every other instantiation stays as it was.  With `update` set (an Adam step) the slot-0 lane of a point writes
// back lambda, m and v after one ascent step on dL/dlambda = 2 lambda r^2 inv_n -- its own residual only, no reduction.
// PDE == PDE_ADR (advection-diffusion-reaction with run-time coefficients, kernels_generic.h), solo launch: the six
// coefficients travel in the same slot (AdrCoef<double>, wave-uniform), and the set's periodic boundary pairs are stored
// pair-interleaved, so the partner of point pt is pt ^ 1 = the neighbouring lane of the same slot: its (u, u_x) come by one
// DPP quad permutation per 32-bit half -- no second launch, no LDS hand-over, no barrier.  The boundary part of the loss is
// summed in the third per-wave slot (lacc[128], free when PDE != 1) and lands in the row at n_theta + 2.
// PDE == PDE_ADR_IDE (the same equation, coefficients trainable, kernels_generic.h), solo launch: the slot carries the mask
// of trained coefficients (AdrIdeArg); the coefficients are entries n_net .. n_net + 5 of the LDS weight copy.  Every wave
// parks a0, a1, nu = exp(log nu), r1, r2, r3, 1 / n_b and the mask in the fourth quarter of its loss-part slots once
// (lacc[192..], one exp per wave) and reads them back per tile, wave-uniform, as PDE_ADR's tile loop does -- no scalar
// register is held across the sweep.  The six coefficient sums cost no new LDS and no register across the sweep either: all
// four slot lanes of a point hold the same o[0..3] and only the slot-0 lanes touch the loss-part slots, so slot lanes 1-3
// of quarter 0 sum d/d (a0, a1, log nu) beside loss_f, those of quarter 1 d/d (r1, r2, r3) beside the data part; each DPP
// row of a quarter is reduced on its own (row16_sum, fixed order) and the per-wave hand-over grows from 4 to 9 values.
// PDE == PDE_ADR with SAW (per-point loss weights, pinn_pw_*), solo launch: the slot carries AdrPwArgs -- the six
// coefficients, the weight array and the step's bias-correction factor (0: the weights are only read).
// The array is indexed by the point (fused20d_api.h): a pair's two lanes read the lo point's entry, so both seed with the
// pair's one lambda, and only the slot-0 lane of the lo point steps it.  Coefficients, 1 / n_b and the array's header are
// parked per wave as PDE_ADR_IDE parks its values, in both variants; inv_n * lambda^2 is formed as SAW forms it for pde 0.
// PDE == PDE_ADR_ROBIN (PDE_ADR with Robin points, kernels_generic.h), solo launch, no point weights: the slot carries
// AdrRobinArg<double> -- the six coefficients, the (alpha, beta) array, the Robin block's first point and length, 1 / N_w.  The
// seed block is PDE_ADR's with one more class branch behind the pairs' (the two DPP moves stay in front of it): a Robin lane
// loads its (alpha, beta) pair (one 16-byte load, issued at the seed block: the one-tile ADR variants have 8 vector
// registers left, too few to hold two more doubles across the forward sweep) and g = tgt[pt], its slot-0 lane adds
// r^2 / N_w to the boundary slot lacc[128], and it seeds sb[0] and sb[1].  Tile loop: first, length and 1 / N_w are parked
// behind the other seven in lacc[192..] (slots 7-9) and the array's address is held in vector registers, as SAW holds its own.
// PDE == PDE_ADR_SRC (PDE_ADR with a source term, kernels_generic.h): PDE_ADR_ROBIN's
// text -- the slot carries AdrSrcArg<double>, the Robin count may be 0 -- with one more operation in the collocation class:
// f is formed as PDE_ADR forms it, then s_i = tgt[pt] is subtracted, uncontracted (a zero source gives PDE_ADR's bits).  The
// value is loaded at the seed block.  No seed formula changes.
// PDE == PDE_ADR_VAR (PDE_ADR with per-point coefficient fields, kernels_generic.h):
// PDE_ADR_SRC's text -- the slot carries AdrVarArg<double>, the Robin count may be 0, the collocation slots of tgt are zero
// without a source -- with one change in the collocation class: the six coefficients are the point's own row of the table,
// kf + 6 (pt - 2 n_b - n_u), three 16-byte loads issued at the seed block inside the collocation branch (the table has n_f
// rows; no other lane touches it).  Residual, source subtraction and the four seeds keep their expressions, so a table of
// constant rows gives PDE_ADR_SRC's bits.  1 / n_b, the Robin triple and the pair exchange are untouched.  Tile loop: the
// table's address is held in vector registers, as the (alpha, beta) array's is.
// PDE == PDE_ADR_ENS (PDE_ADR in an ensemble launch, kernels_generic.h), ENS with or
// without SETS: the slot carries AdrEnsArg, the address of the members' coefficient table [members][8].  Member m = blockIdx.y
// reads its row at the very top of the kernel, wave-uniform (nothing in front of the loads writes memory, so they are
// scalar loads); the six then stand where PDE_ADR's by-value AdrCoef stands -- in scalar registers in the one-tile variant,
// parked with 1 / n_b in lacc[192..] in the tile loop -- and the seed block is PDE_ADR's text.  The member offsets of th, part
// and (SETS) xs, ts, tgt are the Burgers ensemble's.
//
// The type of the slot: what the kind passes everywhere (pde_coef_t) unless the variant puts something else there.  A trait
// with a specialisation per exception: the kernels' mangled names spell F20dArg<PDE, SETS, SAW>::type and nothing about
// which specialisations exist, so a new variant adds a line here (or to PdeCoef, kernels_generic.h) and renames no kernel.
template <int PDE, bool SETS, bool SAW> struct F20dArg { using type = pde_coef_t<double, PDE>; };
template <> struct F20dArg<0, true, false> { using type = const double*; };
template <> struct F20dArg<1, true, false> { using type = const double*; };
template <> struct F20dArg<0, false, true> { using type = SaArgs; };
template <> struct F20dArg<PDE_ADR, false, true> { using type = AdrPwArgs; };
template <int PDE, bool SETS, bool SAW> using f20d_slot_t = typename F20dArg<PDE, SETS, SAW>::type;
__device__ __forceinline__ double f20d_nu(double nu) { return nu; }
__device__ __forceinline__ double f20d_nu(const AdrIdeArg&) { return 0.0; }
__device__ __forceinline__ double f20d_nu(const AdrCoef<double>& k) { return k.nu; }
__device__ __forceinline__ double f20d_nu(const double* nu) { return nu[blockIdx.y]; }   // wave-uniform
__device__ __forceinline__ double f20d_nu(const SaArgs& a) { return a.nu; }
__device__ __forceinline__ double f20d_nu(const AdrPwArgs& a) { return a.k.nu; }
__device__ __forceinline__ double f20d_nu(const AdrRobinArg<double>& a) { return a.k.nu; }
__device__ __forceinline__ double f20d_nu(const Adr2Arg<double>& a) { return a.k.nu; }
__device__ __forceinline__ double f20d_nu(const AdrEnsArg&) { return 0.0; }               // (read from the member's row)
// what a kernel holds of its member's row: the six coefficients (PDE_ADR_ENS), nothing at all (every other kind)
template <int PDE> struct F20dEnsCoef { struct type {}; };
template <> struct F20dEnsCoef<PDE_ADR_ENS> { using type = AdrCoef<double>; };
template <int PDE> using f20d_ens_coef_t = typename F20dEnsCoef<PDE>::type;

static_assert(F20D_WIDTH == FW && f20d_layer_first(1) == w20_desc(8, 0).off_w[1] && f20d_layer_first(7) == w20_desc(8, 2).off_w[7] &&
              f20d_layer_first(4) == w20_desc(4, 0).off_w[4] && f20d_n_net(6) == w20_desc(6, 2).n_net,
              "fused20d_api.h's layer offsets are the flat layout's");
// The kernel text, once under each of its two names: k_fused20d, and k_split20d with the two roles compiled in.
#define PINN_F20D_SPLIT 0
#define PINN_F20D_KERNEL k_fused20d
#include "kernels_fused20d_kernel.h"
#undef PINN_F20D_KERNEL
#undef PINN_F20D_SPLIT
#if PINN_ONETILE_SUM == 0
#define PINN_F20D_SPLIT 1
#define PINN_F20D_KERNEL k_split20d
#include "kernels_fused20d_kernel.h"
#undef PINN_F20D_KERNEL
#undef PINN_F20D_SPLIT
#endif

// One loss+gradient evaluation by k_fused20d<PDE, H, ., ENS, SETS, SAW> (F20dLaunch, fused20d_api.h; nu: the variant's
// coefficient argument).  Every member runs the solo launch plan: the one-tile instantiation when each tile has a workgroup
// of its own, the tile loop otherwise, on a grid of (n_wg, n_members).  With both events given they take the kernel's own
// begin / end timestamps.  Returns a hipError_t (0 = ok).
template <int PDE, int H, bool ENS, bool SETS, bool SAW>
inline int fused20d_launch(const F20dLaunch& a, const f20d_slot_t<PDE, SETS, SAW>& nu) {
  if (!w20_layout_ok(a.nd, H, pde_n_tail(PDE)) || (!ENS && a.n_members != 1)) return (int)hipErrorInvalidValue;
  const size_t lds = fused20d_lds_bytes(H, a.nd.n_theta);
  static unsigned long long attr_set = 0;
  if (first_call_on_device(attr_set)) {
    hipError_t e = hipFuncSetAttribute((const void*)&k_fused20d<PDE, H, false, ENS, SETS, SAW>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e == hipSuccess)
      e = hipFuncSetAttribute((const void*)&k_fused20d<PDE, H, true, ENS, SETS, SAW>,
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  const int n_tiles = a.sd.n_pad / 64;
  if (a.split) {
    // one main workgroup per tile and one helper per pair of tiles; the rows, R and n_wg are the plain launch's
    if constexpr (fused20d_split_built() && (PDE == 0 || PDE == 1) && !ENS && !SETS && !SAW) {
#if PINN_ONETILE_SUM == 0
      if (a.n_wg < n_tiles) return (int)hipErrorInvalidValue;
      auto* const ks = &k_split20d<PDE, H, true, false, false, false>;
      static unsigned long long split_attr_set = 0;
      if (first_call_on_device(split_attr_set)) {
        const hipError_t e = hipFuncSetAttribute((const void*)ks, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
      }
      const dim3 grid(fused20d_split_grid(n_tiles));
      if (a.ev_start && a.ev_stop)
        hipExtLaunchKernelGGL(ks, grid, dim3(256), lds, a.stream, a.ev_start, a.ev_stop, 0, a.th, a.xs, a.ts, a.tgt, a.part,
                              a.row_index, a.R, n_tiles, a.lbx, a.lbt, a.sx, a.st, nu, a.sd, a.stamps, w20_desc(H, pde_n_tail(PDE)));
      else
        hipLaunchKernelGGL(ks, grid, dim3(256), lds, a.stream, a.th, a.xs, a.ts, a.tgt, a.part, a.row_index, a.R, n_tiles,
                           a.lbx, a.lbt, a.sx, a.st, nu, a.sd, a.stamps, w20_desc(H, pde_n_tail(PDE)));
      return (int)hipGetLastError();
#endif
    }
    return (int)hipErrorInvalidValue;
  }
  auto* const kern = a.n_wg >= n_tiles ? &k_fused20d<PDE, H, true, ENS, SETS, SAW> : &k_fused20d<PDE, H, false, ENS, SETS, SAW>;
  const dim3 grid(a.n_wg, a.n_members);
  if (a.ev_start && a.ev_stop)
    hipExtLaunchKernelGGL(kern, grid, dim3(256), lds, a.stream, a.ev_start, a.ev_stop, 0, a.th, a.xs, a.ts, a.tgt, a.part,
                          a.row_index, a.R, n_tiles, a.lbx, a.lbt, a.sx, a.st, nu, a.sd, a.stamps, w20_desc(H, pde_n_tail(PDE)));
  else
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, a.stream, a.th, a.xs, a.ts, a.tgt, a.part, a.row_index, a.R, n_tiles,
                       a.lbx, a.lbt, a.sx, a.st, nu, a.sd, a.stamps, w20_desc(H, pde_n_tail(PDE)));
  return (int)hipGetLastError();
}

}  // namespace pinn
