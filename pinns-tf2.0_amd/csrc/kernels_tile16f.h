// kernels_tile16f.h -- k_t16_fused: the float64 MFMA sweeps of kernels_tile16.h for hidden widths 65..128 with the
// forward and the reverse sweep of a 16-point group in ONE kernel and the stash in registers -- no HBM stash.
//
// Why (BASELINE configs[3]: the Schrodinger net 2-100x4-2 in the reference's arithmetic, N_f = 20000).  The two-kernel
// sweeps move 1.25 GB per evaluation for 0.3 MB of coordinates (profiles/r04_pmc_fetch_write_cfg4_two_kernel.txt): k_t16_fwd writes
// the 6.4 KB/point stash (253 MB), k_t16_bwd reads it back and read-modify-writes the 246 KB gradient row of its
// workgroup once per group (295 MB raw fetched, 366 MB written); ablation (profiles/r03_ablate_t16_f64_w8.txt): stash
// stores / loads -16 / -64 us, row read-modify-write -83 us of 583.
//
// What fits on the chip (one CU, float64, width 100 padded to 7 x 16 = 112 rows, 16-point group):
//   register file 512 KB, LDS 160 KB.
//   exchange tiles  2 x [128][17] x 32 B                           = 139 KB   LDS (B operands of the layer GEMMs, both
//                                                                             operands of the weight-gradient tiles)
//   stash (a, z_x, z_t, z_xx), hidden layers 1..H-1: 3 x 51.2 KB   = 154 KB   -> 96 registers per lane at 8 waves
//   weight-gradient accumulators 3 x 49 tiles x 256 x 8 B          = 301 KB   -> 147 registers per lane at 8 waves
//   the sweeps' own working set (k_t16_bwd: 175 - 32 stash reads)  ~ 143 registers per lane
// 96 + 147 + 143 = 386 > 256 registers per lane (two waves per SIMD; one wave per SIMD has 512 but was measured 30 %
// slower on these sweeps, profiles/r03_t16_ab.txt), and LDS has 21 KB left.  So ONE of the two traffic sources can go.
// This kernel removes the stash (both directions: 509 MB, and one launch); the hidden-layer weight gradients stay a
// read-modify-write per group -- of a tile-major scratch (whole cache lines) which the reduction kernels read directly
// (kernels_optim.h TileScratch; until round 5 it was copied into the partial row at the end of the kernel).
// Layer 0's stash entry is tanh of an affine function of (x, t): recomputed where it is needed, never stored.
//
// Round 5: work is dealt in 4-row STRIPS where a 16-row tile would carry padding.  Width 100 = 25 strips:
// the layer GEMMs' rows belong to waves 0-3 as 16-row tiles (v_mfma_f64_16x16x4) and to waves 4-7 as 2, 2, 2, 3 strips
// (v_mfma_f64_4x4x4, operand broadcast by ds_swizzle, raised wave priority: kernels_tile16.h t16_mma_kstep); the 13 of 49
// gradient tiles with four live rows or columns run as strips too, and tiles, strips and GEMMs are dealt by cost so that
// the four SIMDs carry the same matrix time (T16Deal below).  Issued matrix FLOP = algorithmic + 0.6 % (was + 13 %).
//
// Structure: the arithmetic of k_t16_fwd<double, 8, false, 8> followed by k_t16_bwd<double, 8, PDE, false, 8> (same
// matrix-instruction order in the GEMMs, same tanh; the per-feature sums over a group's points are DPP row sums here, so
// results agree with the two-kernel path to ~1e-16, not bit for bit), with every stash access turned into a register
// access of the lane that produced the entry: wave w owns
// the same feature rows (row0[w] + out_row(lane, r), r < ns[w]) in the forward GEMM AND in the adjoint GEMM, so an entry
// is produced and consumed by the same lane; the elementwise passes of k_t16_bwd that read the stash in (row, point) order are
// re-dealt to the owning lanes.  After the forward sweep the two exchange tiles already hold what the first reverse
// step needs (outputs of layers H-1 and H-2).
// Periodic-boundary seeds (1dcomplex-schrodinger/inf_cont_schrodinger.py:107-129) read the OUTPUTS of a partner point
// that another workgroup may own: the boundary groups are each the first group of their workgroup and hand their outputs
// over inside the kernel (fence + counter + a wait bounded by the wall clock, below); when there are more boundary groups
// than workgroups, on PINN_T16_PREPASS=1, or for good after a hand-over that timed out (a GPU shared with another process:
// engine.hip t16_handover_check turns the device flag into an explicit error) the engine runs k_t16_fwd over them first.
// Where the time of a group goes: profiles/t16f_stamps.py (profiling build), DESIGN.md 4.3.
#pragma once
#include <type_traits>
#include "kernels_tile16.h"

namespace pinn {

// Profiling build (-DPINN_STAMPS, libpinn_hip_stamps.so): s_memtime at the phase boundaries of workgroup 0's SECOND
// group, every wave; read back through pinn_debug_t16f_stamps (profiles/t16f_stamps.py).  Product build: nothing.
#ifdef PINN_STAMPS
__device__ long long g_t16f_stamps[8 * 64];
#define FSTAMP(i)                                                                                         \
  do {                                                                                                    \
    if (blockIdx.x == 0 && grp == (int)gridDim.x && lane == 0) g_t16f_stamps[wave * 64 + (i)] = clock64(); \
  } while (0)
#define KSTAMP(i)                                                                                         \
  do {                                                                                                    \
    if (blockIdx.x == 0 && (threadIdx.x & 63) == 0) g_t16f_stamps[(threadIdx.x >> 6) * 64 + (i)] = clock64(); \
  } while (0)
#else
#define FSTAMP(i) do { } while (0)
#define KSTAMP(i) do { } while (0)
#endif

// dynamic LDS of the kernel; t16_fused_small_in_lds: the per-feature gradients of the biases and of layer 0 ((H + 2) W
// doubles) fit behind the fixed areas and are accumulated there over the groups instead of in the row
// (round 5: the exchange tiles hold 16 ceil(W / 16) rows instead of 128 -- width 100: 17 KB back -- and the parameters every
//  group re-read from L2 outside the GEMMs, dense 0's (w_x, w_t, b) and the output layer's (W, b), are staged behind them when
//  they fit: t16_fused_const_in_lds)
__host__ __device__ inline size_t t16_fused_fixed_doubles(int W) {
  return (size_t)2 * (16 * ((W + 15) / 16)) * T16Geo<8>::PD * 4 + 2 * 8 * 2 * 16 * 4 + 2 * 16 * 4 + 32 + 7 * 16;
}
__host__ __device__ inline bool t16_fused_small_in_lds(int W, int H) {
  return (t16_fused_fixed_doubles(W) + (size_t)(H + 2) * W) * sizeof(double) <= 160 * 1024;
}
__host__ __device__ inline size_t t16_fused_const_doubles(int W, int NO) { return (size_t)3 * W + (size_t)W * NO + NO; }
__host__ __device__ inline bool t16_fused_const_in_lds(int W, int H, int NO) {
  return t16_fused_small_in_lds(W, H) &&
         (t16_fused_fixed_doubles(W) + (size_t)(H + 2) * W + t16_fused_const_doubles(W, NO)) * sizeof(double) <= 160 * 1024;
}
inline size_t t16_fused_lds(int W, int H, int NO) {
  return (t16_fused_fixed_doubles(W) + (t16_fused_small_in_lds(W, H) ? (size_t)(H + 2) * W : 0) +
          (t16_fused_const_in_lds(W, H, NO) ? t16_fused_const_doubles(W, NO) : 0)) * sizeof(double);
}

// Work of one reversed layer dealt to the eight waves (round 5).  Width 100 pads to 7 x 16 = 112 rows: as 16x16 tiles that
// is 49 gradient tiles + 7 feature tiles per layer GEMM of which 13 + 1 carry FOUR live rows or columns -- 13 % of the
// issued v_mfma_f64_16x16x4 work was padding (profiles/r04_pmc_sq_t16_fused_v4.txt), and wave 7, which owns no feature
// tile, was the long pole of every reverse phase with 13 tiles.  When the last tile per side has at most four live rows
// (edge = 1) those 4-row / 4-column STRIPS run on v_mfma_f64_4x4x4 (four independent 4x4x4 blocks: a 16 x 4 strip per
// instruction in 16 cycles instead of 64, same FLOP per cycle; lane maps in kernels_tile16.h t16_mma and below), and the
// tiles are dealt by COST (units of one 16x16x4 instruction = 64 cycles: full tile 16, strip 4, layer GEMM of a full
// feature tile 4 ksteps, of the edge feature tile ksteps) so that every wave -- hence every SIMD -- carries the same
// matrix time.  Width 100: 1253 units per layer, 156-160 per wave (was: 25.5 k cycles on the busiest SIMD, now 20.2 k).
struct T16Deal {
  unsigned char f_lo[8], f_hi[8];   // this wave's range in the list of FULL tiles: i -> (rt, ct) = (i / nfs, i % nfs)
  unsigned char e_lo[8], e_hi[8];   // ... in the list of strips: i < ntl-1: four live COLUMNS (rt = i, ct = ntl-1);
                                    //     then four live ROWS (rt = ntl-1, ct = i - (ntl-1)), the corner last
  int edge;                         // 1: strips in use (1 <= W % 16 <= 4); 0: every tile is a full tile, e ranges empty
  // Feature rows of the layer GEMMs (forward and adjoint): wave w owns rows [row0[w], row0[w] + 4 ns[w]) -- waves 0-3 a
  // 16-row tile (ns = 4: v_mfma_f64_16x16x4), waves 4-7 the remaining ceil(W / 4) - 16 strips of four rows as evenly as
  // they go (ns <= 3: v_mfma_f64_4x4x4 per strip, kernels_tile16.h t16_mma_kstep; ns = 4: a tile).  Width 100: 2, 2, 2, 3
  // -- every SIMD carries 6-7 strips of a layer GEMM instead of 8, 8, 5, 4 (tiles 4 and 5 on the SIMDs of tiles 0 and 1,
  // wave 7 idle: profiles/r04_t16f_stamps_final.txt, forward GEMM phase 15.5 k cycles for 12.8 k of matrix instructions
  // on the busiest SIMD and 6.4 k on the idlest).
  unsigned char row0[8], ns[8];
};

// cost_full / cost_strip: what a full tile / a strip costs a wave, in units of one 16x16x4 instruction of a layer GEMM:
// 16 and 4 by instruction count, 22 and 12 as measured -- a tile's 16 instructions come with 16 ds_read_b128 and a scratch
// read-modify-write, a strip's 16 short ones with the same reads (profiles/r05_t16f_deal_sweep.txt: 380.5 us per step at
// 16,4; 373-377 between 18,6 and 24,12; with the scratch-backed reduction 371.5 vs 364.6).  PINN_T16_COSTS="full,strip"
// overrides them.
constexpr double T16_COST_FULL = 22.0, T16_COST_STRIP = 12.0;
inline T16Deal t16_deal(int W, double cost_full = T16_COST_FULL, double cost_strip = T16_COST_STRIP) {
  T16Deal d{};
  const int ntl = (W + 15) / 16, ksteps = (W + 3) / 4, rem = W % 16;
  d.edge = (rem >= 1 && rem <= 4 && ntl >= 2) ? 1 : 0;
  const int nfs = d.edge ? ntl - 1 : ntl, n_full = nfs * nfs, n_edge = d.edge ? 2 * ntl - 1 : 0;
  {  // rows of the layer GEMMs
    const int S = (W + 3) / 4, R = S > 16 ? S - 16 : 0, base = R / 4, extra = R % 4;
    int row = 0;
    for (int w = 0; w < 8; ++w) {
      const int n = w < 4 ? (S >= 4 * (w + 1) ? 4 : S > 4 * w ? S - 4 * w : 0) : base + ((w - 4) >= 4 - extra ? 1 : 0);
      d.row0[w] = (unsigned char)row;
      d.ns[w] = (unsigned char)n;
      row += 4 * n;
    }
  }
  double gemm[8], budget[8], total = cost_full * n_full + cost_strip * n_edge;
  for (int w = 0; w < 8; ++w) {
    gemm[w] = (double)d.ns[w] * ksteps;        // 4 ksteps instructions of 64 cycles for a tile, ns ksteps x 4 of 16 cycles for strips
    total += gemm[w];
  }
  int nf[8], ne[8], sf = 0, se = 0;
  double want[8];
  for (int w = 0; w < 8; ++w) {
    budget[w] = total / 8.0 - gemm[w];
    if (budget[w] < 0) budget[w] = 0;
    want[w] = budget[w] / cost_full;
    nf[w] = (int)want[w];
    sf += nf[w];
  }
  while (sf != n_full) {               // largest (smallest) fractional part takes (gives) the odd tiles
    int best = -1;
    for (int w = 0; w < 8; ++w) {
      if (sf > n_full && nf[w] == 0) continue;
      const double fr = want[w] - nf[w];
      if (best < 0 || (sf < n_full ? fr > want[best] - nf[best] : fr < want[best] - nf[best])) best = w;
    }
    nf[best] += sf < n_full ? 1 : -1;
    sf += sf < n_full ? 1 : -1;
  }
  for (int w = 0; w < 8; ++w) {
    want[w] = (budget[w] - cost_full * nf[w]) / cost_strip;
    ne[w] = want[w] > 0 ? (int)(want[w] + 0.5) : 0;
    se += ne[w];
  }
  while (se != n_edge) {
    int best = -1;
    for (int w = 0; w < 8; ++w) {
      if (se > n_edge && ne[w] == 0) continue;
      const double fr = want[w] - ne[w];
      if (best < 0 || (se < n_edge ? fr > want[best] - ne[best] : fr < want[best] - ne[best])) best = w;
    }
    ne[best] += se < n_edge ? 1 : -1;
    se += se < n_edge ? 1 : -1;
  }
  int f = 0, e = 0;
  for (int w = 0; w < 8; ++w) {
    d.f_lo[w] = (unsigned char)f; f += nf[w]; d.f_hi[w] = (unsigned char)f;
    d.e_lo[w] = (unsigned char)e; e += ne[w]; d.e_hi[w] = (unsigned char)e;
  }
  return d;
}

template <int PDE, int H>
__global__ __launch_bounds__(512) void k_t16_fused(NetDesc nd, SetDesc sd, const double* __restrict__ th,
                                                   const double* __restrict__ xs, const double* __restrict__ ts,
                                                   const double* __restrict__ tgt, int base, int n_pad, int n_groups,
                                                   double lbx, double lbt, double sx, double st, double nu,
                                                   vec4<double>* __restrict__ O, double* __restrict__ part, int R,
                                                   int accumulate, unsigned int* __restrict__ bsync,
                                                   unsigned int btarget, int n_bgroups, double* __restrict__ gscr,
                                                   long long handover_ticks, T16Deal deal) {
  using real = double;
  using TR = FusedTraits<double>;
  using acc_t = typename TR::acc_t;
  using GEO = T16Geo<8>;
  using V4 = vec4<double>;
  static_assert(H >= 2, "at least one hidden-to-hidden layer");
  constexpr int NT = 8, NWV = 8, WP = GEO::WP, PD = GEO::PD, RP = 4 * NWV, THREADS = 64 * NWV;
  constexpr int NI = WP / RP, KS = 2 * NWV, NKO = WP / KS;
  (void)NT;
  extern __shared__ __attribute__((aligned(16))) char t16_smem[];
  V4* const T0 = reinterpret_cast<V4*>(t16_smem);
  const int rowsP = 16 * ((nd.width + 15) >> 4);                  // rows of an exchange tile (<= WP = 128)
  V4* const T1 = T0 + rowsP * PD;
  real* const red = reinterpret_cast<real*>(T1 + rowsP * PD);     // [2 NWV][2][16][4] output-layer partials
  V4* const seeds = reinterpret_cast<V4*>(red + 2 * NWV * 2 * 16 * 4);   // [2][16]
  real* const hxy = reinterpret_cast<real*>(seeds + 32);          // [2][16] normalised inputs
  real* const lsum = hxy + 32;                                    // [7][16] per-point-slot sums over the groups: loss parts (3),
                                                                  // lambda gradients (2), output-bias gradients (2)
  // Small gradients accumulated ON CHIP over the workgroup's groups and added into the row once: read-modify-writes of
  // the row per group are dependent global round trips (~1.5 k cycles each, a dozen per group on the critical path).
  //   gsm[(H + 2) W] (LDS, when it fits: t16_fused_small_in_lds): bias gradients of layers 1..H-1, then layer 0's
  //   (d/dW_x, d/dW_t, d/db) per feature;  gwacc (registers): output-layer weight gradients, per lane, summed over the
  //   16 points of a DPP row at the end
  real* const gsm = lsum + 7 * 16;
  const bool small_lds = t16_fused_small_in_lds(nd.width, H);
  // parameters used outside the GEMMs, staged once per workgroup (when they fit): [w_x | w_t | b] of dense 0, then the output
  // layer's W [k][o] and b.  Every group read them from L2 in its dense-0, output-layer, dense-H-reverse and last-epilogue
  // phases -- phases with nothing to hide a 1.5 k-cycle round trip behind.
  real* const cst = gsm + (small_lds ? (H + 2) * nd.width : 0);
  const bool cst_lds = t16_fused_const_in_lds(nd.width, H, nd.n_out);
  const int tid0 = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid0 >> 6);
  const int W = nd.width, NO = nd.n_out;
  const int ksteps = (W + 3) / 4;
  const int row0 = deal.row0[wave], ns = deal.ns[wave];           // wave-uniform: this wave's rows of the layer GEMMs (T16Deal)
  const bool tile_live = ns > 0;
  constexpr int T16_STRIP_PRIO = 3;
  // A strips wave shares its SIMD with a tile wave.  With equal priority the arbiter alternates between them instruction
  // by instruction: every 16-cycle strip instruction then queues behind one 64-cycle tile instruction -- 200 x 80 cycles
  // for 3.3 k of matrix time (profiles/r05_t16f_stamps_edge_v6.txt: strips GEMM 14.8 k, the tile wave's 9.9 k).  Raised
  // priority lets the strips wave issue a k-step's 8-12 short instructions back to back; the tile wave runs in its waits.
  if (ns > 0 && ns < 4) __builtin_amdgcn_s_setprio(T16_STRIP_PRIO);
  real* __restrict__ row = part + (size_t)blockIdx.x * R;
  // Hidden-to-hidden weight gradients are accumulated over the workgroup's groups in a TILE-MAJOR scratch of its own
  // (per layer and gradient tile: the 64 lanes' four accumulator values, 2 KB contiguous, whole cache lines read and
  // written) and copied into the partial row once at the end.  Adding each tile into the row directly (k_t16_bwd)
  // touches 16-double segments at an 800-byte row pitch: every segment straddles two cache lines and is written
  // partially -- profiles/r04_pmc_fetch_write_cfg4_two_kernel.txt: 295 MB fetched (raw) / 366 MB written for 315 MB of entries,
  // and 70 of 520 us in this kernel (profiles/r04_ablate_t16_fused_v3.txt: 70 us before, 21 us with the scratch).
  const int ntl = (W + 15) >> 4, n_tiles = ntl * ntl;             // live gradient tiles per side / per layer
  real* __restrict__ gs = gscr + (size_t)blockIdx.x * (H - 1) * n_tiles * 256;
  real c1 = real(1), c2 = nu;
  if (PDE == 1) { c1 = th[nd.n_net]; c2 = exp_r(th[nd.n_net + 1]); }

  KSTAMP(60);
  // A fresh row (accumulate == 0) is STORED entry by entry at the end of the kernel -- every entry has exactly one owner
  // there -- instead of zeroed here and added into: the zero fill (246 KB per workgroup) and the read half of the final
  // read-modify-write were 12 k + ~65 k of the kernel's 995 k cycles (profiles/r04_t16f_stamps_v5.txt).  Only when the
  // small gradients do not fit in LDS (H = 4, widths 126..128) are they still accumulated in the row per group.
  const bool direct = !accumulate && small_lds;
  if (!accumulate && !direct) {
    for (int i = tid0; i < R; i += THREADS) row[i] = real(0);
    __syncthreads();                          // (global stores of one workgroup, read back by the same workgroup)
  }
  if (tid0 < 7 * 16) lsum[tid0] = real(0);    // (published by the first barrier of the group loop)
  {  // rows of the exchange tiles that no wave owns (beyond the last strip: width 100 -> rows 100..111) are read as operands
     // of full gradient tiles, by the output layer and by the last k-step of a GEMM: zero, once -- the sweeps write owned rows only
    const int first = 4 * ((nd.width + 3) / 4) * PD, n = rowsP * PD - first;
    for (int i = tid0; i < n; i += THREADS) { T0[first + i] = V4{0, 0, 0, 0}; T1[first + i] = V4{0, 0, 0, 0}; }
  }
  if (small_lds) for (int i = tid0; i < (H + 2) * nd.width; i += THREADS) gsm[i] = real(0);
  if (cst_lds) {
    for (int i = tid0; i < W; i += THREADS) {
      cst[i] = th[nd.off_w[0] + i]; cst[W + i] = th[nd.off_w[0] + W + i]; cst[2 * W + i] = th[nd.off_b[0] + i];
    }
    for (int i = tid0; i < W * NO + NO; i += THREADS) cst[3 * W + i] = i < W * NO ? th[nd.off_w[H] + i] : th[nd.off_b[H] + i - W * NO];
    __syncthreads();                          // dense 0 of the first group reads them before the loop's first barrier
  }
  // dense 0's parameter `which` (0 w_x, 1 w_t, 2 b) of feature j; the output layer's weight idx = k NO + o and bias o.  The
  // staged copy has the flat vector's own order ([W_0 (2 x W) | b_0] and [W_H (W x NO) | b_H] are contiguous there), so one
  // generic base pointer per block serves both sources (flat loads; wave-uniform pointers)
  const real* const base0 = cst_lds ? static_cast<const real*>(cst) : th + nd.off_w[0];
  const real* const baseH = cst_lds ? static_cast<const real*>(cst + 3 * W) : th + nd.off_w[H];
  auto p0 = [&](const int which, const int j) { return base0[which * W + j]; };
  auto pH = [&](const int idx) { return baseH[idx]; };
  auto bH = [&](const int o) { return baseH[W * NO + o]; };
  real gwacc[4][2] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}};

  // (k_t16_fwd keeps dense 0's parameters and the output layer's k-slice in registers across groups: 40 registers
  //  this kernel needs for the stash -- they are re-read from L2 per group instead)
  KSTAMP(61);
  for (int grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
    const int lp0 = grp * 16;
    // The lane index is re-read through an opaque asm once per group: every per-lane address of the body (six layer
    // matrices, the gradient-row entries of 49 tiles, biases, tiles) is loop-invariant, and with the layer loops
    // unrolled hipcc hoisted ~60 64-bit addresses out of the group loop and spilled them (568 B of scratch per lane)
    int lane = tid0 & 63;
    asm volatile("" : "+v"(lane));
    const int tid = wave * 64 + lane, m = lane & 15, g = lane >> 4, pe = lane & 15;
  // layer 0's stash entry of (feature j, point with normalised inputs hx, ht): recomputed, never stored
  auto dense0 = [&](const int j, const real hx, const real ht) {
    const real w0 = p0(0, j), w1 = p0(1, j), b0 = p0(2, j);
    return V4{tanh_mm(hx * w0 + ht * w1 + b0), sx * w0, st * w1, real(0)};
  };
  // one layer GEMM of this wave's feature tile: t16_gemm_l2 (kernels_tile16.h): unguarded chunks of four k-steps with
  // plain, triple-buffered weight loads from L2, the next k-step's LDS operands requested before the current matrix
  // instructions.
  // (Tried and dropped: requesting a GEMM's first two weight chunks ahead of the phase before it -- the previous layer's
  //  tanh epilogue, the gradient tiles -- so that no GEMM starts with a cold L2 round trip: 256 VGPRs instead of 238
  //  and 449 vs 446 us per step, same box: with two waves per SIMD the other wave already covers that latency.  Second
  //  attempt, right in front of the phase barrier only: 256 VGPRs + 40 B of scratch, 410.6 vs 404.3 us -- the kernel has
  //  no 16 registers to spare anywhere near a GEMM; profiles/r04_t16f_dw_pipeline_ab.txt.)
  auto gemm = [&](const real* __restrict__ Wm, const V4* __restrict__ Bt, auto tr_tag, acc_t& a0, acc_t& a1,
                  acc_t& a2, acc_t& a3) {
    if (ns < 4) t16_gemm_l2<real, decltype(tr_tag)::value, PD, acc_t, true>(Wm, Bt, W, row0 + m, m, g, a0, a1, a2, a3, ns);
    else t16_gemm_l2<real, decltype(tr_tag)::value, PD, acc_t>(Wm, Bt, W, row0 + m, m, g, a0, a1, a2, a3);
  };
  // feature row of accumulator entry r of this lane, or a row beyond every guard when the wave does not own strip r
  auto own_row = [&](const int r) { return r < ns ? row0 + TR::out_row(lane, r) : (1 << 20); };

  // Per-feature sums over the group's 16 points (bias gradients, layer 0's gradients): the lanes that PRODUCE a z_bar
  // entry (row j, point m) sum it over the 16 lanes of their DPP row and lane m == 0 adds it to the feature's slot -- no
  // extra pass over the tile by 100 threads of waves 0 / 1 while the other waves wait (2 k cycles per layer on the
  // critical path, profiles/r04_t16f_stamps_v5.txt).  One owner lane per (slot, feature): no synchronisation.
  auto feature_add = [&](const int slot, real* __restrict__ row_slot, const int j, const real x) {
    const real sum = row16_sum(x);
    if (m == 0 && j < W) {
      if (small_lds) gsm[slot * W + j] += sum;
      else row_slot[j] += sum;
    }
  };

    // =========================================================================================== forward sweep
    FSTAMP(0);
    real a0e[NI];                             // layer 0's tanh values of this thread's (feature, point) items: the reverse
                                              // sweep needs them twice more (a tanh is ~45 instructions; k_t16_bwd reads S)
    {  // dense 0: items (feature j, point pe), point fastest
      const real x = xs[base + lp0 + pe], t = ts[base + lp0 + pe];
      const real hx = sx * (x - lbx) - real(1), ht = st * (t - lbt) - real(1);
      if (tid < 16) { hxy[tid] = hx; hxy[16 + tid] = ht; }
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const int j = (tid >> 4) + RP * i;
        V4 c{0, 0, 0, 0};
        a0e[i] = real(0);
        if (j < W) {
          real d1, d2;
          const V4 s0 = dense0(j, hx, ht);
          a0e[i] = s0.x;
          c = channels_of(s0, d1, d2);
        }
        if (j < rowsP) T0[j * PD + pe] = c;
      }
    }
    V4 stash[H - 1][4];                       // hidden layers 1..H-1, this lane's four rows of its wave's tile
    V4* Tin = T0;
    V4* Tout = T1;
    FSTAMP(1);
#pragma unroll
    for (int l = 1; l < H; ++l) {
      __syncthreads();                        // Tin published
      FSTAMP(2 + 3 * (l - 1));
      if (!tile_live) {                       // no rows of its own (the padding rows of the tiles stay zero: see the prologue)
#pragma unroll
        for (int r = 0; r < 4; ++r) stash[l - 1][r] = V4{0, 0, 0, 0};
      } else {
        const real* __restrict__ bl = th + nd.off_b[l];
        real bj[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int j = own_row(r);
          bj[r] = j < W ? bl[j] : real(0);
        }
        acc_t a0 = {0, 0, 0, 0}, a1 = {0, 0, 0, 0}, a2 = {0, 0, 0, 0}, a3 = {0, 0, 0, 0};
        gemm(th + nd.off_w[l], Tin, std::false_type{}, a0, a1, a2, a3);
        FSTAMP(3 + 3 * (l - 1));
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int j = own_row(r);                                 // feature; the point is m
          V4 c{0, 0, 0, 0}, s{0, 0, 0, 0};
          if (j < W) {
            s = V4{tanh_mm(a0[r] + bj[r]), a1[r], a2[r], a3[r]};
            real d1, d2;
            c = channels_of(s, d1, d2);
          }
          stash[l - 1][r] = s;
          if (j < rowsP) Tout[j * PD + m] = c;
        }
      }
      FSTAMP(4 + 3 * (l - 1));
      V4* tmp = Tin; Tin = Tout; Tout = tmp;
    }
    __syncthreads();
    FSTAMP(14);
    {  // linear output layer: thread = (k-slice ks8, output o, point pe); the slices are summed through LDS
      const int o = (tid >> 4) & 1, ks8 = tid >> 5;
      V4 acc{0, 0, 0, 0};
#pragma unroll
      for (int i = 0; i < NKO; ++i) {
        const int k = ks8 + KS * i;
        const V4 b = k < rowsP ? Tin[k * PD + pe] : V4{0, 0, 0, 0};
        const real w = (k < W && o < NO) ? pH(k * NO + o) : real(0);
        acc.x += b.x * w; acc.y += b.y * w; acc.z += b.z * w; acc.w += b.w * w;
      }
      reinterpret_cast<V4*>(red)[(ks8 * 2 + o) * 16 + pe] = acc;
      __syncthreads();
      if (ks8 == 0 && o < NO) {
        V4 tot = reinterpret_cast<V4*>(red)[(0 * 2 + o) * 16 + pe];
#pragma unroll
        for (int q = 1; q < KS; ++q) {
          const V4 v = reinterpret_cast<V4*>(red)[(q * 2 + o) * 16 + pe];
          tot.x += v.x; tot.y += v.y; tot.z += v.z; tot.w += v.w;
        }
        tot.x += bH(o);
        O[(size_t)o * n_pad + base + lp0 + pe] = tot;            // (for the partner of a boundary pair, and pinn_predict's callers)
        seeds[o * 16 + pe] = tot;                                 // the group's own outputs stay on chip for the seeds
      }
    }
    FSTAMP(15);
    if (grp < n_bgroups) {
      // Periodic-boundary seeds read the outputs of a PARTNER point, which another workgroup may own.  The boundary
      // points fill the first n_bgroups groups of the set, each the FIRST group of its workgroup (grid >= n_bgroups,
      // checked by the host), so those workgroups are co-resident and reach this point without waiting for anybody:
      // publish (fence + counter), wait until all n_bgroups groups of this launch are published (the counter is
      // never reset: btarget = its value after this launch), then drop this CU's L1 so the partners' outputs are
      // read from L2.  Bounded by the 100 MHz wall clock (handover_ticks, 0.5 s by default): a partner that is not
      // resident in time (another process holds part of the GPU) raises bsync[1] -- the host turns that into an explicit
      // error at its next synchronisation and moves the context to the forward pre-pass (engine.hip:
      // t16_handover_check) -- and the loss of this evaluation is poisoned so that nothing consumes it silently.
      __threadfence();
      __syncthreads();
      if (tid == 0) {
        atomicAdd(bsync, 1u);
        const long long t0 = wall_clock64();
        bool arrived = false;
        do {
          arrived = (int)(__hip_atomic_load(bsync, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - btarget) >= 0;
          if (!arrived) __builtin_amdgcn_s_sleep(4);
        } while (!arrived && wall_clock64() - t0 <= handover_ticks);
        if (!arrived) {
          atomicExch(bsync + 1, 1u);
          lsum[0] = __builtin_nan("");
        }
      }
      __syncthreads();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    } else {
      __syncthreads();                        // the group's outputs are in memory (written and read by this workgroup)
    }
    FSTAMP(16);
    // =========================================================================================== reverse sweep
    if (tid < 16) {
      const int pt = base + lp0 + tid;
      V4 sb[2];
      real lt[3], dl[2];
      const V4 ou = seeds[tid], ov = NO > 1 ? seeds[16 + tid] : V4{0, 0, 0, 0};   // (read before this thread overwrites them)
      point_seeds_own<real, PDE>(sd, pt, n_pad, ou, ov, O, tgt, c1, c2, sb, lt, dl);
      seeds[tid] = sb[0]; seeds[16 + tid] = sb[1];
      lsum[tid] += lt[0]; lsum[16 + tid] += lt[1]; lsum[32 + tid] += lt[2];
      lsum[48 + tid] += dl[0]; lsum[64 + tid] += dl[1];
      lsum[80 + tid] += sb[0].x; lsum[96 + tid] += sb[1].x;
    }
    __syncthreads();
    FSTAMP(17);
    // Tin = outputs of layer H-1 (inputs of dense H), Tout = outputs of layer H-2 (inputs of layer H-1): the reverse
    // sweep starts with TI = Tout (A operand of dW_{H-1}) and overwrites Tin with the adjoint of layer H-1's
    // pre-activations
    V4* TI = Tout;
    V4* Bcur = Tin;
    {  // dense H (linear): z_bar = seeds.  This lane's four rows j of tile `wave`, point m: adjoint of layer H-1's
       // pre-activations, gradient of the output weights (sum over the 16 points = the 16 lanes of a DPP row)
      const V4 s0 = seeds[m], s1 = seeds[16 + m];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = own_row(r);
        V4 zb{0, 0, 0, 0};
        real gw0 = 0, gw1 = 0;
        if (j < W) {
          const V4 s = stash[H - 2][r];
          real d1, d2;
          const V4 in = channels_of(s, d1, d2);
          const real w0 = pH(j * NO), w1 = NO > 1 ? pH(j * NO + 1) : real(0);
          V4 ob{s0.x * w0 + s1.x * w1, s0.y * w0 + s1.y * w1, s0.z * w0 + s1.z * w1, s0.w * w0 + s1.w * w1};
          zb = preact_adjoint(s, ob);
          gw0 = dot4(in, s0);
          gw1 = dot4(in, s1);
        }
        gwacc[r][0] += gw0;
        gwacc[r][1] += gw1;
        if (j < rowsP) Bcur[j * PD + m] = zb;
        feature_add(H - 2, row + nd.off_b[H - 1], j, zb.x);      // bias gradient of layer H-1
      }
    }
    // Weight-gradient tiles of a layer: this wave's ranges in the lists of full tiles and of strips (T16Deal above)
    const int nfs = deal.edge ? ntl - 1 : ntl;                   // full tiles per side
    const int t_lo = deal.f_lo[wave], t_hi = deal.f_hi[wave], e_lo = deal.e_lo[wave], e_hi = deal.e_hi[wave];
    FSTAMP(18);
#pragma unroll
    for (int d = H - 1; d >= 1; --d) {
      __syncthreads();                        // Bcur (z_bar of layer d), TI (inputs of layer d) published
      FSTAMP(19 + 6 * (H - 1 - d));
      // ---- dW_d[k][j] += sum over the 64 (point, channel) rows: tiles tau = (rt, ct), A = TI rows k, B = z_bar rows j.
      // The row entries of the NEXT tile are requested before this tile's matrix instructions (a fetch from the
      // 63 MB of partial rows costs 2-3 k cycles, a tile's 16 matrix instructions last 1 k)
      const bool fresh = grp == (int)blockIdx.x && !accumulate;   // this workgroup's first group of the evaluation: the scratch
                                                                  // starts here (a later chunk's launch keeps adding to it)
      V4* __restrict__ gsd = reinterpret_cast<V4*>(gs + (size_t)(d - 1) * n_tiles * 256) + lane;
      // scratch slot of tile (rt, ct) = rt ntl + ct whatever list it is in: 2 KB, a strip uses the first 512 bytes
      auto fetch_old = [&](const int tau, const int slot) {
        return (tau < t_hi && !fresh) ? gsd[(size_t)slot * 64] : V4{0, 0, 0, 0};
      };
      real* __restrict__ gse = gs + (size_t)(d - 1) * n_tiles * 256 + lane;
      auto strip_rc = [&](const int e, int& rt_e, int& ct_e) {        // strip e of the list -> its tile; true: four live columns
        const bool cols = e < ntl - 1;
        rt_e = cols ? e : ntl - 1;
        ct_e = cols ? ntl - 1 : e - (ntl - 1);
        return cols;
      };
      auto fetch_old_e = [&](const int e) {
        int rt_e, ct_e;
        strip_rc(e, rt_e, ct_e);
        return (e < e_hi && !fresh) ? gse[(size_t)(rt_e * ntl + ct_e) * 256] : real(0);
      };
      real old_e = fetch_old_e(e_lo);                                 // (requested a whole tile loop ahead of its use)
      int rt = t_lo / nfs, ct = t_lo - rt * nfs;
      V4 old = fetch_old(t_lo, rt * ntl + ct);
      // (rt, ct) walk the range incrementally (a division per tile is ~40 scalar instructions); the first operands of
      // the NEXT tile are requested with the last quarter of this one, so no tile starts with an exposed LDS round trip.
      // (Tried: the old sums as the initial value of the first accumulator chain -- one vector add per entry less, but
      //  the tile's FIRST matrix instruction then waits for a fetch issued only one tile earlier: 406 -> 425 us per step.)
      const V4* __restrict__ ap = TI + (16 * rt + m) * PD + g;
      const V4* __restrict__ bq = Bcur + (16 * ct + m) * PD + g;
      V4 A = ap[0], B = bq[0];
      for (int tau = t_lo; tau < t_hi; ++tau) {
        int rtn = rt, ctn = ct + 1;
        if (ctn == nfs) { ctn = 0; ++rtn; }
        if (tau + 1 >= t_hi) { rtn = rt; ctn = ct; }               // (last tile: a harmless re-read)
        const V4 nxt = fetch_old(tau + 1, rtn * ntl + ctn);
        const V4* __restrict__ apn = TI + (16 * rtn + m) * PD + g;
        const V4* __restrict__ bqn = Bcur + (16 * ctn + m) * PD + g;
        // two accumulator chains (even / odd quarter of the 16 points) instead of one 16-deep dependent chain, and the
        // operands of quarter s4 + 1 requested before the matrix instructions of quarter s4
        acc_t acc = {0, 0, 0, 0}, acc2 = {0, 0, 0, 0};
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
          const V4 An = s4 < 3 ? ap[4 * (s4 + 1)] : apn[0], Bn = s4 < 3 ? bq[4 * (s4 + 1)] : bqn[0];
          __builtin_amdgcn_sched_barrier(0);
          acc = t16_mfma<real, acc_t>(A.x, B.x, acc);
          acc2 = t16_mfma<real, acc_t>(A.y, B.y, acc2);
          acc = t16_mfma<real, acc_t>(A.z, B.z, acc);
          acc2 = t16_mfma<real, acc_t>(A.w, B.w, acc2);
          __builtin_amdgcn_sched_barrier(0);
          A = An; B = Bn;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] += acc2[r];
        gsd[(size_t)(rt * ntl + ct) * 64] = V4{old.x + acc[0], old.y + acc[1], old.z + acc[2], old.w + acc[3]};
        old = nxt;
        rt = rtn; ct = ctn; ap = apn; bq = bqn;
      }
      // ---- strips: dW[k][j] of a tile with four live columns j (or rows k) on v_mfma_f64_4x4x4, block b = a 4-row strip of
      // the OTHER operand.  Four live columns (rt, ct = ntl-1):  A[b][i][kk] = TI[16 rt + 4 b + i][point 4 s4 + kk] -> lane
      // 16 kk + 4 b + i = the 16x16x4 fetch (row m, point g);  B[b][kk][j] = z_bar[16 ct + j][point 4 s4 + kk], the same for
      // every b -> row (m & 3);  D[b][i][j] in lane 16 i + 4 b + j = entry (k = 16 rt + 4 ((lane >> 2) & 3) + (lane >> 4),
      // j = 16 ct + (lane & 3)).  Four live rows (rt = ntl-1, ct): operands swap roles -- A row (m & 3), B row m -- and
      // D is entry (k = 16 rt + (lane >> 4), j = 16 ct + (lane & 15)), the r = 0 slot of the 16x16x4 layout.
      for (int e = e_lo; e < e_hi; ++e) {
        int rt_e, ct_e;
        const bool cols = strip_rc(e, rt_e, ct_e);
        const real nxt_e = fetch_old_e(e + 1);
        const V4* __restrict__ ape = TI + (16 * rt_e + (cols ? m : (m & 3))) * PD + g;
        const V4* __restrict__ bqe = Bcur + (16 * ct_e + (cols ? (m & 3) : m)) * PD + g;
        real sacc = 0, sacc2 = 0;
        V4 Ae = ape[0], Be = bqe[0];
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
          const V4 An = ape[s4 < 3 ? 4 * (s4 + 1) : 0], Bn = bqe[s4 < 3 ? 4 * (s4 + 1) : 0];
          __builtin_amdgcn_sched_barrier(0);
          sacc = __builtin_amdgcn_mfma_f64_4x4x4f64(Ae.x, Be.x, sacc, 0, 0, 0);
          sacc2 = __builtin_amdgcn_mfma_f64_4x4x4f64(Ae.y, Be.y, sacc2, 0, 0, 0);
          sacc = __builtin_amdgcn_mfma_f64_4x4x4f64(Ae.z, Be.z, sacc, 0, 0, 0);
          sacc2 = __builtin_amdgcn_mfma_f64_4x4x4f64(Ae.w, Be.w, sacc2, 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
          Ae = An; Be = Bn;
        }
        gse[(size_t)(rt_e * ntl + ct_e) * 256] = old_e + (sacc + sacc2);
        old_e = nxt_e;
      }
      FSTAMP(20 + 6 * (H - 1 - d));
      // ---- adjoint of layer d-1: in_bar[k][p] = sum_j W_d[k][j] z_bar[j][p] into registers -- no barrier between the
      // gradient tiles and this GEMM (both only READ the two tiles), so the waves of a SIMD drift apart and one's
      // matrix instructions run under the other's loads and stores
      FSTAMP(21 + 6 * (H - 1 - d));
      acc_t a0 = {0, 0, 0, 0}, a1 = {0, 0, 0, 0}, a2 = {0, 0, 0, 0}, a3 = {0, 0, 0, 0};
      if (tile_live) gemm(th + nd.off_w[d], Bcur, std::true_type{}, a0, a1, a2, a3);
      FSTAMP(22 + 6 * (H - 1 - d));
      __syncthreads();                        // every wave is done reading TI and Bcur: both are rewritten
      FSTAMP(23 + 6 * (H - 1 - d));
      {  // ... straight through layer d-1's tanh into TI (the next layer's z_bar)
        V4* const Bnxt = TI;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int k = own_row(r);
          V4 v{0, 0, 0, 0};
          if (k < W) {
            // layer 0 (d == 1): TI holds its OUTPUT channels, whose first is the tanh value -- this lane's own element,
            // read before it is overwritten below; the other three stash entries are weight constants
            const V4 sk = d >= 2 ? stash[d >= 2 ? d - 2 : 0][r]
                                 : V4{TI[k * PD + m].x, sx * p0(0, k), st * p0(1, k), real(0)};
            v = preact_adjoint(sk, V4{a0[r], a1[r], a2[r], a3[r]});
          }
          if (d >= 2) {
            if (k < rowsP) Bnxt[k * PD + m] = v;
            feature_add(d - 2, row + nd.off_b[d >= 2 ? d - 1 : 0], k, v.x);   // bias gradient of layer d-1
          } else {
            // dense 0: inputs (hx, ht), p0 = (sx, 0), q0 = (0, st); its z_bar goes nowhere else -- not written to the tile
            const real hxm = hxy[m], htm = hxy[16 + m];
            feature_add(H - 1, row + nd.off_w[0], k, hxm * v.x + sx * v.y);
            feature_add(H, row + nd.off_w[0] + W, k, htm * v.x + st * v.z);
            feature_add(H + 1, row + nd.off_b[0], k, v.x);
          }
        }
      }
      if (d >= 2) {                           // inputs of layer d-1 = output channels of layer d-2
        if (d >= 3) {                         // ... from the owning lanes' registers
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int j = own_row(r);
            V4 c{0, 0, 0, 0};
            if (j < W) { real d1, d2; c = channels_of(stash[d >= 3 ? d - 3 : 0][r], d1, d2); }
            if (j < rowsP) Bcur[j * PD + m] = c;
          }
        } else {                              // ... layer 0: recomputed, items (feature j, point pe)
#pragma unroll
          for (int i = 0; i < NI; ++i) {
            const int j = (tid >> 4) + RP * i;
            V4 c{0, 0, 0, 0};
            if (j < W) {
              real d1, d2;
              c = channels_of(V4{a0e[i], sx * p0(0, j), st * p0(1, j), real(0)}, d1, d2);
            }
            if (j < rowsP) Bcur[j * PD + pe] = c;
          }
        }
      }
      FSTAMP(24 + 6 * (H - 1 - d));
      V4* tmp = Bcur; Bcur = TI; TI = tmp;     // roles swap: the old TI holds z_bar, the old Bcur the inputs
    }
    FSTAMP(41);
    __syncthreads();                          // seeds / hxy / tiles are rewritten by the next group; gsm published
    FSTAMP(42);
  }
  KSTAMP(62);
  __syncthreads();                            // (gsm zeroed / accumulated by other lanes than the ones that copy it out)
  auto put = [&](real* __restrict__ dst, const real v) {
    if (direct) *dst = v; else *dst += v;
  };
  {  // the on-chip sums -> the partial row
    const int lane = tid0 & 63, m = lane & 15;
#pragma unroll
    for (int r = 0; r < 4; ++r) {             // output-layer weights: this lane's rows, summed over the 16 points
      const int j = r < ns ? row0 + TR::out_row(lane, r) : (1 << 20);
      const real g0 = row16_sum(gwacc[r][0]), g1 = row16_sum(gwacc[r][1]);
      if (m == 0 && j < W) {
        put(row + nd.off_w[H] + j * NO, g0);
        if (NO > 1) put(row + nd.off_w[H] + j * NO + 1, g1);
      }
    }
    if (small_lds && tid0 < W) {
#pragma unroll
      for (int d = 1; d < H; ++d) put(row + nd.off_b[d] + tid0, gsm[(d - 1) * W + tid0]);
      put(row + nd.off_w[0] + tid0, gsm[(H - 1) * W + tid0]);
      put(row + nd.off_w[0] + W + tid0, gsm[H * W + tid0]);
      put(row + nd.off_b[0] + tid0, gsm[(H + 1) * W + tid0]);
    }
  }
  // (the hidden-layer weight gradients STAY in the tile-major scratch: the reduction kernels read them there --
  //  kernels_optim.h TileScratch; their entries of the partial row are never written and never read)
  if (tid0 < 16) {   // loss parts, lambda gradients, output biases: sums over this workgroup's points
    real l_acc[3], dl_acc[2], gb_acc[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) l_acc[k] = sum16(lsum[16 * k + tid0]);
    dl_acc[0] = sum16(lsum[48 + tid0]); dl_acc[1] = sum16(lsum[64 + tid0]);
    gb_acc[0] = sum16(lsum[80 + tid0]); gb_acc[1] = sum16(lsum[96 + tid0]);
    if (tid0 == 0) {
      put(row + nd.n_theta + 0, l_acc[0]); put(row + nd.n_theta + 1, l_acc[1]); put(row + nd.n_theta + 2, l_acc[2]);
      for (int i = nd.n_theta + 3; direct && i < R; ++i) row[i] = real(0);       // (padding of the row)
      put(row + nd.off_b[H], gb_acc[0]);
      if (NO > 1) put(row + nd.off_b[H] + 1, gb_acc[1]);
      if (PDE == 1) { put(row + nd.n_net, dl_acc[0]); put(row + nd.n_net + 1, dl_acc[1]); }
    }
  }
  KSTAMP(63);
}

}  // namespace pinn
