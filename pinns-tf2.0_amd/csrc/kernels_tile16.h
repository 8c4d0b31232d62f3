// kernels_tile16.h -- shape-generic MFMA sweeps for the continuous models: any uniform hidden width up to 128
// (64 in float64), any depth, 1-2 outputs, all three residual kinds, float32 and float64 -- the fast path for every
// network the width-20 / width-100 kernels do not serve (until now those shapes ran on the one-lane-per-point
// VALU kernels of kernels_generic.h at ~1 TFLOP/s).
//
// Mapping (the same as kernels_wide.h, with runtime width/depth and a compile-time tile count NT = ceil(W/16)):
//   workgroup = 4 waves = one group of 16 points at a time, persistent over groups;
//   every layer is  Z[feature][point] = W^T[feature][k] . IN[k][point]  on v_mfma_{f32,f64}_16x16x4: the A operand
//   is the weight tile (features on the M side), the B operand the exchange tile, so the accumulator register r of
//   lane (n = point, g) is feature out_row(lane, r) of point n: the four Taylor channels of a (feature, point) sit
//   in one lane (tanh chain lane-local) and stash / exchange-tile accesses run along the points (coalesced);
//   exchange tiles are [feature][17] vec4 (value, d/dx, d/dt, d2/dx2): one LDS read serves the four channel MFMAs;
//   weights of the layer in flight live in LDS, fetched one layer ahead through registers (as in kernels_disc.h);
//   stash S and outputs O use the generic kernels' layout, so either half can be paired with k_forward/k_backward
//   (which is how the tests pin each half);
//   weight gradients: NT x NT tiles x 16 MFMAs per layer and group, *added* into the workgroup's own partial row
//   (read-modify-write in L2/HBM: at most 2 P sizeof(real) bytes per group against 24 M_w x 16 FLOP, < 10 % of the
//   time at every shape) -- no register-resident accumulators, so the kernel has room for float64 and for two
//   workgroups per CU.
// Math: SURVEY.md Appendix A (channels_of / preact_adjoint / point_seeds of kernels_generic.h).
#pragma once
#include "kernels_disc.h"
#include "kernels_fused20d.h"

namespace pinn {

// (Ablation builds -- one ingredient compiled out at a time, wrong results by construction, only times are read -- are not part
// of the product sources since round 5.  profiles/ablation_scaffolding.patch holds the -DPINN_ABL / -DPINN_ABLD / -DT16_ABL
// switches of profiles/ablate_*.py; it is not kept up with these sources: it reverse-applies to the tree at ee3788e; check that
// commit out for the ablation builds.  Their results are under profiles/*ablate*.txt.)

// T16_AHEAD 1: the eight-wave reverse sweep fetches the row entries of all its dW tiles, and the next layer's stash, ahead of
// the matrix instructions -- measured 8 us SLOWER on cfg 4 float64 (605 vs 597 us, same box, profiles/r03_t16_ab.txt): with
// two waves per SIMD the other wave already covers those latencies and the extra live registers cost more.  The switch stays
// although it is settled: its single-trip `ti` loop around k_t16_bwd's tile loop shapes the code hipcc generates -- flattened,
// all 18 k_t16_bwd instantiations change (+2..35 instructions, +2 VGPRs, 20 B of scratch in two;
// profiles/retire_switches_device_code.txt).
#ifndef T16_AHEAD
#define T16_AHEAD 0
#endif

// Tried and dropped (the arms were in the sources up to 7a77e26, profiles/retire_switches_device_code.txt):
//   four waves per workgroup for the float64 sweeps above width 64 (the round-2 kernels) instead of eight
//     (profiles/r03_ablate_t16_f64_w8.txt)
//   the eight-wave reverse sweep fetching the row entries of a fresh row's first group, which are the zeros this workgroup
//     has just written
//   LDS operands of the layer GEMMs requested two k-steps ahead instead of one: 254-256 VGPRs in k_t16_fused and 1.5 %
//     SLOWER there (same box, cfg 4 float64 410.5 vs 417.3 us per step), within +-0.5 % on the two-kernel sweeps
//   the four-wave variants (widths <= 64) on hand-written chunk loops (weights fetched one chunk of four k-steps ahead,
//     two chunks in the eight-wave variants: 583 vs 605 us on cfg 4 float64, profiles/r03_t16_ab.txt, r03_t16_depth.txt) and
//     one-chain gradient tiles instead of t16_gemm_l2 / the two-chain tiles: same-box A/B (profiles/r04_t16_gemm4_ab.txt)
//     2x50^4x1 f64 142.5 -> 130.5 us, f32 80.9 -> 74.5; 2x64^6x1 f64 241.8 -> 229.5; register counts keep the launch
//     plan's workgroups per CU (f32 forward 112 VGPRs: occupancy 3 -> 4)

// tanh of the MFMA sweeps.  float64: the library tanh() is several hundred instructions with branches -- at width 100
// a lane evaluates 8 of them per layer behind 12.8 k cycles of matrix instructions, on a SIMD that holds one wave, so
// they were a third of the forward sweep (cfg 4 float64: 286 us -> profiles/r03_time_cfg4.txt); tanh_d is the
// exp + Newton-quotient form of k_fused20d (relative error < 1e-16 before the final rounding).  float32 keeps tanhf.
template <typename real> __device__ __forceinline__ real tanh_mm(real z);
template <> __device__ __forceinline__ float tanh_mm<float>(float z) { return tanhf(z); }
template <> __device__ __forceinline__ double tanh_mm<double>(double z) {
  return tanh_d(z);
}
template <typename real, typename acc_t>
__device__ __forceinline__ acc_t t16_mfma(real a, real b, acc_t c) {
  return FusedTraits<real>::mfma(a, b, c);
}

template <int NT> struct T16Geo {
  static constexpr int WP = 16 * NT;
  static constexpr int PD = 17;                // exchange tile row pitch in vec4 (16 points + 1 pad)
  static constexpr int TILE = WP * PD;         // vec4 per exchange tile
  static constexpr int WLD = WP + 16;          // weights [k][j] read as A[m = j][4s+g = k]: rows 4s+g, cols m
  static constexpr int TLD = WP + 4;           // weights [k][j] read as A[m = k][4s+g = j]
  static constexpr int NPRE = WP * WP / 256;
};
template <int NT> inline size_t t16_fwd_lds(size_t rs, bool wlds, int nwv = 4) {
  return (size_t)(2 * T16Geo<NT>::TILE * 4 + (wlds ? T16Geo<NT>::WP * T16Geo<NT>::WLD : 0) + 2 * nwv * 2 * 16 * 4) * rs;
}
template <int NT> inline size_t t16_bwd_lds(size_t rs, bool wlds) {
  return (size_t)(2 * T16Geo<NT>::TILE * 4 + (wlds ? T16Geo<NT>::WP * T16Geo<NT>::TLD : 0) + 2 * 16 * 4 + 32) * rs;
}

template <typename real>
__device__ __forceinline__ real sum16(real v) {        // sum over the 16 lanes of a DPP row; every lane gets it
  v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4); v += __shfl_xor(v, 8);
  return v;
}

// Matrix instructions of one k-step of a layer GEMM: weight `w` (this lane's A operand in the 16x16x4 pattern: row
// row0 + (lane & 15), k-step row lane >> 4) times the four channels of `b`.
//   STRIPS = false: the wave owns a 16-row tile, one v_mfma_f64_16x16x4 per channel (64 cycles each).
//   STRIPS = true (float64 only, round 5): the wave owns ns <= 3 STRIPS of four rows, rows row0 + 4 r + (0..3); strip r runs
//   on v_mfma_f64_4x4x4 (four independent 4x4x4 blocks, 16 cycles, the same FLOP per cycle:
//   profiles/r02_ubench_mfma_f64_4x4x4.txt) with block b = points 4b..4b+3:
//     A[b][i][k]: lane 16 k + 4 b + i -> weight of (row 4 r + i, k-step row k), the same for every b: quad r of the lane's
//                 16-lane row, broadcast to its four quads by one ds_swizzle (bit mode: lane' = (lane & 0x13) | 4 r);
//     B[b][k][j]: lane 16 k + 4 b + j -> (B row 4 s + k, point 4 b + j): exactly the 16x16x4 operand fetch (row g, point m);
//     D[b][i][j]: lane 16 i + 4 b + j -> (row 4 r + (lane >> 4), point lane & 15): entry r of the 16x16x4 result layout
//                 (row g + 4 r, point m) -- so everything downstream of the GEMM is the same code for both kinds of wave.
//   Width 100 = 25 strips: waves 0-3 keep a 16-row tile, waves 4-7 take 2, 2, 2, 3 strips (T16Deal).
template <int R>
__device__ __forceinline__ double t16_quad_bcast(const double x) {
  // value of lane (lane & 0x33) | (R << 2): ds_swizzle_b32 in bit mode works inside each half of 32 lanes, offset =
  // 0x8000 would be the quad mode; bit mode: and_mask[4:0] | or_mask[9:5] | xor_mask[14:10]
  constexpr int pattern = 0x13 | ((R << 2) << 5);
  const int lo = __builtin_amdgcn_ds_swizzle(__double2loint(x), pattern);
  const int hi = __builtin_amdgcn_ds_swizzle(__double2hiint(x), pattern);
  return __hiloint2double(hi, lo);
}

// ws: the strips' operands of THIS k-step, already broadcast; wn: the weight of the NEXT k-step -- each strip's operand is
// re-broadcast IN PLACE right behind the four matrix instructions that read it, so a swizzle travels while the other
// strips' instructions occupy the pipe (with the ds_swizzle in FRONT of its matrix instructions, or all of them behind the
// k-step next to the LDS reads of the one after -- one s_waitcnt lgkmcnt(0) for both -- a two-strip GEMM took 16 k cycles
// for 3.3 k of matrix time: profiles/r05_t16f_stamps_edge_v4.txt, _v5.txt)
template <typename real, bool STRIPS, typename acc_t>
__device__ __forceinline__ void t16_mma_kstep(const real w, real (&ws)[3], const real wn, const vec4<real>& b, const int ns,
                                              acc_t& a0, acc_t& a1, acc_t& a2, acc_t& a3) {
  if constexpr (STRIPS) {
    static_assert(sizeof(real) == 8, "strips are float64 only");
    a0[0] = __builtin_amdgcn_mfma_f64_4x4x4f64(ws[0], b.x, a0[0], 0, 0, 0);
    a1[0] = __builtin_amdgcn_mfma_f64_4x4x4f64(ws[0], b.y, a1[0], 0, 0, 0);
    a2[0] = __builtin_amdgcn_mfma_f64_4x4x4f64(ws[0], b.z, a2[0], 0, 0, 0);
    a3[0] = __builtin_amdgcn_mfma_f64_4x4x4f64(ws[0], b.w, a3[0], 0, 0, 0);
    ws[0] = t16_quad_bcast<0>(wn);
    if (ns > 1) {                              // (wave-uniform)
      a0[1] = __builtin_amdgcn_mfma_f64_4x4x4f64(ws[1], b.x, a0[1], 0, 0, 0);
      a1[1] = __builtin_amdgcn_mfma_f64_4x4x4f64(ws[1], b.y, a1[1], 0, 0, 0);
      a2[1] = __builtin_amdgcn_mfma_f64_4x4x4f64(ws[1], b.z, a2[1], 0, 0, 0);
      a3[1] = __builtin_amdgcn_mfma_f64_4x4x4f64(ws[1], b.w, a3[1], 0, 0, 0);
      ws[1] = t16_quad_bcast<1>(wn);
    }
    if (ns > 2) {
      a0[2] = __builtin_amdgcn_mfma_f64_4x4x4f64(ws[2], b.x, a0[2], 0, 0, 0);
      a1[2] = __builtin_amdgcn_mfma_f64_4x4x4f64(ws[2], b.y, a1[2], 0, 0, 0);
      a2[2] = __builtin_amdgcn_mfma_f64_4x4x4f64(ws[2], b.z, a2[2], 0, 0, 0);
      a3[2] = __builtin_amdgcn_mfma_f64_4x4x4f64(ws[2], b.w, a3[2], 0, 0, 0);
      ws[2] = t16_quad_bcast<2>(wn);
    }
  } else {
    a0 = t16_mfma<real, acc_t>(w, b.x, a0);
    a1 = t16_mfma<real, acc_t>(w, b.y, a1);
    a2 = t16_mfma<real, acc_t>(w, b.z, a2);
    a3 = t16_mfma<real, acc_t>(w, b.w, a3);
  }
}

// One layer GEMM of a 16-row feature tile (or of ns strips of it, STRIPS) with the weights read straight from L2 (round 4;
// the eight-wave sweeps and k_t16_fused):  acc_c[r] += sum_k A(row, k) B_c[k][point m],  A(row, k) = Wm[row * W + k] if
// TRANSPOSED (adjoint GEMM) else Wm[k * W + row] (forward GEMM); `ra` = this lane's row (row0 + m), B rows are vec4 (four
// Taylor channels).
//  * k-steps whose four rows k = 4 s + g all exist (s < W / 4) run UNGUARDED in chunks of four: plain loads (a padded
//    output row ra >= W reads row W - 1; its results are discarded by the caller), three weight buffers in rotation --
//    the loop is unrolled by three, no register copies, and the wait before a chunk is for loads issued two chunks
//    earlier.  (Guarded loads compile to a predicated branch each, 8 instructions, and make every k-step its own basic
//    block whose ds_read is waited for right before its four matrix instructions.)
//  * the B operands of k-step s + 1 are requested from LDS BEFORE the matrix instructions of k-step s (sched_barrier
//    pins it);
//  * at most three unguarded and one guarded (W % 4 != 0) k-step remain for the tail.
template <typename real, bool TRANSPOSED, int PD, typename acc_t, bool STRIPS = false>
__device__ __forceinline__ void t16_gemm_l2(const real* __restrict__ Wm, const vec4<real>* __restrict__ Bt, const int W,
                                            const int ra, const int m, const int g, acc_t& a0, acc_t& a1, acc_t& a2,
                                            acc_t& a3, const int ns = 4) {
  using V4 = vec4<real>;
  const int ksteps = (W + 3) >> 2, kfull = W >> 2, nfc = kfull >> 2;   // k-steps; unguarded ones; full chunks of four
  const int rac = ra < W ? ra : W - 1;
  const int kstr = TRANSPOSED ? 4 : 4 * W;                        // elements per k-step
  const real* __restrict__ wp = Wm + (TRANSPOSED ? rac * W + g : g * W + rac);
  const V4* __restrict__ bp = Bt + g * PD + m;                    // B rows 4 s + g, point m: + 4 PD per k-step
  auto fetch = [&](int c, real (&dst)[4]) {                       // chunk c (clamped: a fetch beyond the last chunk re-reads it)
    const int cc = c < nfc ? c : (nfc > 0 ? nfc - 1 : 0);
#pragma unroll
    for (int u = 0; u < 4; ++u) dst[u] = wp[(4 * cc + u) * kstr];
  };
  real w0[4], w1[4], w2[4];
  if (nfc > 0) { fetch(0, w0); fetch(1, w1); }
  V4 bc = bp[0];
  real ws[3] = {0, 0, 0};                                         // STRIPS: the current k-step's weights, one per strip
  auto spread = [&](const real w, real (&dst)[3]) {
    if constexpr (STRIPS) { dst[0] = t16_quad_bcast<0>(w); dst[1] = t16_quad_bcast<1>(w); dst[2] = t16_quad_bcast<2>(w); }
  };
  if (nfc > 0) spread(w0[0], ws);
  auto chunk = [&](const int c, real (&cur)[4], real (&nxt)[4], real (&fill)[4]) {
    fetch(c + 2, fill);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const V4 bn = bp[(4 * c + u + 1) * 4 * PD];                 // next k-step's rows (always inside the tile)
      __builtin_amdgcn_sched_barrier(0);
      t16_mma_kstep<real, STRIPS>(cur[u], ws, u < 3 ? cur[u + 1] : nxt[0], bc, ns, a0, a1, a2, a3);   // (after the last chunk: a harmless re-read)
      __builtin_amdgcn_sched_barrier(0);
      bc = bn;
    }
  };
  for (int c = 0; c < nfc; c += 3) {
    chunk(c, w0, w1, w2);
    if (c + 1 < nfc) chunk(c + 1, w1, w2, w0);
    if (c + 2 < nfc) chunk(c + 2, w2, w0, w1);
  }
  for (int ks = 4 * nfc; ks < ksteps; ++ks) {                     // tail: <= 3 unguarded k-steps + one guarded
    const int k = 4 * ks + g;
    const real a = k < W ? wp[(k < W ? ks : 0) * kstr] : real(0);
    const V4 b = bp[ks * 4 * PD];
    spread(a, ws);
    t16_mma_kstep<real, STRIPS>(a, ws, a, b, ns, a0, a1, a2, a3);
  }
}

// ---------------------------------------------------------------------------------------------------------
// forward sweep over points [base, base + 16 n_groups): fills S and O exactly as k_forward does
// ---------------------------------------------------------------------------------------------------------
// NWV = waves per workgroup: 4 (one per SIMD), or 8 for the widths whose two exchange tiles leave room for ONE
// workgroup per CU (float64 above width 64): the group's tiles are then dealt to eight waves, two per SIMD, and one
// wave's matrix instructions run under the other's loads, address arithmetic and tanh chain.  (SQ counters of the
// 4-wave float64 width-100 sweeps, profiles/r03_pmc_cfg4_f64.txt: matrix pipe busy 39 % / 28 % of the wave cycles,
// the rest issue of other instructions and s_waitcnt -- nothing overlapped with one wave per SIMD.)
template <typename real, int NT, bool WLDS, int NWV = 4>
__global__ __launch_bounds__(64 * NWV) void k_t16_fwd(NetDesc nd, const real* __restrict__ th,
                                                 const real* __restrict__ xs, const real* __restrict__ ts, int base,
                                                 int n_pad, int s_pad, int n_groups, real lbx, real lbt, real sx,
                                                 real st, vec4<real>* __restrict__ S, vec4<real>* __restrict__ O) {
  using TR = FusedTraits<real>;
  using acc_t = typename TR::acc_t;
  using GEO = T16Geo<NT>;
  using V4 = vec4<real>;
  constexpr int WP = GEO::WP, PD = GEO::PD, WLD = GEO::WLD;
  extern __shared__ __attribute__((aligned(16))) char t16_smem[];
  V4* const T0 = reinterpret_cast<V4*>(t16_smem);
  V4* const T1 = T0 + GEO::TILE;
  real* const wb = reinterpret_cast<real*>(T1 + GEO::TILE);      // [WP][WLD] (WLDS only; else weights come from L2)
  real* const red = wb + (WLDS ? WP * WLD : 0);                   // [2 NWV][2][16][4] output-layer partials
  static_assert(NWV == 4 || !WLDS, "the LDS weight staging is written for 256 threads");
  constexpr int RP = 4 * NWV;                                     // feature rows per elementwise pass (threads / 16)
  constexpr int NI = WP / RP;                                     // passes over the padded width
  constexpr int KS = 2 * NWV;                                     // k-slices of the output layer (threads / 32)
  constexpr int NKO = WP / KS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int W = nd.width, H = nd.n_hidden, NO = nd.n_out;
  const int m = lane & 15, g = lane >> 4;
  const int ksteps = (W + 3) / 4;
  const int pe = tid & 15;                                        // the point of this thread's elementwise items

  real pre[GEO::NPRE];                        // (dead when !WLDS)
  if constexpr (WLDS) { if (H > 1) wt_load<real, NT, WP>(pre, th + nd.off_w[1], W, W, W, tid); }
  // parameters that every group reuses: dense 0 of this thread's features, the output layer's k-slice
  real p0x[NI], p0t[NI], p0b[NI], pout[NKO];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int j = (tid >> 4) + RP * i;
    p0x[i] = j < W ? th[nd.off_w[0] + j] : real(0);
    p0t[i] = j < W ? th[nd.off_w[0] + W + j] : real(0);
    p0b[i] = j < W ? th[nd.off_b[0] + j] : real(0);
  }
#pragma unroll
  for (int i = 0; i < NKO; ++i) {
    const int k = (tid >> 5) + KS * i, o = (tid >> 4) & 1;
    pout[i] = (k < W && o < NO) ? th[nd.off_w[H] + k * NO + o] : real(0);
  }

  for (int grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
    const int lp0 = grp * 16;
    {  // dense 0: items (feature j, point pe), point fastest
      const real x = xs[base + lp0 + pe], t = ts[base + lp0 + pe];
      const real hx = sx * (x - lbx) - real(1), ht = st * (t - lbt) - real(1);
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const int j = (tid >> 4) + RP * i;
        V4 s{0, 0, 0, 0}, c{0, 0, 0, 0};
        if (j < W) {
          const real w0 = p0x[i], w1 = p0t[i], b0 = p0b[i];
          s = V4{tanh_mm(hx * w0 + ht * w1 + b0), sx * w0, st * w1, real(0)};
          S[(size_t)j * s_pad + lp0 + pe] = s;
          real d1, d2;
          c = channels_of(s, d1, d2);
        }
        T0[j * PD + pe] = c;
      }
    }
    V4* Tin = T0;
    V4* Tout = T1;
    for (int l = 1; l < H; ++l) {
      __syncthreads();                        // Tin published; nobody reads wb any more
      if constexpr (WLDS) {
        wt_store<real, NT, WP>(pre, wb, WLD, tid);
        __syncthreads();
        const int ln = l + 1 < H ? l + 1 : 1;  // next matrix on its way: W_{l+1}, or W_1 for the next group
        wt_load<real, NT, WP>(pre, th + nd.off_w[ln], W, W, W, tid);
      }
      const real* __restrict__ bl = th + nd.off_b[l];
      const real* __restrict__ Wl = th + nd.off_w[l];
      for (int ct = wave; ct < NT; ct += NWV) {
        if (16 * ct >= W) {                                       // tile entirely in the padding (wave-uniform): zeros
#pragma unroll
          for (int r = 0; r < 4; ++r) Tout[(16 * ct + TR::out_row(lane, r)) * PD + m] = V4{0, 0, 0, 0};
          continue;
        }
        real bj[4];                                               // biases of this lane's four features (in flight
#pragma unroll                                                    //  under the MFMAs)
        for (int r = 0; r < 4; ++r) {
          const int j = 16 * ct + TR::out_row(lane, r);
          bj[r] = j < W ? bl[j] : real(0);
        }
        acc_t a0 = {0, 0, 0, 0}, a1 = {0, 0, 0, 0}, a2 = {0, 0, 0, 0}, a3 = {0, 0, 0, 0};
        const int ja = 16 * ct + m;                               // A[m = feature 16ct+m][k]
        if constexpr (WLDS) {
#pragma unroll 4
          for (int ks = 0; ks < ksteps; ++ks) {
            const int k = 4 * ks + g;
            const real a = wb[k * WLD + ja];
            const V4 b = Tin[k * PD + m];                         // B[k][n = point m]
            a0 = t16_mfma<real, acc_t>(a, b.x, a0);
            a1 = t16_mfma<real, acc_t>(a, b.y, a1);
            a2 = t16_mfma<real, acc_t>(a, b.z, a2);
            a3 = t16_mfma<real, acc_t>(a, b.w, a3);
          }
        } else {
          t16_gemm_l2<real, false, PD, acc_t>(Wl, Tin, W, ja, m, g, a0, a1, a2, a3);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int j = 16 * ct + TR::out_row(lane, r);           // feature; the point is m
          V4 c{0, 0, 0, 0};
          if (j < W) {
            const V4 s{tanh_mm(a0[r] + bj[r]), a1[r], a2[r], a3[r]};
            S[((size_t)l * W + j) * s_pad + lp0 + m] = s;
            real d1, d2;
            c = channels_of(s, d1, d2);
          }
          Tout[j * PD + m] = c;
        }
      }
      V4* tmp = Tin; Tin = Tout; Tout = tmp;
    }
    __syncthreads();
    {  // linear output layer: thread = (k-slice ks8, output o, point pe); the slices are summed through LDS
      const int o = (tid >> 4) & 1, ks8 = tid >> 5;
      V4 acc{0, 0, 0, 0};
#pragma unroll
      for (int i = 0; i < NKO; ++i) {
        const int k = ks8 + KS * i;               // pout is zero beyond the width / the outputs
        const V4 b = Tin[k * PD + pe];
        const real w = pout[i];
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
        tot.x += th[nd.off_b[H] + o];
        O[(size_t)o * n_pad + base + lp0 + pe] = tot;
      }
    }
    __syncthreads();                          // the next group's dense 0 overwrites T0
  }
}

// ---------------------------------------------------------------------------------------------------------
// reverse sweep over points [base, base + 16 n_groups), consuming S and O: seeds, adjoints through every layer,
// all weight gradients added into one partial row per workgroup (zeroed here unless `accumulate`).
// WLDS: the layer's weight matrix is staged in LDS for the adjoint GEMM (else read from global / L2).
// ---------------------------------------------------------------------------------------------------------
template <typename real, int NT, int PDE, bool WLDS, int NWV = 4>
__global__ __launch_bounds__(64 * NWV) void k_t16_bwd(NetDesc nd, SetDesc sd, const real* __restrict__ th,
                                                 const real* __restrict__ xs, const real* __restrict__ ts,
                                                 const real* __restrict__ tgt, int base, int n_pad, int s_pad,
                                                 int n_groups, real lbx, real lbt, real sx, real st, real nu,
                                                 const vec4<real>* __restrict__ S, const vec4<real>* __restrict__ O,
                                                 real* __restrict__ part, int R, int accumulate) {
  using TR = FusedTraits<real>;
  using acc_t = typename TR::acc_t;
  using GEO = T16Geo<NT>;
  using V4 = vec4<real>;
  constexpr int WP = GEO::WP, PD = GEO::PD, TLD = GEO::TLD;
  extern __shared__ __attribute__((aligned(16))) char t16_smem[];
  // two exchange tiles that swap roles every layer: X = inputs of the layer being reversed (A operand of dW), then
  // overwritten by the adjoint of the layer below; Y = adjoint of this layer's pre-activations, then refilled with
  // the inputs of the layer below
  V4* const TA = reinterpret_cast<V4*>(t16_smem);
  V4* const TB = TA + GEO::TILE;
  real* const wt = reinterpret_cast<real*>(TB + GEO::TILE);       // [WP][TLD] (WLDS only)
  V4* const seeds = reinterpret_cast<V4*>(wt + (WLDS ? WP * TLD : 0));   // [2][16]
  real* const hxy = reinterpret_cast<real*>(seeds + 32);          // [2][16] normalised inputs
  static_assert(NWV == 4 || !WLDS, "the LDS weight staging is written for 256 threads");
  constexpr int RP = 4 * NWV, THREADS = 64 * NWV;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int W = nd.width, H = nd.n_hidden, NO = nd.n_out;
  const int m = lane & 15, g = lane >> 4, pe = tid & 15;
  const int ksteps = (W + 3) / 4;
  real* __restrict__ row = part + (size_t)blockIdx.x * R;
  real c1 = real(1), c2 = nu;
  if (PDE == 1) { c1 = th[nd.n_net]; c2 = exp_r(th[nd.n_net + 1]); }

  if (!accumulate) {
    for (int i = tid; i < R; i += THREADS) row[i] = real(0);
    __syncthreads();                          // (global stores of one workgroup, read back by the same workgroup)
  }
  real l_acc[3] = {0, 0, 0}, dl_acc[2] = {0, 0}, gb_acc[2] = {0, 0};   // threads 0..15: one point each

  real pre[GEO::NPRE];                        // (dead when !WLDS)
  if constexpr (WLDS) { if (H > 1) wt_load<real, NT, WP>(pre, th + nd.off_w[H - 1], W, W, W, tid); }

  for (int grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
    const int lp0 = grp * 16;
    if (tid < 16) {
      const int pt = base + lp0 + tid;
      V4 sb[2];
      real lt[3], dl[2];
      point_seeds<real, PDE>(sd, pt, n_pad, O, tgt, c1, c2, sb, lt, dl);
      seeds[tid] = sb[0]; seeds[16 + tid] = sb[1];
      l_acc[0] += lt[0]; l_acc[1] += lt[1]; l_acc[2] += lt[2];
      dl_acc[0] += dl[0]; dl_acc[1] += dl[1];
      gb_acc[0] += sb[0].x; gb_acc[1] += sb[1].x;
      hxy[tid] = sx * (xs[pt] - lbx) - real(1);
      hxy[16 + tid] = st * (ts[pt] - lbt) - real(1);
    }
    __syncthreads();
    V4* TI = TA;                              // inputs of the layer being reversed
    V4* Bcur = TB;                            // adjoint of its pre-activations
    {  // dense H (linear): z_bar = seeds.  Items (feature j, point pe): adjoint of layer H-1's pre-activations,
       // gradient of the output weights (sum over the 16 points = the 16 lanes of a DPP row), inputs of layer H-1
      const V4 s0 = seeds[pe], s1 = seeds[16 + pe];
      for (int j = tid >> 4; j < WP; j += RP) {
        V4 zb{0, 0, 0, 0};
        real gw0 = 0, gw1 = 0;
        if (j < W) {
          const V4 s = S[((size_t)(H - 1) * W + j) * s_pad + lp0 + pe];
          real d1, d2;
          const V4 in = channels_of(s, d1, d2);
          const real w0 = th[nd.off_w[H] + j * NO], w1 = NO > 1 ? th[nd.off_w[H] + j * NO + 1] : real(0);
          V4 ob{s0.x * w0 + s1.x * w1, s0.y * w0 + s1.y * w1, s0.z * w0 + s1.z * w1, s0.w * w0 + s1.w * w1};
          zb = preact_adjoint(s, ob);
          gw0 = dot4(in, s0);
          gw1 = dot4(in, s1);
        }
        Bcur[j * PD + pe] = zb;
        gw0 = sum16(gw0);
        gw1 = sum16(gw1);
        if (pe == 0 && j < W) {
          row[nd.off_w[H] + j * NO] += gw0;
          if (NO > 1) row[nd.off_w[H] + j * NO + 1] += gw1;
        }
        if (H > 1) {
          V4 c{0, 0, 0, 0};
          if (j < W) {
            real d1, d2;
            c = channels_of(S[((size_t)(H - 2) * W + j) * s_pad + lp0 + pe], d1, d2);
          }
          TI[j * PD + pe] = c;
        }
      }
    }
    for (int d = H - 1; d >= 1; --d) {
      if constexpr (WLDS) wt_store<real, NT, WP>(pre, wt, TLD, tid);
      __syncthreads();                        // Bcur (z_bar of layer d), TI (inputs of layer d), weights published
      if constexpr (WLDS) {                   // next matrix: W_{d-1}, or W_{H-1} for the next group
        const int dn = d >= 2 ? d - 1 : H - 1;
        wt_load<real, NT, WP>(pre, th + nd.off_w[dn], W, W, W, tid);
      }
      // ---- dW_d[k][j] += sum over the 64 (point, channel) rows: tiles tau = (rt, ct), A = TI rows k, B = z_bar rows j
      const int ntl = (W + 15) >> 4;                              // live tiles per side: the others are padding
      // The row entries a tile updates are fetched for ALL of this wave's tiles before its first matrix instruction
      // (MAXT x 4 registers): the partial rows of 256 workgroups do not fit the L2s, a fetch costs 2-3 k cycles and a
      // tile's 16 matrix instructions last 1 k, so fetching per tile stalled every tile (ablation, float64 width 100,
      // profiles/r03_ablate_t16_f64.txt: the read-modify-write was 83 of 434 us).  Same thread reads and writes an
      // entry, group after group: program order keeps the accumulation exact.
      constexpr int MAXT = (NT * NT + NWV - 1) / NWV;
      constexpr bool AHEAD = NWV == 8 && T16_AHEAD;   // (the four-wave variants keep the per-tile fetch: they were tuned, and
                                              //  are launched, for two or three workgroups per CU at their register count)
      real oldv[AHEAD ? MAXT : 1][4];
      if constexpr (AHEAD) {
#pragma unroll
        for (int ti = 0; ti < MAXT; ++ti) {
          const int tau = wave + ti * NWV;
          const int rt = tau / ntl, ct = tau - rt * ntl, j = 16 * ct + m;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int k = 16 * rt + TR::out_row(lane, r);
            oldv[ti][r] = (tau < ntl * ntl && k < W && j < W) ? row[nd.off_w[d] + k * W + j] : real(0);
          }
        }
      }
#pragma unroll
      for (int ti = 0; ti < (AHEAD ? MAXT : 1); ++ti)
      for (int tau = wave + ti * NWV; tau < ntl * ntl; tau += (AHEAD ? NT * NT * NWV : NWV)) {   // AHEAD: one tile per ti
        const int rt = tau / ntl, ct = tau - rt * ntl;
        const int j = 16 * ct + m;
        real old[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int k = 16 * rt + TR::out_row(lane, r);
          if constexpr (AHEAD) old[r] = oldv[ti][r];
          else {
            // the first group of a fresh row adds to the zeros this workgroup has just written: nothing to fetch
            // (eight-wave variants; one fifth of the row reads at five groups per workgroup)
            old[r] = (k < W && j < W && !(NWV == 8 && !accumulate && grp == (int)blockIdx.x))
                         ? row[nd.off_w[d] + k * W + j] : real(0);
          }
        }
        acc_t acc = {0, 0, 0, 0};
        {
          // (round 4, as k_t16_fused) two accumulator chains instead of one 16-deep dependent chain, and the operands
          // of quarter s4 + 1 requested from LDS before the matrix instructions of quarter s4
          acc_t acc2 = {0, 0, 0, 0};
          const V4* __restrict__ ap = TI + (16 * rt + m) * PD + g;
          const V4* __restrict__ bq = Bcur + (16 * ct + m) * PD + g;
          V4 A = ap[0], B = bq[0];
#pragma unroll
          for (int s4 = 0; s4 < 4; ++s4) {
            const V4 An = ap[s4 < 3 ? 4 * (s4 + 1) : 0], Bn = bq[s4 < 3 ? 4 * (s4 + 1) : 0];
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
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int k = 16 * rt + TR::out_row(lane, r);
          if (k < W && j < W) row[nd.off_w[d] + k * W + j] = old[r] + acc[r];
        }
      }
      if (tid < W) {                          // bias gradient of layer d
        real sb_ = 0;
        for (int p = 0; p < 16; ++p) sb_ += Bcur[tid * PD + p].x;
        row[nd.off_b[d] + tid] += sb_;
      }
      __syncthreads();                        // every wave is done reading TI (dW): it becomes the output tile
      // ---- adjoint of layer d-1: in_bar[k][p] = sum_j W_d[k][j] z_bar[j][p], then straight through its tanh
      V4* const Bnxt = TI;
      // the stash of layer d-2 (inputs of the next layer down, written into the tile after this GEMM) is requested
      // now, so that its HBM latency runs under the matrix instructions instead of after them
      constexpr int NREF = WP / RP;
      V4 sref[AHEAD ? NREF : 1];
      if (AHEAD && d >= 2) {
#pragma unroll
        for (int i = 0; i < NREF; ++i) {
          const int j = (tid >> 4) + RP * i;
          sref[AHEAD ? i : 0] = j < W ? S[((size_t)(d - 2) * W + j) * s_pad + lp0 + pe] : V4{0, 0, 0, 0};
        }
      }
      const real* __restrict__ Wd = th + nd.off_w[d];
      for (int kt = wave; kt < NT; kt += NWV) {
        if (16 * kt >= W) {                   // tile entirely in the padding (wave-uniform): zeros
#pragma unroll
          for (int r = 0; r < 4; ++r) Bnxt[(16 * kt + TR::out_row(lane, r)) * PD + m] = V4{0, 0, 0, 0};
          continue;
        }
        V4 sk[4];                             // stash of layer d-1 for this lane's four features (point m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int k = 16 * kt + TR::out_row(lane, r);
          sk[r] = k < W ? S[((size_t)(d - 1) * W + k) * s_pad + lp0 + m] : V4{0, 0, 0, 0};
        }
        acc_t a0 = {0, 0, 0, 0}, a1 = {0, 0, 0, 0}, a2 = {0, 0, 0, 0}, a3 = {0, 0, 0, 0};
        const int k = 16 * kt + m;
        if constexpr (WLDS) {
#pragma unroll 4
          for (int ks = 0; ks < ksteps; ++ks) {
            const int jj = 4 * ks + g;
            const real a = wt[k * TLD + jj];
            const V4 b = Bcur[jj * PD + m];
            a0 = t16_mfma<real, acc_t>(a, b.x, a0);
            a1 = t16_mfma<real, acc_t>(a, b.y, a1);
            a2 = t16_mfma<real, acc_t>(a, b.z, a2);
            a3 = t16_mfma<real, acc_t>(a, b.w, a3);
          }
        } else {
          t16_gemm_l2<real, true, PD, acc_t>(Wd, Bcur, W, k, m, g, a0, a1, a2, a3);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int k = 16 * kt + TR::out_row(lane, r);
          Bnxt[k * PD + m] = k < W ? preact_adjoint(sk[r], V4{a0[r], a1[r], a2[r], a3[r]}) : V4{0, 0, 0, 0};
        }
      }
      __syncthreads();                        // every wave is done reading Bcur (adjoint GEMM): it is refilled
      if (d >= 2) {                           // inputs of layer d-1 = output channels of layer d-2
#pragma unroll
        for (int i = 0; i < NREF; ++i) {
          const int j = (tid >> 4) + RP * i;
          V4 c{0, 0, 0, 0};
          if (j < W) {
            real d1, d2;
            if constexpr (AHEAD) c = channels_of(sref[i], d1, d2);
            else c = channels_of(S[((size_t)(d - 2) * W + j) * s_pad + lp0 + pe], d1, d2);
          }
          Bcur[j * PD + pe] = c;
        }
      }
      V4* tmp = Bcur; Bcur = TI; TI = tmp;     // roles swap: the old TI holds z_bar, the old Bcur the inputs
    }
    __syncthreads();                          // z_bar of dense 0 published (also covers H == 1)
    if (tid < W) {  // dense 0: inputs (hx, ht), p0 = (sx, 0), q0 = (0, st)
      real gx = 0, gt = 0, gb = 0;
      for (int p = 0; p < 16; ++p) {
        const V4 zb = Bcur[tid * PD + p];
        gx += hxy[p] * zb.x + sx * zb.y;
        gt += hxy[16 + p] * zb.x + st * zb.z;
        gb += zb.x;
      }
      row[nd.off_w[0] + tid] += gx;
      row[nd.off_w[0] + W + tid] += gt;
      row[nd.off_b[0] + tid] += gb;
    }
    __syncthreads();                          // seeds / hxy / tiles are rewritten by the next group
  }
  if (tid < 16) {   // loss parts, lambda gradients, output biases: sums over this workgroup's points
#pragma unroll
    for (int k = 0; k < 3; ++k) l_acc[k] = sum16(l_acc[k]);
    dl_acc[0] = sum16(dl_acc[0]); dl_acc[1] = sum16(dl_acc[1]);
    gb_acc[0] = sum16(gb_acc[0]); gb_acc[1] = sum16(gb_acc[1]);
    if (tid == 0) {
      row[nd.n_theta + 0] += l_acc[0]; row[nd.n_theta + 1] += l_acc[1]; row[nd.n_theta + 2] += l_acc[2];
      row[nd.off_b[H]] += gb_acc[0];
      if (NO > 1) row[nd.off_b[H] + 1] += gb_acc[1];
      if (PDE == 1) { row[nd.n_net] += dl_acc[0]; row[nd.n_net + 1] += dl_acc[1]; }
    }
  }
}

}  // namespace pinn
