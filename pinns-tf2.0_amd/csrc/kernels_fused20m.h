// kernels_fused20m.h -- float32 loss+gradient kernel for width-20 tanh MLPs, every contraction on
// the matrix instructions (k_fused20m).  Same workgroup mapping as k_fused20 (kernels_fused20.h:
// 4 waves, lane = point, 64-point tiles, LDS exchange tiles, 16x16x4 weight-gradient tiles), with
//   * persistent workgroups (grid = min(tiles, CUs)); weight-gradient accumulators and the first/
//     last-layer partial sums live in registers across tiles, one gradient row per workgroup;
//   * the Taylor-channel stash (a, z_x, z_t, z_xx) of the wave's 5 features x H layers parked
//     explicitly in AGPRs (160 of the 512-register budget of a one-wave-per-SIMD kernel): no HBM
//     stash, the only global traffic is 8 B/point, the 23 KB weight image and the gradient row;
//   * both layer loops fully unrolled (H is a template parameter);
//   * the layer GEMVs on v_mfma_f32_4x4x1_16B_f32 (below).  Its predecessor with packed-FMA GEMVs
//     (weights lane-distributed, v_readlane -> SGPR operand) measured 72k cycles per tile against
//     64k here (git history: kernels_fused20r.h).
//
// Measured on gfx950 (profiles/r01_ubench_*.txt): a lone wave per SIMD issues one instruction per
// ~5.3 cycles, and v_mfma_f32_* shares the FP32 datapath with the vector ALU (an MFMA and packed
// FMAs never overlap).  A packed FMA retires 128 MACs per issue slot and needs its weight in an
// SGPR (one v_readlane per weight); v_mfma_f32_4x4x1_16B_f32 retires 256 MACs per slot at the full
// 32 MAC/clk/SIMD and takes the weights as a VGPR *pattern*: 16 blocks of 4 lanes, block b
//   D_b[i][j] += A_b[i] * B_b[j],   A: lane 4b+i,  B: lane 4b+j,  D: VGPR i of lane 4b+j.
// With lane = point, B is simply the input-feature register in_c[k], A is the register holding
// W[k][f0 + lane%4] (period-4 pattern, one ds_read_b128 delivers four k at once), and D's four
// VGPRs are out_c[f0..f0+3] of the same point: lane = point in, lane = point out, no padding
// at 4-feature granularity (20 = 5 groups), no readlane, no splat.
//
// Ownership: wave w owns features {4w..4w+3} (group w: all four Taylor channels, 80 MFMAs per layer
// and direction) plus feature 16+w.  Group 4 (features 16..19) is computed one *channel* per wave
// (20 MFMAs), the four channels meet in a 4-row LDS scratch (Q) and wave w picks feature 16+w up
// from there: 100 MFMAs = 826 cycles per wave, layer and direction, against ~2100 cycles for
// the packed-FMA form.
//
// LDS weight image (floats), per hidden dense layer d = 1..H-1, WIMG = 820:
//   [0,400)   W_d^T : [j][k]  forward patterns   (lane reads [(f0 + lane%4)*20 + 4m .. +3])
//   [400,800) W_d   : [k][j]  reverse patterns
//   [800,820) b_d
//
// Math: SURVEY.md Appendix A.1-A.3 == nested GradientTapes of inf_cont_burgers.py:65-90 under
// the outer tape of utils/neuralnetwork.py:55-59.
#pragma once
#include <hip/hip_ext.h>
#include "kernels_fused20.h"

namespace pinn {

// (Ablation builds -- one ingredient compiled out at a time, wrong results by construction, only times are read -- are not part
// of the product sources since round 5.  profiles/ablation_scaffolding.patch holds the -DPINN_ABL / -DPINN_ABLD / -DT16_ABL
// switches of profiles/ablate_*.py; it is not kept up with these sources: it reverse-applies to the tree at ee3788e; check that
// commit out for the ablation builds.  Their results are under profiles/*ablate*.txt.)

typedef float v2f __attribute__((ext_vector_type(2)));
typedef float v4f __attribute__((ext_vector_type(4)));

// The per-layer stash lives in the accumulation half of the unified register file: parking it
// there explicitly (instead of letting the allocator spill to AGPRs) keeps it out of the VGPR
// pressure the scheduler reasons about, so LDS reads can be hoisted well ahead of their use.
__device__ __forceinline__ float agpr_put(const float x) {
  float a;
  asm("v_accvgpr_write_b32 %0, %1" : "=a"(a) : "v"(x));
  return a;
}
__device__ __forceinline__ float agpr_get(const float a) {
  float x;
  asm("v_accvgpr_read_b32 %0, %1" : "=v"(x) : "a"(a));
  return x;
}
__device__ __forceinline__ v4f agpr_put4(const v4f s) {
  return v4f{agpr_put(s.x), agpr_put(s.y), agpr_put(s.z), agpr_put(s.w)};
}
__device__ __forceinline__ v4f agpr_get4(const v4f a) {
  return v4f{agpr_get(a.x), agpr_get(a.y), agpr_get(a.z), agpr_get(a.w)};
}

// one 1-KiB piece global -> LDS (lane i: 16 bytes from g to lds_piece + 16 i), invisible to the compiler -- and so to
// its hazard recogniser: an LDS-DMA that reads m0 needs one wait state behind the s_mov that wrote it (LLVM
// checkReadM0Hazards, gfx9), hence the s_nop INSIDE the asm; tests/helpers/isa_lint.py checks the built library for it.
__device__ __forceinline__ void lds_dma_b128(const float* g, float* lds_piece) {
  const unsigned base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) void*)lds_piece;
  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" : : "v"(g), "s"(base) : "memory", "m0");
}
// makes the compiler wait for a loaded value here
__device__ __forceinline__ void consume4(v4f& v) { asm volatile("" : "+v"(v)); }

// tanh(x) = 1 - 2 / (1 + e^{2x}); absolute error ~1 ulp of 1.0 (cf. tanh_bf)
__device__ __forceinline__ float tanh_r5(float x) {
  const float e = __builtin_amdgcn_exp2f(x * 2.8853900817779268f);
  return fmaf(-2.0f, __builtin_amdgcn_rcpf(1.0f + e), 1.0f);
}

// layer-output channels (h, p, q, r) from a stash entry s = (a, zp, zq, zr)
__device__ __forceinline__ v4f channels4(const v4f s) {
  const float a = s.x, d1 = fmaf(-a, a, 1.0f);
  const float t = (-2.0f * a) * s.y;
  return v4f{a, d1 * s.y, d1 * s.z, d1 * fmaf(t, s.y, s.w)};
}

// adjoint of the pre-activation channels (A.3)
__device__ __forceinline__ v4f preact_adjoint4(const v4f s, const v4f ob) {
  const float a = s.x, a2 = a * a, d1 = 1.0f - a2;
  const float d2 = (-2.0f * a) * d1;
  const float d3 = (-2.0f * d1) * fmaf(-3.0f, a2, 1.0f);
  const float zpw = s.y * ob.w;
  const float dot = fmaf(s.w, ob.w, fmaf(s.z, ob.z, s.y * ob.y));
  v4f zb;
  zb.x = fmaf(d3 * s.y, zpw, fmaf(d2, dot, d1 * ob.x));
  zb.y = fmaf(d2 + d2, zpw, d1 * ob.y);
  zb.z = d1 * ob.z;
  zb.w = d1 * ob.w;
  return zb;
}


constexpr int WIMG = 820;

// padded to whole 1-KiB pieces: the image is brought into LDS by asynchronous LDS-DMA
// (four pieces per round, one per wave: every wave issues the same, compile-time number of DMA
// instructions, so the compiler's vmcnt bookkeeping stays exact and waiting for an earlier plain load
// does not wait for the image)
inline size_t fused20m_image_floats(int n_hidden) { return ((size_t)(n_hidden - 1) * WIMG + 1023) / 1024 * 1024; }
// exchange area in float4: the four [FROWS][65] tiles + the group-4 meeting point Q -- or, if larger, what the
// epilogue parks there (25 row-sum rows of 68 floats per wave + the weight-gradient partials of (H-1) layers)
constexpr int fused20m_xchg_v4(int n_hidden) {
  const int tiles = (4 * FROWS + 4) * 65, epi = 25 * 68 + 4 * (n_hidden - 1) * 2 * 64;
  return tiles > epi ? tiles : epi;
}
inline size_t fused20m_lds_bytes(int n_hidden) {
  return fused20m_image_floats(n_hidden) * 4 + (size_t)fused20m_xchg_v4(n_hidden) * 16;
}

// Called by every kernel that writes a weight: mirrors flat parameter i into the LDS image.
__device__ __forceinline__ void pack_store_m(const NetDesc& nd, float* __restrict__ img, int i, float v) {
  if (!img) return;
  const int lo = nd.off_w[1], hi = nd.off_w[nd.n_hidden];
  if (i < lo || i >= hi) return;
  constexpr int PER = FW * FW + FW;
  const int d1 = (i - lo) / PER, rem = (i - lo) - d1 * PER;
  float* __restrict__ base = img + d1 * WIMG;
  if (rem < FW * FW) {
    const int k = rem / FW, j = rem - k * FW;
    base[j * FW + k] = v;
    base[FW * FW + rem] = v;
  } else {
    base[2 * FW * FW + rem - FW * FW] = v;
  }
}

typedef float acc4 __attribute__((ext_vector_type(4)));

// acc_own[c][i] += sum_k P[(f_own+i)][k] in_c[k]   (c = 0..3)  -- 80 MFMAs
// acc_g4[i]     += sum_k P[(16+i)][k]    in_wave[k]            -- 20 MFMAs (channel = wave index)
// P = 20x20 row-major pattern matrix in LDS (W^T forward, W reverse); in = 20 float4 tiles rows.
// g4_ready(acc_g4) is called as soon as the group-4 unit is complete (the caller publishes it).
// this lane's weight patterns of a 20x20 pattern matrix P (LDS image, or the global image for the
// very first layer): ao = rows of the wave's own group, ag = rows of group 4
__device__ __forceinline__ void load_patterns(const float* __restrict__ P, const int wave, const int lane,
                                              v4f (&ao)[5], v4f (&ag)[5]) {
  const v4f* __restrict__ po = reinterpret_cast<const v4f*>(P + (4 * wave + (lane & 3)) * FW);
  const v4f* __restrict__ pg = reinterpret_cast<const v4f*>(P + (16 + (lane & 3)) * FW);
#pragma unroll
  for (int m = 0; m < 5; ++m) { ao[m] = po[m]; ag[m] = pg[m]; }
}

template <typename G4, typename SIDE>
__device__ __forceinline__ void gemv_mfma(acc4 (&acc_own)[4], acc4& acc_g4, const v4f (&ao)[5], const v4f (&ag)[5],
                                          const int wave, const int lane, const v4f (&in)[FW],
                                          G4 g4_ready, SIDE side) {
#pragma unroll
  for (int k = 0; k < FW; ++k) {
    const float a = ao[k >> 2][k & 3];
    acc_own[0] = __builtin_amdgcn_mfma_f32_4x4x1f32(a, in[k].x, acc_own[0], 0, 0, 0);
    side(4 * k);
    acc_own[1] = __builtin_amdgcn_mfma_f32_4x4x1f32(a, in[k].y, acc_own[1], 0, 0, 0);
    side(4 * k + 1);
    acc_own[2] = __builtin_amdgcn_mfma_f32_4x4x1f32(a, in[k].z, acc_own[2], 0, 0, 0);
    side(4 * k + 2);
    acc_own[3] = __builtin_amdgcn_mfma_f32_4x4x1f32(a, in[k].w, acc_own[3], 0, 0, 0);
    side(4 * k + 3);
  }
  // group 4, one channel per wave: uniform branch, only the selected 20 MFMAs execute; two
  // accumulators so that consecutive MFMAs do not depend on each other.  (Running this unit
  // first, to cover its LDS exchange with the own-group MFMAs, measured 5 % slower per layer.)
  acc4 g4b = {0, 0, 0, 0};
#define G4_CHAIN(COMP)                                                                             \
  _Pragma("unroll") for (int k = 0; k < FW; k += 2) {                                              \
    acc_g4 = __builtin_amdgcn_mfma_f32_4x4x1f32(ag[k >> 2][k & 3], in[k].COMP, acc_g4, 0, 0, 0);   \
    g4b = __builtin_amdgcn_mfma_f32_4x4x1f32(ag[(k + 1) >> 2][(k + 1) & 3], in[k + 1].COMP, g4b, 0, 0, 0); \
  }
  if (wave == 0) { G4_CHAIN(x) } else if (wave == 1) { G4_CHAIN(y) } else if (wave == 2) { G4_CHAIN(z) } else { G4_CHAIN(w) }
#undef G4_CHAIN
  acc_g4 += g4b;
  g4_ready(acc_g4);
}

// ONE_TILE: the launch has at least as many workgroups as tiles (the 10^4-point headline), so the
// tile loop is a single pass: no loop-carried coordinate prefetch, which lets the compiler wait for
// the first coordinates without also draining the image DMA issued behind them.
#define PINN_F20M_BOUNDS __launch_bounds__(256)
#define PINN_STASH_KEEP(d) true
template <int PDE, int H, bool ONE_TILE>
__global__ PINN_F20M_BOUNDS void k_fused20m(const float* __restrict__ th, const float* __restrict__ img,
                                            const float* __restrict__ xs, const float* __restrict__ ts,
                                            const float* __restrict__ tgt, float* __restrict__ part, int R,
                                            int n_tiles, float lbx, float lbt, float sx, float st, float nu,
                                            SetDesc sd, long long* __restrict__ stamps) {
  constexpr W20Desc nd = w20_desc(H, pde_n_tail(PDE));      // (pointers + R + n_tiles = the 14 preloaded argument dwords)
  constexpr int RS4 = 65;
  constexpr int BUFV = FROWS * RS4;                 // v4f elements per exchange buffer
  constexpr int NW = ((H - 1) * WIMG + 1023) / 1024 * 1024;   // floats of weight image (whole rounds of 4 DMA pieces)
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  float* const wl = reinterpret_cast<float*>(lds_raw);
  v4f* const xb = reinterpret_cast<v4f*>(wl + NW);
  v4f* const Q = xb + 4 * BUFV;                     // group-4 meeting point: [4][RS4] float4
  float* const Qf = reinterpret_cast<float*>(Q);

  STAMP(0);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  float* __restrict__ row = part + (size_t)blockIdx.x * R;
  // this wave's features: local jj = 0..3 -> 4*wave + jj, jj = 4 -> 16 + wave
  auto feat = [&](int jj) { return jj < 4 ? 4 * wave + jj : 16 + wave; };

  // first tile's coordinates
  int tile = blockIdx.x;
  float x = 0.0f, t = 0.0f;
  if (tile < n_tiles) { x = xs[tile * 64 + lane]; t = ts[tile * 64 + lane]; }

  // first hidden layer of the first tile: its patterns and biases come straight from the global
  // image into registers, in the same memory round trip as the coordinates -- the LDS image is only
  // needed from the second hidden layer on
  v4f pre_o[5], pre_g[5], pre_b, pre_bg;
  load_patterns(img, wave, lane, pre_o, pre_g);
  pre_b = *reinterpret_cast<const v4f*>(img + 2 * FW * FW + 4 * wave);
  pre_bg = *reinterpret_cast<const v4f*>(img + 2 * FW * FW + 16);

  STAMP(19);
  if (wave == 0) {
    xb[0 * BUFV + FW * RS4 + lane] = v4f{1, 0, 0, 0};
    xb[2 * BUFV + FW * RS4 + lane] = v4f{1, 0, 0, 0};
  }
  // first / last dense layer parameters of this wave (wave-uniform)
  float w0x[FF], w0t[FF], b0[FF], wLo[FF], wL[FW];
#pragma unroll
  for (int jj = 0; jj < FF; ++jj) {
    w0x[jj] = th[nd.off_w[0] + feat(jj)];
    w0t[jj] = th[nd.off_w[0] + FW + feat(jj)];
    b0[jj] = th[nd.off_b[0] + feat(jj)];
    wLo[jj] = th[nd.off_w[H] + feat(jj)];
  }
#pragma unroll
  for (int k = 0; k < FW; ++k) wL[k] = th[nd.off_w[H] + k];
  const float bL = th[nd.off_b[H]];
  float c1 = 1.0f, c2 = nu;
  if (PDE == 1) { c1 = th[nd.n_net]; c2 = __expf(th[nd.n_net + 1]); }
  const float inv_nf = (float)sd.inv_nf, inv_nu = (float)sd.inv_nu;

  // accumulators that live across tiles
  // dW_d (+ db_d as row 20) = IN^T . ZB over the tile's 256 (point,channel) rows, as
  //   dwm[d]: the 16x16 block (k < 16, j < 16) on v_mfma_f32_16x16x4 -- this wave's quarter of the rows
  //           (points 16q + 4w .. +3 of every lane group q), 16 MFMAs;
  //   dwf[d]: the fringe (k = 16..20 or j = 16..19; 164 entries) as 14 of the 16 independent 4x4
  //           blocks of v_mfma_f32_4x4x1_16B, one (point,channel) row per instruction -- this wave's
  //           16 points, 64 MFMAs.
  // (Padding the fringe out to three more 16x16 tiles, one tile per wave, cost 64 x 32-cycle
  // MFMAs per wave and layer; this split costs 16 x 32 + 64 x 8.)  The four waves' partial sums meet
  // once per kernel in the epilogue.
  acc4 dwm[H], dwf[H];
#pragma unroll
  for (int d = 0; d < H; ++d) dwm[d] = dwf[d] = acc4{0, 0, 0, 0};
  float g0x[FF], g0t[FF], g0b[FF], gH[FF];
#pragma unroll
  for (int jj = 0; jj < FF; ++jj) g0x[jj] = g0t[jj] = g0b[jj] = gH[jj] = 0.0f;
  float gHb = 0.0f, l_res = 0.0f, l_dat = 0.0f, dl0 = 0.0f, dl1 = 0.0f;

  // main block operands: A row = input feature lane%16, B column = output feature lane%16,
  // lane group q = lane/16 supplies point 16q + 4w + jj at step jj
  // fringe block b = lane/4 -> (input-feature group kg, output-feature group jg):
  //   b 0..3: (4, b)   b 4..7: (5 = ones row, b-4)   b 8..11: (b-8, 4)   b 12: (4, 4)   b 13..15: (5, 4)
  // (a macro: the tile loop re-derives these from an opaque copy of the lane index once per tile, see there)
#define PINN_LANE_INDICES_M(L)                                                                                        \
  const int lane = (L);                                                                                                \
  const int mrow = (lane & 15) * RS4 + (lane >> 4) * 16 + 4 * wave;                                                    \
  const int fblk = lane >> 2;                                                                                          \
  const int fkg = fblk < 4 ? 4 : fblk < 8 ? 5 : fblk < 12 ? fblk - 8 : fblk == 12 ? 4 : 5;                             \
  const int fjg = fblk < 8 ? (fblk & 3) : 4;                                                                           \
  const int farow = min(4 * fkg + (lane & 3), FW) * RS4 + 16 * wave;     /* rows past the ones row repeat it */        \
  const int fbrow = (4 * fjg + (lane & 3)) * RS4 + 16 * wave;                                                          \
  const int qw = 4 * lane + wave;                             /* float index of (point, channel = wave) in a Q row */  \
  (void)mrow; (void)farow; (void)fbrow; (void)qw; (void)fkg; (void)fjg; (void)fblk
  STAMP(1);
  bool image_pending = true;

  for (; tile < n_tiles; tile += gridDim.x) {
    // tile loop: lane index re-read through an opaque asm once per tile, per-lane indices re-derived -- keeps hipcc from
    // carrying the LDS addresses they feed across the loop: same-box A/B at N_f = 10^6 1307 / 1316 vs 1333 / 1337 us per
    // Adam step (-1.7 %), the 10-layer tile-loop variant's scratch 216 -> 136 B per lane (profiles/r04_opaque_lane_ab.txt)
    int lane_o = tid & 63;
    if (!ONE_TILE) asm volatile("" : "+v"(lane_o));
    PINN_LANE_INDICES_M(lane_o);
    const int pt = tile * 64 + lane;
    const float hx = fmaf(sx, x - lbx, -1.0f), ht = fmaf(st, t - lbt, -1.0f);
    {  // next tile's coordinates: in flight during this tile
      const int nt = tile + gridDim.x;
      if (!ONE_TILE && nt < n_tiles) { x = xs[nt * 64 + lane]; t = ts[nt * 64 + lane]; }
    }
    v4f stash[H][FF];                            // AGPR-resident (agpr_put4 / agpr_get4)

    // ------------------------------------------------------------------ forward
#pragma unroll
    for (int jj = 0; jj < FF; ++jj) {            // dense 0: p0 = (sx, 0), q0 = (0, st), r0 = 0
      const float z = fmaf(hx, w0x[jj], fmaf(ht, w0t[jj], b0[jj]));
      const v4f s{tanh_r5(z), sx * w0x[jj], st * w0t[jj], 0.0f};
      stash[0][jj] = PINN_STASH_KEEP(0) ? agpr_put4(s) : v4f{0.25f, 0.5f, 0.25f, 0.5f};
      xb[feat(jj) * RS4 + lane] = channels4(s);
    }
    if (image_pending) {                         // the pre-loaded patterns have arrived (same round trip as x, t)
#pragma unroll
      for (int m = 0; m < 5; ++m) { consume4(pre_o[m]); consume4(pre_g[m]); }
      consume4(pre_b); consume4(pre_bg);
      STAMP(22);
    }
    lds_barrier();
    if (image_pending) {
      // ---- weight image -> LDS by asynchronous LDS-DMA (global_load_lds_dwordx4: 1 KiB per wave
      // instruction, no registers), in flight during the first hidden layer and drained before the
      // second.  Written as inline assembly on purpose: hipcc makes every LDS access that follows a
      // DMA it knows about wait for vmcnt(0) (it cannot tell the image from the exchange tiles),
      // which would put the whole fetch latency back in front of the first layer.  Unseen, the DMA
      // can only make the compiler's own vmcnt waits stricter (counters retire in order), and all
      // its earlier loads have been consumed by now.
#pragma unroll
      for (int m = 0; m < NW / 1024; ++m)
        lds_dma_b128(img + (4 * m + wave) * 256 + lane * 4, wl + (4 * m + wave) * 256);
      STAMP(23);
    }
#pragma unroll
    for (int d = 1; d < H; ++d) {
      const v4f* __restrict__ Xin = xb + ((d - 1) & 1) * BUFV;
      v4f* __restrict__ Xout = xb + (d & 1) * BUFV;
      const float* __restrict__ wimg = wl + (d - 1) * WIMG;
      v4f xin[FW];
#pragma unroll
      for (int k = 0; k < FW; ++k) xin[k] = Xin[k * RS4 + lane];
      acc4 acc_own[4], acc_g4;
      v4f ao[5], ag[5];
      if (d == 1 && image_pending) {
#pragma unroll
        for (int m = 0; m < 5; ++m) { ao[m] = pre_o[m]; ag[m] = pre_g[m]; }
        acc_own[0] = pre_b; acc_g4 = pre_bg;
      } else {
        load_patterns(wimg, wave, lane, ao, ag);
        acc_own[0] = *reinterpret_cast<const v4f*>(wimg + 2 * FW * FW + 4 * wave);   // bias b_d[4w..4w+3]
        acc_g4 = *reinterpret_cast<const v4f*>(wimg + 2 * FW * FW + 16);
      }
      acc_own[1] = acc_own[2] = acc_own[3] = acc4{0, 0, 0, 0};
      if (wave != 0) acc_g4 = acc4{0, 0, 0, 0};                                      // bias rides on channel h
      if (d == 4) STAMP(24);
      // group 4: this wave's channel of features 16..19 is published as soon as it is complete
      gemv_mfma(acc_own, acc_g4, ao, ag, wave, lane, xin,
                [&](const acc4& g) {
#pragma unroll
                  for (int i = 0; i < 4; ++i) Qf[i * RS4 * 4 + qw] = g[i];
                },
                [](int) {});
      if (d == 4) STAMP(25);
      if (d == 1 && image_pending) STAMP(20);
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const v4f s{tanh_r5(acc_own[0][jj]), acc_own[1][jj], acc_own[2][jj], acc_own[3][jj]};
        stash[d][jj] = PINN_STASH_KEEP(d) ? agpr_put4(s) : v4f{0.25f, 0.5f, 0.25f, 0.5f};
        Xout[(4 * wave + jj) * RS4 + lane] = channels4(s);
      }
      if (d == 4) STAMP(26);
      lds_barrier();
      if (d == 4) STAMP(27);
      {
        const v4f z4 = Q[wave * RS4 + lane];      // feature 16+wave: (h, p, q, r) pre-activations
        const v4f s{tanh_r5(z4.x), z4.y, z4.z, z4.w};
        stash[d][4] = PINN_STASH_KEEP(d) ? agpr_put4(s) : v4f{0.25f, 0.5f, 0.25f, 0.5f};
        Xout[(16 + wave) * RS4 + lane] = channels4(s);
      }
      if (d == 1 && image_pending) {             // first tile only: this wave's DMA pieces have landed
        STAMP(21);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        image_pending = false;
      }
      lds_barrier();
      STAMP(1 + d);
    }
    // linear output layer (every wave computes it) -> o = (u, u_x, u_t, u_xx)
    v4f o{bL, 0, 0, 0};
    {
      const v4f* __restrict__ Xin = xb + ((H - 1) & 1) * BUFV;
      v4f xin[FW];
#pragma unroll
      for (int k = 0; k < FW; ++k) xin[k] = Xin[k * RS4 + lane];
#pragma unroll
      for (int k = 0; k < FW; ++k) {
        o.x = fmaf(xin[k].x, wL[k], o.x); o.y = fmaf(xin[k].y, wL[k], o.y);
        o.z = fmaf(xin[k].z, wL[k], o.z); o.w = fmaf(xin[k].w, wL[k], o.w);
      }
    }

    // ------------------------------------------------------------------ seeds + loss parts
    v4f sb{0, 0, 0, 0};
    {
      const int cls = point_class(sd, pt);
      const bool res = (PDE == 0) ? (cls == CLS_COL) : (cls == CLS_DATA);
      if (res) {
        const float wgt = (PDE == 0) ? inv_nf : inv_nu;
        const float f = o.z + c1 * o.x * o.y - c2 * o.w;
        const float fbar = 2.0f * f * wgt;
        l_res += f * f * wgt;
        sb = v4f{fbar * c1 * o.y, fbar * c1 * o.x, fbar, -c2 * fbar};
        if (PDE == 1) { dl0 += fbar * o.x * o.y; dl1 -= fbar * c2 * o.w; }
      }
      if (cls == CLS_DATA) {
        const float dd = o.x - tgt[pt];
        l_dat += dd * dd * inv_nu;
        sb.x += 2.0f * dd * inv_nu;
      }
    }

    // ------------------------------------------------------------------ reverse sweep
    v4f ob[FF];                              // adjoint of the outputs of the layer below, own features
    {  // dense H (linear): z_bar = sb
      gHb += sb.x;
#pragma unroll
      for (int kk = 0; kk < FF; ++kk) {
        const v4f in = channels4(PINN_STASH_KEEP(H - 1) ? agpr_get4(stash[H - 1][kk]) : stash[H - 1][kk]);
        gH[kk] += fmaf(in.w, sb.w, fmaf(in.z, sb.z, fmaf(in.y, sb.y, in.x * sb.x)));
        ob[kk] = sb * wLo[kk];
      }
    }
    lds_barrier();          // every wave is done reading the forward tile before it is overwritten
    STAMP(H + 1);
#pragma unroll
    for (int d = H - 1; d >= 1; --d) {
      const int pair = (H - 1 - d) & 1;
      v4f* __restrict__ IN = xb + (2 * pair) * BUFV;
      v4f* __restrict__ ZB = xb + (2 * pair + 1) * BUFV;
      // phase A: publish own z_bar (layer d) and own layer-(d-1) output channels
#pragma unroll
      for (int kk = 0; kk < FF; ++kk) {
        ZB[feat(kk) * RS4 + lane] = preact_adjoint4(PINN_STASH_KEEP(d) ? agpr_get4(stash[d][kk]) : stash[d][kk], ob[kk]);
        IN[feat(kk) * RS4 + lane] = channels4(PINN_STASH_KEEP(d - 1) ? agpr_get4(stash[d - 1][kk]) : stash[d - 1][kk]);
      }
      if (d == 4) STAMP(28);
      lds_barrier();
      if (d == 4) STAMP(29);
      // phase B: adjoint of own layer-(d-1) outputs  in_bar[k] = sum_j z_bar_j W_d[k][j]  (4x4x1 MFMAs)
      //          and dW_d tile += IN^T . ZB over the 256 (point,channel) rows (16x16x4 MFMAs),
      //          one of the latter after every pair of the former
      const float* __restrict__ wimg = wl + (d - 1) * WIMG + FW * FW;
      v4f zin[FW];
#pragma unroll
      for (int j = 0; j < FW; ++j) zin[j] = ZB[j * RS4 + lane];
      // operand rings, refilled two steps ahead: main block step jj = 0..3 (4 MFMAs each, one per
      // channel), fringe step p = 0..15 (one point, 4 MFMAs)
      v4f ma[2], mb[2], fa4[2], fb4[2];
      ma[0] = IN[mrow + 0]; mb[0] = ZB[mrow + 0];
      ma[1] = IN[mrow + 1]; mb[1] = ZB[mrow + 1];
      fa4[0] = IN[farow + 0]; fb4[0] = ZB[fbrow + 0];
      fa4[1] = IN[farow + 1]; fb4[1] = ZB[fbrow + 1];
      acc4 acc_own[4], acc_g4 = {0, 0, 0, 0};
#pragma unroll
      for (int c = 0; c < 4; ++c) acc_own[c] = acc4{0, 0, 0, 0};
      acc4 accm = dwm[d], accf = dwf[d];
      auto dw_mfma = [&](int s) {              // s = 0..79, one after every own-group GEMV MFMA
        if (s % 5 == 4) {                      // 16 main-block MFMAs: step jj = m/4, channel m%4
          const int m = s / 5, jj = m >> 2, c = m & 3;
          const v4f a = ma[jj & 1], b = mb[jj & 1];
          accm = __builtin_amdgcn_mfma_f32_16x16x4f32(a[c], b[c], accm, 0, 0, 0);
          if (c == 3 && jj + 2 < 4) { ma[jj & 1] = IN[mrow + jj + 2]; mb[jj & 1] = ZB[mrow + jj + 2]; }
        } else {                               // 64 fringe MFMAs: point p = m/4, channel m%4
          const int m = s - s / 5, p = m >> 2, c = m & 3;
          const v4f a = fa4[p & 1], b = fb4[p & 1];
          accf = __builtin_amdgcn_mfma_f32_4x4x1f32(a[c], b[c], accf, 0, 0, 0);
          if (c == 3 && p + 2 < 16) { fa4[p & 1] = IN[farow + p + 2]; fb4[p & 1] = ZB[fbrow + p + 2]; }
        }
      };
      v4f ao[5], ag[5];
      load_patterns(wimg, wave, lane, ao, ag);
      gemv_mfma(acc_own, acc_g4, ao, ag, wave, lane, zin,
                [&](const acc4& g) {
#pragma unroll
                  for (int i = 0; i < 4; ++i) Qf[i * RS4 * 4 + qw] = g[i];
                },
                [&](int slot) { dw_mfma(slot); });   // slots 0..79
      dwm[d] = accm; dwf[d] = accf;
      if (d == 4) STAMP(30);
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) ob[kk] = v4f{acc_own[0][kk], acc_own[1][kk], acc_own[2][kk], acc_own[3][kk]};
      lds_barrier();
      ob[4] = Q[wave * RS4 + lane];
      STAMP(2 * H + 1 - d);
    }
    {  // dense 0: inputs (hx, ht), p0 = (sx, 0), q0 = (0, st)
#pragma unroll
      for (int kk = 0; kk < FF; ++kk) {
        const v4f zb = preact_adjoint4(PINN_STASH_KEEP(0) ? agpr_get4(stash[0][kk]) : stash[0][kk], ob[kk]);
        g0x[kk] += fmaf(hx, zb.x, sx * zb.y);
        g0t[kk] += fmaf(ht, zb.x, st * zb.z);
        g0b[kk] += zb.x;
      }
    }
    lds_barrier();          // the next tile's first layer overwrites an exchange buffer
    if (ONE_TILE) break;
  }
  STAMP(2 * H + 1);

  // -------------------------------------------------------------------- one gradient row per workgroup
  {
    // 25 per-lane partials -> lane totals through this wave's slice of the (now free) exchange
    // area: 25 row writes, then lane (v, half) adds up 32 entries of row v with 8 ds_read_b128 and
    // the two halves meet through one bpermute.  (A DPP butterfly per value costs ~3x the issue slots.)
    constexpr int NV = 25, RSF = 68;                 // rows; padded row stride in floats (16-B aligned)
    float* __restrict__ red = reinterpret_cast<float*>(xb) + wave * (NV * RSF);
    // behind the four waves' row areas: the weight-gradient partials, [wave][layer][main|fringe][lane]
    constexpr int PSW = (H - 1) * 2 * 64;            // float4 per wave
    v4f* const psum = xb + NV * RSF;
    static_assert(NV * RSF + 4 * PSW <= fused20m_xchg_v4(H), "partials fit in the exchange area");
#pragma unroll
    for (int d = 1; d < H; ++d) {
      psum[wave * PSW + ((d - 1) * 2 + 0) * 64 + lane] = dwm[d];
      psum[wave * PSW + ((d - 1) * 2 + 1) * 64 + lane] = dwf[d];
    }
#pragma unroll
    for (int kk = 0; kk < FF; ++kk) {
      red[(0 + kk) * RSF + lane] = g0x[kk];
      red[(5 + kk) * RSF + lane] = g0t[kk];
      red[(10 + kk) * RSF + lane] = g0b[kk];
      red[(15 + kk) * RSF + lane] = gH[kk];
    }
    red[20 * RSF + lane] = l_res; red[21 * RSF + lane] = l_dat; red[22 * RSF + lane] = gHb;
    red[23 * RSF + lane] = dl0;   red[24 * RSF + lane] = dl1;
    const int v = lane & 31, half = lane >> 5;
    float tot = 0.0f;
    if (v < NV) {
      const v4f* __restrict__ src = reinterpret_cast<const v4f*>(red + v * RSF + 32 * half);
      v4f q[8];
#pragma unroll
      for (int m = 0; m < 8; ++m) q[m] = src[m];
      v4f s4 = ((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]));
      tot = (s4.x + s4.y) + (s4.z + s4.w);
    }
    tot += __int_as_float(__builtin_amdgcn_ds_bpermute((lane ^ 32) << 2, __float_as_int(tot)));
    if (lane < 20) {
      const int grp = lane / 5, kk = lane - grp * 5;
      const int f = kk < 4 ? 4 * wave + kk : 16 + wave;
      const int base = grp == 0 ? nd.off_w[0] : grp == 1 ? nd.off_w[0] + FW : grp == 2 ? nd.off_b[0] : nd.off_w[H];
      row[base + f] = tot;
    } else if (wave == 0 && lane < NV) {
      if (lane == 20) { row[nd.n_theta + 0] = tot; row[nd.n_theta + 2] = 0.0f; }
      if (lane == 21) row[nd.n_theta + 1] = tot;
      if (lane == 22) row[nd.off_b[H]] = tot;
      if (PDE == 1 && lane == 23) row[nd.n_net] = tot;
      if (PDE == 1 && lane == 24) row[nd.n_net + 1] = tot;
    }
    STAMP(31);
    // dW / db: the four waves' partial blocks (published above) are added up layer by layer, wave w
    // taking layers w+1, w+5, ...  b_d sits right behind W_d in the flat layout, so input-feature row
    // 20 (the ones row) lands on the bias.
    lds_barrier();
    const int km = 4 * (lane >> 4), jm = lane & 15;              // main block: VGPR r -> input feature km + r
    PINN_LANE_INDICES_M(tid & 63);
    const int kf = 4 * fkg, jf = 4 * fjg + (lane & 3);           // fringe block: VGPR r -> input feature kf + r
    const bool okf = fblk <= 13;
#pragma unroll
    for (int half = 0; half < (H - 1 + 3) / 4; ++half) {
      const int d1 = wave + 4 * half;
      if (d1 < H - 1) {
        float* __restrict__ dst = row + nd.off_w[1] + d1 * (FW * FW + FW);
        const v4f* __restrict__ src = psum + (d1 * 2) * 64 + lane;
        const v4f m4 = (src[0 * PSW] + src[1 * PSW]) + (src[2 * PSW] + src[3 * PSW]);
        const v4f f4 = (src[0 * PSW + 64] + src[1 * PSW + 64]) + (src[2 * PSW + 64] + src[3 * PSW + 64]);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          dst[(km + r) * FW + jm] = m4[r];
          if (okf && kf + r <= FW) dst[(kf + r) * FW + jf] = f4[r];
        }
      }
    }
  }
  STAMP(2 * H + 2);
}

// returns a hipError_t (0 = ok)
template <int PDE, int H>
inline int fused20m_launch(const NetDesc& nd, const SetDesc& sd, const float* th, const float* img,
                           const float* xs, const float* ts, const float* tgt, float lbx, float lbt,
                           float sx, float st, float nu, float* part, int R, int n_wg,
                           hipStream_t stream, long long* stamps = nullptr, hipEvent_t ev_start = nullptr,
                           hipEvent_t ev_stop = nullptr) {
  if (!w20_layout_ok(nd, H, pde_n_tail(PDE))) return (int)hipErrorInvalidValue;
  const size_t lds = fused20m_lds_bytes(H);
  static unsigned long long attr_set = 0;
  if (first_call_on_device(attr_set)) {
    hipError_t e = hipFuncSetAttribute((const void*)k_fused20m<PDE, H, false>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e == hipSuccess)
      e = hipFuncSetAttribute((const void*)k_fused20m<PDE, H, true>,
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  const int n_tiles = sd.n_pad / 64;
  auto* const kern = n_wg >= n_tiles ? k_fused20m<PDE, H, true> : k_fused20m<PDE, H, false>;
  if (ev_start && ev_stop)      // the events take the kernel's own begin / end timestamps (what a profiler reports)
    hipExtLaunchKernelGGL(kern, dim3(n_wg), dim3(256), lds, stream, ev_start, ev_stop, 0, th, img, xs, ts, tgt, part,
                          R, n_tiles, lbx, lbt, sx, st, nu, sd, stamps);
  else
    hipLaunchKernelGGL(kern, dim3(n_wg), dim3(256), lds, stream, th, img, xs, ts, tgt, part, R, n_tiles, lbx, lbt, sx,
                       st, nu, sd, stamps);
  return (int)hipGetLastError();
}

}  // namespace pinn
