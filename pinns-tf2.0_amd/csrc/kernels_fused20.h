// kernels_fused20.h -- fused loss+gradient kernel for width-20 tanh MLPs (the Burgers nets of
// 1d-burgers/inf_cont_burgers.py:33 and ide_cont_burgers.py:33), one launch per evaluation.
//
// Mapping (wave64, gfx950):
//   workgroup = 256 threads = 4 waves = one tile of 64 points; lane = point, wave w owns the
//   5 features [5w, 5w+5) of every hidden layer (one wave per SIMD of the CU).
//   * hidden-layer weights are staged once per workgroup into LDS in two per-wave packed layouts
//     (forward columns / reverse rows); a wave fetches the 5 weights it needs per step with one
//     broadcast ds_read_b128 (+b32), so the FMAs are VGPR x VGPR and nothing competes for SGPRs.
//   * layer GEMVs (forward z = in.W, reverse in_bar = z_bar.W^T): each wave needs all 20 input
//     features of its 64 points -> exchanged through LDS as [feature][point] float4 (h,p,q,r)
//     tiles (ds_read_b128, conflict-free); 20 independent accumulators per step give the ILP a
//     single wave per SIMD needs.
//   * weight gradient dW = IN^T . ZBAR is a [21 x 256] x [256 x 20] contraction over the tile's
//     (point,channel) rows: it runs on the matrix pipe as four 16x16 output tiles (one per wave)
//     of v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64 reading A and B straight from the same
//     LDS exchange tiles (row stride padded so the b128 operand fetches are conflict-free),
//     interleaved with the reverse GEMV's vector FMAs.  A constant "ones" feature row turns the
//     bias gradient into row 20 of the same product.  No cross-lane shuffles, no atomics; f32
//     MFMA is bit-equal to an fmaf chain, so the result is deterministic.
//   * per-layer Taylor channels (a, z_x, z_t, z_xx) of the wave's own 5 features are stashed to
//     HBM/L2 in [layer][feature][point] order (1 KiB contiguous per wave store) and read back by
//     the same lanes in the reverse sweep, prefetched one layer ahead; workgroup barriers wait on
//     LDS traffic only, never on those stores.
//   * each workgroup emits one partial-gradient row; k_reduce_rows sums rows in fixed order.
//
// Math: SURVEY.md Appendix A.1-A.3 == nested GradientTapes of inf_cont_burgers.py:65-90 under
// the outer tape of utils/neuralnetwork.py:55-59.
#pragma once
#include <hip/hip_ext.h>
#include "kernels_generic.h"

namespace pinn {

constexpr int FW = 20;          // hidden width served by this kernel
constexpr int FF = 5;           // features per wave
constexpr int FROWS = 21;       // 20 features + the ones row (bias gradient)

template <typename real> struct FusedTraits;
template <> struct FusedTraits<float> {
  using acc_t = float __attribute__((ext_vector_type(4)));
  static constexpr int RS4 = 65;     // LDS row stride in vec4 units (64 points + 1 pad): 1040 B
  static constexpr int NBUF = 2;     // ping-pong (IN, ZBAR) pairs -> one barrier per layer
  static constexpr int WS = 8;       // packed-weight slot: 5 weights + 3 pad = 32 B
  static __device__ __forceinline__ void load5(const float* p, float w[5]) {
    const vec4<float> a = *reinterpret_cast<const vec4<float>*>(p);
    w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w; w[4] = p[4];
  }
  static __device__ __forceinline__ acc_t mfma(float a, float b, acc_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ int out_row(int lane, int reg) { return (lane >> 4) * 4 + reg; }
};
template <> struct FusedTraits<double> {
  using acc_t = double __attribute__((ext_vector_type(4)));
  static constexpr int RS4 = 65;     // 65 * 32 B = 2080 B
  static constexpr int NBUF = 1;     // 160 KiB LDS holds one pair in f64 -> two barriers per layer
  static constexpr int WS = 6;       // 5 weights + 1 pad = 48 B
  static __device__ __forceinline__ void load5(const double* p, double w[5]) {
    struct alignas(16) d2 { double a, b; };
    const d2 u = *reinterpret_cast<const d2*>(p), v = *reinterpret_cast<const d2*>(p + 2);
    w[0] = u.a; w[1] = u.b; w[2] = v.a; w[3] = v.b; w[4] = p[4];
  }
  static __device__ __forceinline__ acc_t mfma(double a, double b, acc_t c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ int out_row(int lane, int reg) { return (lane >> 4) + 4 * reg; }
};

// Flat-vector layout of a 2 -> 20 x H -> 1 net as COMPILE-TIME constants (the reference layout: W then b per dense
// layer, utils/neuralnetwork.py:60-77 get_weights / set_weights).  The register-stash kernels take their offsets from
// here, not from a NetDesc argument: weight addresses become immediate operands and, with the pointers leading the
// argument list, the first loads of a launch do not wait for a kernel-argument fetch (the leading 14 dwords of the
// arguments are preloaded into SGPRs: -mllvm -amdgpu-kernarg-preload-count, pinn_native.COMMON_FLAGS).  The launch
// wrappers check the engine's NetDesc against it (w20_layout_ok).
struct W20Desc { int off_w[MAX_DENSE]; int off_b[MAX_DENSE]; int n_net; int n_theta; };
// (n_tail: trailing equation parameters behind the net's scalars -- 0, 2 lambdas or the six adr coefficients, pde_n_tail)
constexpr W20Desc w20_desc(int H, int n_tail) {
  W20Desc r{};
  int off = 0, in = 2;
  for (int d = 0; d <= H; ++d) {
    const int out = d < H ? FW : 1;
    r.off_w[d] = off; off += in * out;
    r.off_b[d] = off; off += out;
    in = out;
  }
  r.n_net = off;
  r.n_theta = off + n_tail;
  return r;
}
inline bool w20_layout_ok(const NetDesc& nd, int H, int n_tail) {
  const W20Desc w = w20_desc(H, n_tail);
  if (nd.n_hidden != H || nd.width != FW || nd.n_out != 1 || nd.n_net != w.n_net || nd.n_theta != w.n_theta) return false;
  for (int d = 0; d <= H; ++d)
    if (nd.off_w[d] != w.off_w[d] || nd.off_b[d] != w.off_b[d]) return false;
  return true;
}

inline bool fused20_supported(const NetDesc& nd) {
  return nd.width == FW && nd.n_out == 1 && nd.n_hidden >= 2;
}
inline int fused20_rows(const SetDesc& sd) { return sd.n_pad / 64; }

// LDS carve-up (units of `real`):
//   [exchange buffers: 2*NBUF x FROWS x RS4 vec4] [Pf: (H-1) x 20 x 4 x WS] [Pb: same] [bh: (H-1) x 20]
//   Pf[d][k][w][jj] = W_d[k][5w+jj]   (forward:  wave w's 5 columns of input row k)
//   Pb[d][j][w][kk] = W_d[5w+kk][j]   (reverse:  wave w's 5 rows at output column j)
template <typename real>
inline size_t fused20_lds_bytes(int n_hidden) {
  using TR = FusedTraits<real>;
  const size_t xch = (size_t)2 * TR::NBUF * FROWS * TR::RS4 * 4;
  const size_t wts = (size_t)(n_hidden - 1) * (2 * FW * 4 * TR::WS + FW);
  return (xch + wts) * sizeof(real);
}

// LDS-only workgroup barrier: orders this wave's ds ops before the barrier without waiting for
// outstanding global stores (the stash is only ever re-read by the thread that wrote it).
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// branch-free tanh: sign(x) * (1 - e^{-2|x|}) / (1 + e^{-2|x|}).  Absolute error ~1 ulp of 1.0,
// the same order as the roundoff already carried by the 20-term pre-activation sums.
__device__ __forceinline__ float tanh_bf(float x) {
  const float t = __builtin_amdgcn_exp2f(fabsf(x) * -2.8853900817779268f);
  const float r = (1.0f - t) * __builtin_amdgcn_rcpf(1.0f + t);
  return copysignf(r, x);
}
__device__ __forceinline__ double tanh_bf(double x) {
  const double t = exp(-2.0 * fabs(x));
  return copysign((1.0 - t) / (1.0 + t), x);
}

// Optional per-wave phase timeline (s_memtime ticks), compiled in only with -DPINN_STAMPS
// (the profiling build libpinn_hip_stamps.so); see profiles/stamps.py.
#ifdef PINN_STAMPS
#define STAMP(i)                                                                   \
  do {                                                                             \
    if (stamps && (threadIdx.x & 63) == 0)                                         \
      stamps[((size_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 32 + (i)] = clock64(); \
  } while (0)
#else
#define STAMP(i) do { } while (0)
#endif

template <typename real, int PDE>
__global__ __launch_bounds__(256) void k_fused20(NetDesc nd, SetDesc sd,
                                                 const real* __restrict__ th,
                                                 const real* __restrict__ xs,
                                                 const real* __restrict__ ts,
                                                 const real* __restrict__ tgt, real lbx, real lbt,
                                                 real sx, real st, real nu,
                                                 vec4<real>* __restrict__ S,
                                                 real* __restrict__ part, int R,
                                                 long long* __restrict__ stamps) {
  using TR = FusedTraits<real>;
  using acc_t = typename TR::acc_t;
  constexpr int RS4 = TR::RS4;
  constexpr int WS = TR::WS;
  constexpr int BUFV = FROWS * RS4;               // vec4 elements per exchange buffer
  extern __shared__ __attribute__((aligned(32))) unsigned char lds_raw[];
  vec4<real>* const lds = reinterpret_cast<vec4<real>*>(lds_raw);

  STAMP(0);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j0 = wave * FF;
  const int pt = blockIdx.x * 64 + lane;
  const int n_pad = sd.n_pad;
  const int H = nd.n_hidden;
  real* __restrict__ row = part + (size_t)blockIdx.x * R;

  auto BUF = [&](int b) { return lds + b * BUFV; };
  real* const Pf = reinterpret_cast<real*>(lds + 2 * TR::NBUF * BUFV);
  real* const Pb = Pf + (H - 1) * FW * 4 * WS;
  real* const bh = Pb + (H - 1) * FW * 4 * WS;

  // ---- stage the hidden-layer weights into LDS in the two per-wave packed layouts
  for (int idx = tid; idx < (H - 1) * FW * FW; idx += 256) {
    const int d1 = idx / (FW * FW), rem = idx - d1 * FW * FW;
    const int k = rem / FW, j = rem - k * FW;
    const real w = th[nd.off_w[d1 + 1] + rem];
    Pf[((d1 * FW + k) * 4 + j / FF) * WS + j % FF] = w;
    Pb[((d1 * FW + j) * 4 + k / FF) * WS + k % FF] = w;
  }
  for (int idx = tid; idx < (H - 1) * FW; idx += 256) {
    const int d1 = idx / FW;
    bh[idx] = th[nd.off_b[d1 + 1] + idx - d1 * FW];
  }
  // ones row (feature 20 of every IN buffer): (1,0,0,0) per point -> bias gradients via MFMA
  if (wave == 0) {
#pragma unroll
    for (int b = 0; b < 2 * TR::NBUF; b += 2) BUF(b)[FW * RS4 + lane] = vec4<real>{1, 0, 0, 0};
  }

  const real x = xs[pt], t = ts[pt];
  const real hx = sx * (x - lbx) - real(1), ht = st * (t - lbt) - real(1);

  // ------------------------------------------------------------------ forward
  vec4<real> cur_s[FF];                   // stash entries of the current layer, own features
  {  // dense 0
    const real* __restrict__ W0 = th + nd.off_w[0];
    const real* __restrict__ b0 = th + nd.off_b[0];
    vec4<real>* __restrict__ X = BUF(0);
#pragma unroll
    for (int jj = 0; jj < FF; ++jj) {
      const int j = j0 + jj;
      const real w0 = W0[j], w1 = W0[FW + j];
      const real z = hx * w0 + ht * w1 + b0[j];
      const vec4<real> s{tanh_bf(z), sx * w0, st * w1, real(0)};
      cur_s[jj] = s;
      S[(size_t)j * n_pad + pt] = s;
      real d1, d2;
      X[j * RS4 + lane] = channels_of(s, d1, d2);
    }
  }
  __syncthreads();                        // weights staged + layer-0 tile published
  STAMP(1);
  int cur = 0;
  for (int d = 1; d < H; ++d) {
    const vec4<real>* __restrict__ Xin = BUF(cur);
    vec4<real>* __restrict__ Xout = BUF(cur ^ 1);
    const real* __restrict__ Wf = Pf + ((d - 1) * FW * 4 + wave) * WS;
    real az[FF], ap[FF], aq[FF], ar[FF];
#pragma unroll
    for (int jj = 0; jj < FF; ++jj) {
      az[jj] = bh[(d - 1) * FW + j0 + jj];
      ap[jj] = aq[jj] = ar[jj] = real(0);
    }
#pragma unroll
    for (int k = 0; k < FW; ++k) {
      const vec4<real> in = Xin[k * RS4 + lane];
      real w[FF];
      TR::load5(Wf + k * 4 * WS, w);
#pragma unroll
      for (int jj = 0; jj < FF; ++jj) {
        az[jj] += in.x * w[jj]; ap[jj] += in.y * w[jj]; aq[jj] += in.z * w[jj]; ar[jj] += in.w * w[jj];
      }
    }
    vec4<real>* __restrict__ Sd = S + (size_t)d * FW * n_pad + pt;
#pragma unroll
    for (int jj = 0; jj < FF; ++jj) {
      const vec4<real> s{tanh_bf(az[jj]), ap[jj], aq[jj], ar[jj]};
      cur_s[jj] = s;
      Sd[(size_t)(j0 + jj) * n_pad] = s;
      real d1, d2;
      Xout[(j0 + jj) * RS4 + lane] = channels_of(s, d1, d2);
    }
    cur ^= 1;
    lds_barrier();
    STAMP(1 + d);
  }
  // linear output layer (every wave computes it: 80 FMAs) -> o = (u, u_x, u_t, u_xx)
  vec4<real> o{th[nd.off_b[H]], 0, 0, 0};
  {
    const real* __restrict__ WL = th + nd.off_w[H];
    const vec4<real>* __restrict__ Xin = BUF(cur);
#pragma unroll
    for (int k = 0; k < FW; ++k) {
      const vec4<real> in = Xin[k * RS4 + lane];
      const real w = WL[k];
      o.x += in.x * w; o.y += in.y * w; o.z += in.z * w; o.w += in.w * w;
    }
  }

  // ------------------------------------------------------------------ seeds + loss parts
  real c1 = real(1), c2 = nu;
  if (PDE == 1) { c1 = th[nd.n_net]; c2 = exp(th[nd.n_net + 1]); }
  vec4<real> sb{0, 0, 0, 0};
  {
    real lt0 = 0, lt1 = 0, dl0 = 0, dl1 = 0;
    const int cls = point_class(sd, pt);
    const real inv_nf = (real)sd.inv_nf, inv_nu = (real)sd.inv_nu;
    const bool res = (PDE == 0) ? (cls == CLS_COL) : (cls == CLS_DATA);
    if (res) {
      const real wgt = (PDE == 0) ? inv_nf : inv_nu;
      const real f = o.z + c1 * o.x * o.y - c2 * o.w;
      const real fb = real(2) * f * wgt;
      lt0 = f * f * wgt;
      sb = vec4<real>{fb * c1 * o.y, fb * c1 * o.x, fb, -c2 * fb};
      if (PDE == 1) { dl0 = fb * o.x * o.y; dl1 = -fb * c2 * o.w; }
    }
    if (cls == CLS_DATA) {
      const real dd = o.x - tgt[pt];
      lt1 = dd * dd * inv_nu;
      sb.x += real(2) * dd * inv_nu;
    }
    if (wave == 0) {
      const real a = wave_sum(lt0), b = wave_sum(lt1);
      if (lane == 0) { row[nd.n_theta + 0] = a; row[nd.n_theta + 1] = b; row[nd.n_theta + 2] = real(0); }
      if (PDE == 1) {
        const real g1 = wave_sum(dl0), g2 = wave_sum(dl1);
        if (lane == 0) { row[nd.n_net] = g1; row[nd.n_net + 1] = g2; }
      }
    }
  }

  // ------------------------------------------------------------------ reverse sweep
  vec4<real> ob[FF];                       // adjoint of the outputs of the layer below, own features
  vec4<real> prev_s[FF];                   // stash of layer d-1 (prefetched one layer ahead)
  {
    const vec4<real>* __restrict__ Sp = S + (size_t)(H - 2) * FW * n_pad + pt;
#pragma unroll
    for (int kk = 0; kk < FF; ++kk) prev_s[kk] = Sp[(size_t)(j0 + kk) * n_pad];
  }
  {  // dense H (linear): z_bar = sb
    const real* __restrict__ WL = th + nd.off_w[H];
    real keep = 0;
#pragma unroll
    for (int kk = 0; kk < FF; ++kk) {
      real d1, d2;
      const vec4<real> in = channels_of(cur_s[kk], d1, d2);
      const real g = wave_sum(dot4(in, sb));
      if (lane == kk) keep = g;
      const real w = WL[j0 + kk];
      ob[kk] = vec4<real>{sb.x * w, sb.y * w, sb.z * w, sb.w * w};
    }
    if (lane < FF) row[nd.off_w[H] + j0 + lane] = keep;
    if (wave == 0) {
      const real g = wave_sum(sb.x);
      if (lane == 0) row[nd.off_b[H]] = g;
    }
  }
  lds_barrier();          // every wave is done reading the forward tile before it is overwritten
  STAMP(H + 1);

  const int ti = wave >> 1, tj = wave & 1;                    // this wave's 16x16 tile of dW
  const int fa = min(16 * ti + (lane & 15), FW);              // A row: input feature (20 = ones)
  const int fb = min(16 * tj + (lane & 15), FW - 1);          // B column: output feature
  const int kq = (lane >> 4) * 16;                            // this lane group's 16 points
  int pair = 0;
  for (int d = H - 1; d >= 1; --d) {
    vec4<real>* __restrict__ IN = BUF(2 * pair);
    vec4<real>* __restrict__ ZB = BUF(2 * pair + 1);
    vec4<real> next_s[FF];
    {
      const int dn = d >= 2 ? d - 2 : 0;                      // (d == 1: harmless re-read)
      const vec4<real>* __restrict__ Sp = S + (size_t)dn * FW * n_pad + pt;
#pragma unroll
      for (int kk = 0; kk < FF; ++kk) next_s[kk] = Sp[(size_t)(j0 + kk) * n_pad];
    }
    // phase A: publish own z_bar (layer d) and own layer-(d-1) output channels
#pragma unroll
    for (int kk = 0; kk < FF; ++kk) {
      ZB[(j0 + kk) * RS4 + lane] = preact_adjoint(cur_s[kk], ob[kk]);
      real d1, d2;
      IN[(j0 + kk) * RS4 + lane] = channels_of(prev_s[kk], d1, d2);
    }
    lds_barrier();
    // phase B: matrix pipe -- dW_d tile = IN^T . ZB over the 256 (point,channel) rows;
    //          vector pipe -- adjoint of own layer-(d-1) outputs = sum_j z_bar_j W_d[k][j]
    const real* __restrict__ Wb = Pb + ((d - 1) * FW * 4 + wave) * WS;
    acc_t acc = {0, 0, 0, 0};
#pragma unroll
    for (int kk = 0; kk < FF; ++kk) ob[kk] = vec4<real>{0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < FW; ++j) {
      if (j < 16) {
        const vec4<real> a4 = IN[fa * RS4 + kq + j];
        const vec4<real> b4 = ZB[fb * RS4 + kq + j];
        acc = TR::mfma(a4.x, b4.x, acc);
        acc = TR::mfma(a4.y, b4.y, acc);
        acc = TR::mfma(a4.z, b4.z, acc);
        acc = TR::mfma(a4.w, b4.w, acc);
      }
      const vec4<real> z4 = ZB[j * RS4 + lane];
      real w[FF];
      TR::load5(Wb + j * 4 * WS, w);
#pragma unroll
      for (int kk = 0; kk < FF; ++kk) {
        ob[kk].x += z4.x * w[kk]; ob[kk].y += z4.y * w[kk];
        ob[kk].z += z4.z * w[kk]; ob[kk].w += z4.w * w[kk];
      }
    }
    {  // scatter the dW / db tile into this workgroup's partial row
      const int jg = 16 * tj + (lane & 15);
      if (jg < FW) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int ig = 16 * ti + TR::out_row(lane, r);
          if (ig < FW) row[nd.off_w[d] + ig * FW + jg] = acc[r];
          else if (ig == FW) row[nd.off_b[d] + jg] = acc[r];
        }
      }
    }
#pragma unroll
    for (int kk = 0; kk < FF; ++kk) { cur_s[kk] = prev_s[kk]; prev_s[kk] = next_s[kk]; }
    if (TR::NBUF == 2) pair ^= 1; else lds_barrier();
    STAMP(2 * H + 1 - d);
  }
  {  // dense 0: inputs (hx, ht), p0 = (sx, 0), q0 = (0, st)
    real kx = 0, kt = 0, kb = 0;
#pragma unroll
    for (int kk = 0; kk < FF; ++kk) {
      const vec4<real> zb = preact_adjoint(cur_s[kk], ob[kk]);
      const real gx = wave_sum(hx * zb.x + sx * zb.y);
      const real gt = wave_sum(ht * zb.x + st * zb.z);
      const real gb = wave_sum(zb.x);
      if (lane == kk) { kx = gx; kt = gt; kb = gb; }
    }
    if (lane < FF) {
      row[nd.off_w[0] + j0 + lane] = kx;
      row[nd.off_w[0] + FW + j0 + lane] = kt;
      row[nd.off_b[0] + j0 + lane] = kb;
    }
  }
  STAMP(2 * H + 1);
}

// returns a hipError_t (0 = ok)
template <typename real, int PDE>
inline int fused20_launch(const NetDesc& nd, const SetDesc& sd, const real* th, const real* xs,
                          const real* ts, const real* tgt, real lbx, real lbt, real sx, real st,
                          real nu, vec4<real>* S, real* part, int R, hipStream_t stream,
                          long long* stamps = nullptr, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr) {
  const size_t lds = fused20_lds_bytes<real>(nd.n_hidden);
  static size_t attr_set[64] = {};                 // per device: the attribute belongs to the device's code object
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (attr_set[dev & 63] < lds) {
    hipError_t e = hipFuncSetAttribute((const void*)k_fused20<real, PDE>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
    attr_set[dev & 63] = lds;
  }
  if (ev_start && ev_stop)      // the events take the kernel's own begin / end timestamps (what a profiler reports)
    hipExtLaunchKernelGGL((k_fused20<real, PDE>), dim3(sd.n_pad / 64), dim3(256), lds, stream, ev_start, ev_stop, 0,
                          nd, sd, th, xs, ts, tgt, lbx, lbt, sx, st, nu, S, part, R, stamps);
  else
    hipLaunchKernelGGL((k_fused20<real, PDE>), dim3(sd.n_pad / 64), dim3(256), lds, stream, nd, sd, th,
                       xs, ts, tgt, lbx, lbt, sx, st, nu, S, part, R, stamps);
  return (int)hipGetLastError();
}

}  // namespace pinn
