// kernels_optim.h -- deterministic gradient reduction, Adam, device-resident L-BFGS.
// All optimiser state is float64 whatever the kernel compute dtype (the reference is
// float64 end to end, utils/neuralnetwork.py:24-26); the compute kernels read a `real`
// mirror of the weights that these kernels keep in sync.
#pragma once
#include "kernels_wide.h"

namespace pinn {

// gl[c] = sum over rows of part[row*R + c] in a fixed order (bit-reproducible).
// gl layout: [0, n_theta) gradient | n_theta+0..2 loss parts (residual, data, boundary).
// Block = 64 columns x 16 row-slices (row r belongs to slice r & 15): 1024 threads; the slices are combined through LDS
// in index order.  Grid = ceil(R / 64) blocks.
// A thread of slice q owns rows q, q + 16, ...; accumulator k of its eight takes rows q + 16 k, q + 16 k + 128, ... in that
// order.  PINN_REDUCE_ONE_ROUND = 1 requests the 16 rows of every 256 (predicated) before the first wait: one memory round
// trip for any launch of up to 256 rows.  0 is the earlier schedule: 8 loads per round, and each row of the tail behind a
// branch and a wait of its own -- at the headline's 158 rows three dependent round trips.  Same sums, bit for bit
// (tests/test_gpu_reduce_one_round.py); the A/B is profiles/reduce_one_round_ab.txt.
#ifndef PINN_REDUCE_ONE_ROUND
#define PINN_REDUCE_ONE_ROUND 1
#endif
constexpr int RED_COLS = 64;
constexpr int RED_SLICES = 16;
constexpr int RED_THREADS = RED_COLS * RED_SLICES;   // (measured: 8 / 16 / 32 columns per workgroup, i.e. 8x / 4x / 2x the
                                                     //  workgroups, are no faster: f64 Adam step 41.9 / 40.9 / 40.6 vs 40.9 us; neither are two columns per thread
                                                     //  on an even row pitch, 512 threads, bit-identical sums: 41.3 vs 40.8 us, f32 29.3 vs 28.3; nor non-temporal row
                                                     //  loads: 41.9 vs 40.8 us -- part of the rows is still in an L2.  None of these touched the
                                                     //  chain of dependent load rounds inside a thread; PINN_REDUCE_ONE_ROUND does: headline step
                                                     //  44.31 -> 43.63 us at 158 rows, nothing at 128 rows, where the loop was one round already:
                                                     //  profiles/reduce_one_round_ab.txt)

template <typename real>
__device__ __forceinline__ double reduce_column(const real* __restrict__ part, int n_rows, int R,
                                                int c, int q, double (*sh)[RED_COLS]) {
  const int cl = threadIdx.x & 63;
  double a0 = 0, a1 = 0, a2 = 0, a3 = 0, a4 = 0, a5 = 0, a6 = 0, a7 = 0;
  if (c < R) {
#if PINN_REDUCE_ONE_ROUND
    // q = threadIdx.x >> 6 is the wave's number, so row numbers and predicates are uniform (scalar branches round the loads).
    // With per-lane row numbers the 16 address pairs live next to the 16 values: 95 VGPRs, and k_reduce_xgmi spills (200 B)
    const unsigned lane_off = (unsigned)c * (unsigned)sizeof(real);
    for (int r0 = __builtin_amdgcn_readfirstlane(q); r0 < n_rows; r0 += 16 * RED_SLICES) {
      real v[16];
#pragma unroll
      for (int i = 0; i < 16; ++i)
        v[i] = (r0 + i * RED_SLICES < n_rows)
                   ? *(const real*)((const char*)(part + (size_t)(r0 + i * RED_SLICES) * R) + lane_off) : real(0);
      // an absent row keeps the accumulator (a + 0.0 would turn a -0.0 into +0.0); rows r0 + 128.. follow rows r0.. as in the loop below
#define PINN_RED_ADD(a, i) a = (r0 + (i) * RED_SLICES < n_rows) ? a + (double)v[i] : a
      PINN_RED_ADD(a0, 0); PINN_RED_ADD(a1, 1); PINN_RED_ADD(a2, 2); PINN_RED_ADD(a3, 3);
      PINN_RED_ADD(a4, 4); PINN_RED_ADD(a5, 5); PINN_RED_ADD(a6, 6); PINN_RED_ADD(a7, 7);
      PINN_RED_ADD(a0, 8); PINN_RED_ADD(a1, 9); PINN_RED_ADD(a2, 10); PINN_RED_ADD(a3, 11);
      PINN_RED_ADD(a4, 12); PINN_RED_ADD(a5, 13); PINN_RED_ADD(a6, 14); PINN_RED_ADD(a7, 15);
#undef PINN_RED_ADD
    }
#else
    const real* __restrict__ p = part + c;
    int r = q;
    for (; r + 7 * RED_SLICES < n_rows; r += 8 * RED_SLICES) {
      a0 += (double)p[(size_t)(r + 0 * RED_SLICES) * R]; a1 += (double)p[(size_t)(r + 1 * RED_SLICES) * R];
      a2 += (double)p[(size_t)(r + 2 * RED_SLICES) * R]; a3 += (double)p[(size_t)(r + 3 * RED_SLICES) * R];
      a4 += (double)p[(size_t)(r + 4 * RED_SLICES) * R]; a5 += (double)p[(size_t)(r + 5 * RED_SLICES) * R];
      a6 += (double)p[(size_t)(r + 6 * RED_SLICES) * R]; a7 += (double)p[(size_t)(r + 7 * RED_SLICES) * R];
    }
    if (r < n_rows) a0 += (double)p[(size_t)r * R];
    if (r + 1 * RED_SLICES < n_rows) a1 += (double)p[(size_t)(r + 1 * RED_SLICES) * R];
    if (r + 2 * RED_SLICES < n_rows) a2 += (double)p[(size_t)(r + 2 * RED_SLICES) * R];
    if (r + 3 * RED_SLICES < n_rows) a3 += (double)p[(size_t)(r + 3 * RED_SLICES) * R];
    if (r + 4 * RED_SLICES < n_rows) a4 += (double)p[(size_t)(r + 4 * RED_SLICES) * R];
    if (r + 5 * RED_SLICES < n_rows) a5 += (double)p[(size_t)(r + 5 * RED_SLICES) * R];
    if (r + 6 * RED_SLICES < n_rows) a6 += (double)p[(size_t)(r + 6 * RED_SLICES) * R];
#endif
  }
  sh[q][cl] = ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7));
  __syncthreads();
  double tot = 0;
  if (q == 0) {
#pragma unroll
    for (int i = 0; i < RED_SLICES; ++i) tot += sh[i][cl];
  }
  return tot;
}

// Hidden-layer weight gradients that k_t16_fused (kernels_tile16f.h) leaves in its TILE-MAJOR scratch instead of copying
// them into the partial rows (round 5): one block of `stride` doubles per workgroup, slot e = (layer - 1) n_tiles + rt ntl + ct
// of 256 doubles = the 64 lanes' four accumulator entries (vec4 per lane) of gradient tile (rt, ct); a strip (T16Deal) uses
// the first 64 doubles.  The copy cost every workgroup a 294 KB read + 246 KB scattered write at the end of the kernel, all
// CUs at once (34 k of 886 k cycles, profiles/r05_t16f_stamps_edge_v1.txt), only for this reduction to read the rows back.
// Now the reduction kernels take those columns from the scratch: workgroups [n_cb, n_cb + n_slots) of their grid own one
// slot each (whole 2 KB lines per row block), the column workgroups skip the columns that are `backed`.
struct TileScratch {
  const double* gscr;       // nullptr: every column comes from the partial rows
  long long stride;         // doubles per workgroup block (a multiple of 256)
  int n_slots, n_tiles, ntl, W, edge, off_w1, pitch;   // n_slots = (H - 1) n_tiles; off_w1 = off_w[1]; pitch = W W + W
  __host__ __device__ bool backed(const int c) const {
    if (!gscr) return false;
    const int rel = c - off_w1;
    if (rel < 0) return false;
    const int l = rel / pitch;
    return l < n_slots / n_tiles && rel - l * pitch < W * W;
  }
  // flat-vector column of entry `comp` of lane L's vec4 in slot e, or -1 (padding).  Lane maps: kernels_tile16f.h
  // (full tile: row 16 rt + (L >> 4) + 4 comp, column 16 ct + (L & 15); strips: entry sl = 4 L + comp of the first 64)
  __device__ int column(const int e, const int L, const int comp) const {
    const int dl = e / n_tiles, tau = e - dl * n_tiles, rt = tau / ntl, ct = tau - rt * ntl;
    const int kind = !edge ? 0 : rt == ntl - 1 ? 2 : ct == ntl - 1 ? 1 : 0;
    int k, j;
    if (kind == 0) { k = 16 * rt + (L >> 4) + 4 * comp; j = 16 * ct + (L & 15); }
    else {
      if (L >= 16) return -1;
      const int sl = 4 * L + comp;
      k = 16 * rt + (kind == 1 ? 4 * ((sl >> 2) & 3) : 0) + (sl >> 4);
      j = 16 * ct + (kind == 1 ? (sl & 3) : (sl & 15));
    }
    return (k < W && j < W) ? off_w1 + dl * pitch + k * W + j : -1;
  }
};

// sums of slot e (the 64 lanes of the tile: every 2 KB block) over the n_rows workgroup blocks, fixed order (slices of rows,
// then the slices in index order); tot[comp] valid in the threads of slice 0 (threadIdx.x < 64), whose tile lane is L.  One
// workgroup per slot: 147 workgroups for cfg 4, which leaves 109 CUs idle in a launch that is pure streaming (17.7 us for
// 75 MB, profiles/r05_cfg4_kernel_stats_v7.txt).  (Tried and dropped: half a slot per workgroup, 294 workgroups for cfg 4:
// 20.3 us against 17.4 -- 1 KB pieces stream worse.)
__device__ __forceinline__ void reduce_slot(const TileScratch& ts, const int n_rows, const int sb, double (*sh)[RED_COLS],
                                            double (&tot)[4], int& e, int& L) {
  using V4 = vec4<double>;
  constexpr int NSL = RED_THREADS / 64;                           // row slices
  e = sb;
  const int q = threadIdx.x / 64, l = threadIdx.x - q * 64;
  L = l;
  double* const shf = &sh[0][0];                                  // [NSL][64]
  const V4* __restrict__ p = reinterpret_cast<const V4*>(ts.gscr + (size_t)e * 256) + L;
  const size_t sv = (size_t)(ts.stride / 4);
  V4 a[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) a[u] = V4{0, 0, 0, 0};
  // a strip's slot holds 64 doubles: lanes 16.. of the vec4 view are padding nobody wrote -- not read (20 % of cfg 4's bytes)
  int r = (ts.column(e, L, 0) < 0 && ts.column(e, L, 1) < 0 && ts.column(e, L, 2) < 0 && ts.column(e, L, 3) < 0) ? n_rows : q;
  for (; r + 7 * NSL < n_rows; r += 8 * NSL) {
    V4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = p[(size_t)(r + u * NSL) * sv];
#pragma unroll
    for (int u = 0; u < 8; ++u) { a[u].x += v[u].x; a[u].y += v[u].y; a[u].z += v[u].z; a[u].w += v[u].w; }
  }
#pragma unroll
  for (int u = 0; u < 7; ++u)
    if (r + u * NSL < n_rows) {
      const V4 v = p[(size_t)(r + u * NSL) * sv];
      a[u].x += v.x; a[u].y += v.y; a[u].z += v.z; a[u].w += v.w;
    }
  auto sum8 = [&](auto get) {
    return ((get(a[0]) + get(a[1])) + (get(a[2]) + get(a[3]))) + ((get(a[4]) + get(a[5])) + (get(a[6]) + get(a[7])));
  };
  const double part4[4] = {sum8([](const V4& t) { return t.x; }), sum8([](const V4& t) { return t.y; }),
                           sum8([](const V4& t) { return t.z; }), sum8([](const V4& t) { return t.w; })};
#pragma unroll
  for (int comp = 0; comp < 4; ++comp) {
    if (comp) __syncthreads();
    shf[q * 64 + l] = part4[comp];
    __syncthreads();
    tot[comp] = 0;
    if (q == 0) {
#pragma unroll
      for (int i = 0; i < NSL; ++i) tot[comp] += shf[i * 64 + l];
    }
  }
}

// One Adam step of entry i in the form of TF-2.0 ResourceApplyAdam (reference call site
// utils/neuralnetwork.py:114): m += (1-b1)(g-m); v += (1-b2)(g^2-v); theta -= alpha*m/(sqrt(v)+eps), alpha =
// lr*sqrt(1-b2^t)/(1-b1^t) computed by the host.  Every kernel that steps weights calls this one function, so a member of
// an ensemble, a rank of a data-parallel group and a solo context run the same arithmetic.  Returns the new weight.
__device__ __forceinline__ double adam_entry(const int i, const double g, double* __restrict__ theta,
                                             double* __restrict__ m, double* __restrict__ v, const double alpha,
                                             const double b1, const double b2, const double eps) {
  const double mi = m[i] + (1.0 - b1) * (g - m[i]);
  const double vi = v[i] + (1.0 - b2) * (g * g - v[i]);
  m[i] = mi;
  v[i] = vi;
  const double t = theta[i] - alpha * mi / (sqrt(vi) + eps);
  theta[i] = t;
  return t;
}
// ... and the copies of the new weight the sweeps read: the working-precision vector and the packed float32 image
template <typename real>
__device__ __forceinline__ void adam_step(const int i, const double g, double* __restrict__ theta,
                                          real* __restrict__ theta_r, double* __restrict__ m, double* __restrict__ v,
                                          const double alpha, const double b1, const double b2, const double eps,
                                          const NetDesc& nd, float* __restrict__ img) {
  const double t = adam_entry(i, g, theta, m, v, alpha, b1, b2, eps);
  theta_r[i] = (real)t;
  pack_store_any(nd, img, i, (float)t);
}

// Non-finite guard (SURVEY 5 "failure detection"; the reference has none: a NaN loss just propagates,
// utils/custom_lbfgs.py:154).  The thread that owns a loss slot records the number of the first evaluation whose
// reduced loss part is not finite; nothing else changes, the trajectory stays the reference's.
__device__ __forceinline__ void note_nonfinite(double g, int c, int n_theta, unsigned long long eval_no,
                                               unsigned long long* __restrict__ nonfinite) {
  if (nonfinite && c >= n_theta && c < n_theta + 3 && !isfinite(g)) atomicCAS(nonfinite, 0ull, eval_no);
}

template <typename real>
__global__ __launch_bounds__(RED_THREADS) void k_reduce_rows(const real* __restrict__ part, int n_rows,
                                                             int R, double* __restrict__ gl, int n_theta = 0,
                                                             unsigned long long eval_no = 0,
                                                             unsigned long long* __restrict__ nonfinite = nullptr,
                                                             TileScratch ts = TileScratch{}) {
  __shared__ double sh[RED_SLICES][RED_COLS];
  const int q = threadIdx.x >> 6, n_cb = (R + RED_COLS - 1) / RED_COLS;
  if ((int)blockIdx.x >= n_cb) {               // a slot of k_t16_fused's scratch (grid = n_cb + ts.n_slots)
    double tot[4];
    int e, L;
    reduce_slot(ts, n_rows, blockIdx.x - n_cb, sh, tot, e, L);
    if (threadIdx.x < 64) {
#pragma unroll
      for (int comp = 0; comp < 4; ++comp) {
        const int c = ts.column(e, L, comp);
        if (c >= 0) gl[c] = tot[comp];
      }
    }
    return;
  }
  const int c = blockIdx.x * RED_COLS + (threadIdx.x & 63);
  const bool skip = ts.backed(c);
  const double g = reduce_column(part, n_rows, R, skip ? R : c, q, sh);
  if (q == 0 && c < R && !skip) { gl[c] = g; note_nonfinite(g, c, n_theta, eval_no, nonfinite); }
}

// Single-GPU Adam step fused behind the reduction (no all-reduce in between): same arithmetic as
// k_reduce_rows followed by k_adam.  loss3 (may be null) <- the three loss parts of this step.
template <typename real>
__global__ __launch_bounds__(RED_THREADS) void k_reduce_adam(const real* __restrict__ part, int n_rows,
                                                             int R, double* __restrict__ gl, int n,
                                                             double* __restrict__ theta,
                                                             real* __restrict__ theta_r,
                                                             double* __restrict__ m, double* __restrict__ v,
                                                             double alpha, double b1, double b2, double eps,
                                                             double* __restrict__ loss3, NetDesc nd,
                                                             float* __restrict__ img,
                                                             unsigned long long eval_no = 0,
                                                             unsigned long long* __restrict__ nonfinite = nullptr,
                                                             TileScratch ts = TileScratch{}) {
  __shared__ double sh[RED_SLICES][RED_COLS];
  const int q = threadIdx.x >> 6, n_cb = (R + RED_COLS - 1) / RED_COLS;
  auto finish = [&](const int c, const double g) {
    gl[c] = g;
    note_nonfinite(g, c, n, eval_no, nonfinite);
    if (c < n) {
      adam_step(c, g, theta, theta_r, m, v, alpha, b1, b2, eps, nd, img);
    } else if (loss3 && c < n + 3) {
      loss3[c - n] = g;
    }
  };
  if ((int)blockIdx.x >= n_cb) {               // a slot of k_t16_fused's scratch (grid = n_cb + ts.n_slots)
    double tot[4];
    int e, L;
    reduce_slot(ts, n_rows, blockIdx.x - n_cb, sh, tot, e, L);
    if (threadIdx.x < 64) {
#pragma unroll
      for (int comp = 0; comp < 4; ++comp) {
        const int c = ts.column(e, L, comp);
        if (c >= 0) finish(c, tot[comp]);
      }
    }
    return;
  }
  const int c = blockIdx.x * RED_COLS + (threadIdx.x & 63);
  const bool skip = ts.backed(c);
  const double g = reduce_column(part, n_rows, R, skip ? R : c, q, sh);
  if (q != 0 || c >= R || skip) return;
  finish(c, g);
}

// ---- ensembles: K members sharing the point set, float64, kernel path 7 (grid.y = member) ------------------------------
// The member kernels below are k_reduce_rows / k_reduce_adam with per-member bases and the same per-column arithmetic, so a
// member's gradient, moments and weights are bit-identical to a solo engine's.  Layouts: part [K][n_rows][R], gl [K][R],
// theta / m / v [K][n], theta_r [K][sw] (sw = fused20d_weight_doubles(n): the LDS-DMA pieces of k_fused20d's ENS variants),
// loss3 [K][3] (per step), nonfinite [K].
constexpr int ENS_MAX = 64;
struct EnsStep {
  double alpha[ENS_MAX];                  // Adam: the member's step size, formed on the host exactly as adam_issue forms it
  unsigned long long eval_no[ENS_MAX];    // the member's evaluation number; 0: the member is not reduced by this launch
};

__global__ __launch_bounds__(RED_THREADS) void k_reduce_rows_ens(const double* __restrict__ part, int n_rows, int R,
                                                                 double* __restrict__ gl, int n_theta,
                                                                 unsigned long long* __restrict__ nonfinite, EnsStep es) {
  __shared__ double sh[RED_SLICES][RED_COLS];
  const int mem = blockIdx.y;
  const unsigned long long eval_no = es.eval_no[mem];
  if (eval_no == 0) return;
  part += (size_t)mem * n_rows * R;
  gl += (size_t)mem * R;
  const int q = threadIdx.x >> 6, c = blockIdx.x * RED_COLS + (threadIdx.x & 63);
  const double g = reduce_column(part, n_rows, R, c, q, sh);
  if (q == 0 && c < R) { gl[c] = g; note_nonfinite(g, c, n_theta, eval_no, nonfinite + mem); }
}

__global__ __launch_bounds__(RED_THREADS) void k_reduce_adam_ens(const double* __restrict__ part, int n_rows, int R,
                                                                 double* __restrict__ gl, int n, int sw,
                                                                 double* __restrict__ theta, double* __restrict__ theta_r,
                                                                 double* __restrict__ m, double* __restrict__ v,
                                                                 double b1, double b2, double eps,
                                                                 double* __restrict__ loss3,
                                                                 unsigned long long* __restrict__ nonfinite, EnsStep es) {
  __shared__ double sh[RED_SLICES][RED_COLS];
  const int mem = blockIdx.y;
  const unsigned long long eval_no = es.eval_no[mem];
  if (eval_no == 0) return;
  const double alpha = es.alpha[mem];
  part += (size_t)mem * n_rows * R;
  gl += (size_t)mem * R;
  theta += (size_t)mem * n; m += (size_t)mem * n; v += (size_t)mem * n;
  theta_r += (size_t)mem * sw;
  const int q = threadIdx.x >> 6, c = blockIdx.x * RED_COLS + (threadIdx.x & 63);
  const double g = reduce_column(part, n_rows, R, c, q, sh);
  if (q != 0 || c >= R) return;
  gl[c] = g;
  note_nonfinite(g, c, n, eval_no, nonfinite + mem);
  if (c < n) {
    theta_r[c] = adam_entry(c, g, theta, m, v, alpha, b1, b2, eps);
  } else if (loss3 && c < n + 3) {
    loss3[(size_t)mem * 3 + c - n] = g;
  }
}

// The Adam step as a launch of its own (behind an all-reduce of gl)
template <typename real>
__global__ void k_adam(int n, const double* __restrict__ gl, double* __restrict__ theta,
                       real* __restrict__ theta_r, double* __restrict__ m,
                       double* __restrict__ v, double alpha, double b1, double b2, double eps,
                       double* __restrict__ loss3, int n_theta, NetDesc nd,
                       float* __restrict__ img) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 3 && loss3) loss3[i] = gl[n_theta + i];
  if (i >= n) return;
  adam_step(i, gl[i], theta, theta_r, m, v, alpha, b1, b2, eps, nd, img);
}

template <typename real>
__global__ void k_cast_weights(int n, const double* __restrict__ theta, real* __restrict__ theta_r,
                               NetDesc nd, float* __restrict__ img) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { theta_r[i] = (real)theta[i]; pack_store_any(nd, img, i, (float)theta[i]); }
}

// ---------------------------------------------------------------------------------------------
// L-BFGS (utils/custom_lbfgs.py:39-236), one 1024-thread workgroup, float64.
// ---------------------------------------------------------------------------------------------
// row stride (doubles) of the two history rings: even, so that a row starts 16-byte aligned (pair loads in k_lbc_dots)
__host__ __device__ inline size_t ring_ld(int n) { return ((size_t)n + 1) & ~(size_t)1; }

struct LbfgsState {
  int n_iter;        // state.nIter
  int func_eval;     // currentFuncEval
  int hist_len;      // len(old_dirs)
  int hist_head;     // ring index of the oldest pair
  int done;          // 0 running | 1 nIter==maxIter | 2 gtd>-tolX | 3 maxEval | 4 tolFun | 5 step<tolX | 6 |df|<tolX | 7 initial tolFun
  int n_logged;      // log_fn calls so far
  int pad0, pad1;
  double Hdiag, t, f, f_old, final_loss;
};

constexpr int LB_THREADS = 1024;

__device__ __forceinline__ double block_sum(double v, double* sh) {
  // fixed-shape reduction: wave DPP sum, then the 16 wave totals in index order
  const double w = wave_sum(v);
  const int wid = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[wid] = w;
  __syncthreads();
  double tot = 0;
#pragma unroll
  for (int i = 0; i < LB_THREADS / 64; ++i) tot += sh[i];
  return tot;
}

// Compute the search direction, step, and advance x (custom_lbfgs.py:84-174).
//   g    : gradient at the current x (= gl from the last evaluation)
//   x    : L-BFGS iterate;  theta/theta_r: model weights (set only when an evaluation follows,
//          i.e. when nIter != maxIter -- custom_lbfgs.py:176 + neuralnetwork.py:94)
template <typename real>
__global__ __launch_bounds__(LB_THREADS) void k_lbfgs_step(
    int n, int max_iter, int n_corr, double lr, double tol_x, LbfgsState* __restrict__ st,
    const double* __restrict__ g, double* __restrict__ x, double* __restrict__ theta,
    real* __restrict__ theta_r, double* __restrict__ d, double* __restrict__ g_old,
    double* __restrict__ Sh, double* __restrict__ Yh, double* __restrict__ ro,
    double* __restrict__ al, double* __restrict__ q, NetDesc nd, float* __restrict__ img) {
  __shared__ double sh[LB_THREADS / 64];
  __shared__ int s_flag;
  if (st->done) return;
  const int tid = threadIdx.x;
  const int n_iter = st->n_iter + 1;
  int hist_len = st->hist_len, head = st->hist_head;
  double Hdiag = st->Hdiag;
  const double t_prev = st->t;

  if (n_iter == 1) {                                   // :90-95
    for (int i = tid; i < n; i += LB_THREADS) d[i] = -g[i];
    hist_len = 0; head = 0; Hdiag = 1.0;
  } else {
    // y = g - g_old, s = d*t  (:98-100); staged in q (y) and al-free scratch d stays d
    double ys_p = 0, yy_p = 0;
    for (int i = tid; i < n; i += LB_THREADS) {
      const double y = g[i] - g_old[i], s = d[i] * t_prev;
      ys_p += y * s; yy_p += y * y;
    }
    const double ys = block_sum(ys_p, sh);
    const double yy = block_sum(yy_p, sh);
    if (ys > 1e-10) {                                  // :102-114
      int slot;
      if (hist_len == n_corr) { slot = head; head = (head + 1) % n_corr; }
      else { slot = (head + hist_len) % n_corr; hist_len += 1; }
      for (int i = tid; i < n; i += LB_THREADS) {
        Sh[(size_t)slot * ring_ld(n) + i] = d[i] * t_prev;
        Yh[(size_t)slot * ring_ld(n) + i] = g[i] - g_old[i];
      }
      if (tid == 0) ro[slot] = 1.0 / ys;               // 1/dot(old_stps[i], old_dirs[i]) (:121-123)
      Hdiag = ys / yy;
    }
    __syncthreads();
    // two-loop recursion (:126-141); logical index i -> ring slot (head+i)%n_corr
    for (int i = tid; i < n; i += LB_THREADS) q[i] = -g[i];
    __syncthreads();
    for (int li = hist_len - 1; li >= 0; --li) {
      const int slot = (head + li) % n_corr;
      double p = 0;
      for (int i = tid; i < n; i += LB_THREADS) p += Sh[(size_t)slot * ring_ld(n) + i] * q[i];
      const double a = block_sum(p, sh) * ro[slot];
      if (tid == 0) al[slot] = a;
      for (int i = tid; i < n; i += LB_THREADS) q[i] -= a * Yh[(size_t)slot * ring_ld(n) + i];
      __syncthreads();
    }
    for (int i = tid; i < n; i += LB_THREADS) q[i] *= Hdiag;          // r = q*Hdiag
    __syncthreads();
    for (int li = 0; li < hist_len; ++li) {
      const int slot = (head + li) % n_corr;
      double p = 0;
      for (int i = tid; i < n; i += LB_THREADS) p += Yh[(size_t)slot * ring_ld(n) + i] * q[i];
      const double be = block_sum(p, sh) * ro[slot];
      const double co = al[slot] - be;
      for (int i = tid; i < n; i += LB_THREADS) q[i] += co * Sh[(size_t)slot * ring_ld(n) + i];
      __syncthreads();
    }
    for (int i = tid; i < n; i += LB_THREADS) d[i] = q[i];
  }
  __syncthreads();
  // g_old = g, f_old = f  (:143-145); gtd = g.d (:151)
  double gtd_p = 0, ga_p = 0;
  for (int i = tid; i < n; i += LB_THREADS) {
    const double gi = g[i];
    g_old[i] = gi;
    gtd_p += gi * d[i];
    ga_p += fabs(gi);
  }
  const double gtd = block_sum(gtd_p, sh);
  const double gabs = block_sum(ga_p, sh);
  if (tid == 0) s_flag = (gtd > -tol_x) ? 1 : 0;       // :154-156
  __syncthreads();
  if (s_flag) {
    if (tid == 0) {
      st->n_iter = n_iter; st->hist_len = hist_len; st->hist_head = head; st->Hdiag = Hdiag;
      st->f_old = st->f; st->done = 2;
    }
    return;
  }
  double t;                                            // :159-163
  if (n_iter == 1) { const double inv = 1.0 / gabs; t = inv < 1.0 ? inv : 1.0; }
  else t = lr;
  const bool will_eval = (n_iter != max_iter);         // :176
  for (int i = tid; i < n; i += LB_THREADS) {
    const double xi = x[i] + t * d[i];                 // :174
    x[i] = xi;
    if (will_eval) { theta[i] = xi; theta_r[i] = (real)xi; pack_store_any(nd, img, i, (float)xi); }
  }
  if (tid == 0) {
    st->n_iter = n_iter; st->hist_len = hist_len; st->hist_head = head; st->Hdiag = Hdiag;
    st->t = t; st->f_old = st->f;
    if (!will_eval) st->done = 1;                      // :192 (nIter == maxIter)
  }
}

// After the re-evaluation: bookkeeping and the break tests of custom_lbfgs.py:185-224.
__global__ __launch_bounds__(LB_THREADS) void k_lbfgs_post(
    int n, int n_theta, int max_iter, double max_eval, double tol_fun, double tol_x,
    LbfgsState* __restrict__ st, const double* __restrict__ gl, const double* __restrict__ d,
    int* __restrict__ log_iters, double* __restrict__ log_losses, int initial) {
  __shared__ double sh[LB_THREADS / 64];
  if (st->done) return;
  const int tid = threadIdx.x;
  const double f = gl[n_theta] + gl[n_theta + 1] + gl[n_theta + 2];
  double ga_p = 0, sa_p = 0;
  const double t = st->t;
  for (int i = tid; i < n; i += LB_THREADS) {
    ga_p += fabs(gl[i]);
    if (!initial) sa_p += fabs(d[i] * t);
  }
  const double gabs = block_sum(ga_p, sh);
  const double sabs = block_sum(sa_p, sh);
  if (tid != 0) return;
  if (initial) {                                       // :65-76
    st->f = f; st->func_eval = 1;
    if (gabs <= tol_fun) st->done = 7;
    return;
  }
  const double f_old = st->f_old;
  st->f = f;
  st->func_eval += 1;
  const int n_iter = st->n_iter;
  if (n_iter == max_iter) { st->done = 1; return; }    // :192 (unreachable: step sets it)
  if ((double)st->func_eval >= max_eval) { st->done = 3; return; }   // :195
  if (gabs <= tol_fun) { st->done = 4; return; }       // :200-203
  if (sabs <= tol_x) { st->done = 5; return; }         // :206-209
  if (fabs(f - f_old) < tol_x) { st->done = 6; return; }   // :212-215
  const int k = st->n_logged;                          // :217-218
  log_iters[k] = n_iter;
  log_losses[k] = f;
  st->n_logged = k + 1;
  if (n_iter == max_iter - 1) st->final_loss = f;      // :223-224
}

// ---------------------------------------------------------------------------------------------
// Compact L-BFGS: same iteration as k_lbfgs_step, restructured so that no kernel contains a
// chain of dependent full-length reductions.
//   k_lbc_dots   one workgroup per history slot (two, each on half of the vector, when n <= 4096): every dot product this iteration needs
//                (s_a.y_c, s_c.y_a, y_a.y_c, s_a.g, y_a.g, y_c.s_c, y_c.y_c, g.g, |g|_1, |t d|_1) in
//                parallel; also materialises the candidate pair s_c = t d, y_c = g - g_old.
//   k_lbc_coef_apply   (a) the bookkeeping/break tests of custom_lbfgs.py:185-224 for the evaluation
//                that precedes this iteration (k_lbfgs_post folded in, `do_post`);
//                (b) accepts the pair (y.s > 1e-10), maintains the Gram matrices
//                SY[a][b] = s_a.y_b, YY[a][b] = y_a.y_b, and runs the two-loop recursion of
//                custom_lbfgs.py:126-141 on *scalars* -- every vector of the recursion lives in
//                span{s_j, y_j, g}, so alpha_i/beta_i follow from the Gram entries alone.  One
//                lane per history slot; each lane carries the running sum it will need when its
//                turn comes, so a recursion step is: lane i finishes alpha_i -> broadcast ->
//                every lane does one fma.  No cross-lane reductions inside the loops.
//                Emits d = cg g + sum_j (cy_j y_j + cs_j s_j), gtd, the step t and the break flag.
//                (c) d, g_old, x += t d (and the model weights when an evaluation follows), in
//                the same launch: every workgroup repeats (a)-(b) and updates its own 64 weights.
// Mathematically identical to the reference recursion; rounding differs at the 1e-16 level.
// The ring has m+1 slots so that the candidate never overwrites a pair that may still be needed.
// ---------------------------------------------------------------------------------------------
struct LbcExtra {
  int apply, will_eval, pad0, pad1;
  double cg, gtd;
};

// pinn_lbfgs_begin clears nine device arrays (ring buffers, Gram matrices, coefficient vectors): one launch instead of
// nine hipMemsetAsync launches (each costs a launch floor, ~40 us together -- visible in the driver's 20-step blocks)
struct ZeroList {
  double* p[10];
  unsigned long long n[10];     // doubles
  int count;
  double* state;                // LbfgsState as doubles: all zero except Hdiag = 1 (custom_lbfgs.py:91-95), one thread
  int state_doubles, hdiag_index;
};
__global__ __launch_bounds__(256) void k_zero_list(ZeroList zl) {
  if (zl.state && blockIdx.x == 0 && threadIdx.x == 0)
    for (int i = 0; i < zl.state_doubles; ++i) zl.state[i] = i == zl.hdiag_index ? 1.0 : 0.0;
  for (int a = 0; a < zl.count; ++a) {
    double* __restrict__ p = zl.p[a];
    const unsigned long long n = zl.n[a];
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n;
         i += (unsigned long long)gridDim.x * 256)
      p[i] = 0.0;
  }
}

constexpr int LBC_THREADS = 1024;  // k_lbc_coef: 16 waves stage the Gram matrices, wave 0 runs the recursion
constexpr int LBC_ROWS = 4;        // ceil(62 / 16) matrix rows per thread
constexpr int LBD_THREADS = 1024;  // k_lbc_dots: n = 3021 is three strides of a 1024-thread block
constexpr int LBC_NSCAL = 5;       // trailing scalars of the dots array

// sums NV values over the block: DPP wave sums, one LDS exchange, wave totals added in index order
template <int NV>
__device__ __forceinline__ void block_sums(double (&v)[NV], double (*sh)[8]) {
  const int w = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const double t = wave_sum(v[i]);
    if ((threadIdx.x & 63) == 0) sh[w][i] = t;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    double t = 0;
#pragma unroll
    for (int k = 0; k < LBD_THREADS / 64; ++k) t += sh[k][i];
    v[i] = t;
  }
}

// dots layout: [0,M1) s_a.y_c | [M1,2M1) s_c.y_a | [2M1,3M1) y_a.y_c | [3M1,4M1) s_a.g |
//              [4M1,5M1) y_a.g | 5M1+0 y_c.s_c | +1 y_c.y_c | +2 g.g | +3 |g|_1 | +4 |t d|_1
// HALVES = 2 (n <= 4096): grid (M1, 2), workgroup (a, h) covers the pair stride h only and writes the partial set h
// (dots + h * (5 M1 + 5)); k_lbc_coef_apply adds the two sets.  Half the loads per CU again (5 per wave).
template <int HALVES>
__global__ __launch_bounds__(LBD_THREADS) void k_lbc_dots(
    int n, int M1, const LbfgsState* __restrict__ st, const double* __restrict__ g,
    const double* __restrict__ g_old, const double* __restrict__ d, double* __restrict__ Sh,
    double* __restrict__ Yh, double* __restrict__ dots_all) {
  __shared__ double sh[LBD_THREADS / 64][8];
  double* __restrict__ dots = dots_all + (HALVES == 2 ? blockIdx.y * (5 * M1 + LBC_NSCAL) : 0);
  const int u0 = HALVES == 2 ? (int)blockIdx.y : 0;
  // Thread t owns the element PAIRS {2t, 2t+1} + 2048 u, u < NS: every global access is 16 bytes per lane (the cost of
  // this kernel's one round of reads is the number of vector-memory instructions per CU, ~20 ticks each: 10 per wave
  // instead of 15 with one element per lane and three strides); ring rows are ring_ld(n) apart, so every pair is
  // 16-byte aligned.
  constexpr int NS = HALVES == 2 ? 1 : 2;         // pair strides of 2 x LBD_THREADS covered by this workgroup (n <= 4096 fast path)
  typedef double d2 __attribute__((ext_vector_type(2)));
  const int a = blockIdx.x, tid = threadIdx.x;
  const int done0 = st->done, head = st->hist_head, len = st->hist_len, n_it = st->n_iter;
  const double t = st->t;
  d2 gv[NS], gov[NS], dv[NS], sav[NS], yav[NS];
#pragma unroll
  for (int u = 0; u < NS; ++u) {
    const int i = 2 * tid + (u0 + u) * 2 * LBD_THREADS;
    const d2 z = {0.0, 0.0};
    gv[u] = gov[u] = dv[u] = sav[u] = yav[u] = z;
    if (i + 1 < n) {
      gv[u] = *reinterpret_cast<const d2*>(g + i); gov[u] = *reinterpret_cast<const d2*>(g_old + i);
      dv[u] = *reinterpret_cast<const d2*>(d + i);
      sav[u] = *reinterpret_cast<const d2*>(Sh + (size_t)a * ring_ld(n) + i);
      yav[u] = *reinterpret_cast<const d2*>(Yh + (size_t)a * ring_ld(n) + i);
    } else if (i < n) {
      gv[u].x = g[i]; gov[u].x = g_old[i]; dv[u].x = d[i]; sav[u].x = Sh[(size_t)a * ring_ld(n) + i]; yav[u].x = Yh[(size_t)a * ring_ld(n) + i];
      if (i + 1 < n) {
        gv[u].y = g[i + 1]; gov[u].y = g_old[i + 1]; dv[u].y = d[i + 1];
        sav[u].y = Sh[(size_t)a * ring_ld(n) + i + 1]; yav[u].y = Yh[(size_t)a * ring_ld(n) + i + 1];
      }
    }
  }
  if (done0) return;
  const bool first = (n_it == 0);
  int c = head + len; if (c >= M1) c -= M1;
  int pos = a - head; if (pos < 0) pos += M1;
  if (a == c) {
    double v[7] = {0, 0, 0, 0, 0, 0, 0};          // ys yy sg yg gg ga sa
    auto one = [&](const int i, const double gi, const double go, const double di) {
      if (i < n) {
        v[4] += gi * gi; v[5] += fabs(gi);
        if (!first) {
          const double y = gi - go, s = di * t;
          Sh[(size_t)c * ring_ld(n) + i] = s; Yh[(size_t)c * ring_ld(n) + i] = y;
          v[0] += y * s; v[1] += y * y; v[2] += s * gi; v[3] += y * gi; v[6] += fabs(s);
        }
      }
    };
#pragma unroll
    for (int u = 0; u < NS; ++u) {
      const int i = 2 * tid + (u0 + u) * 2 * LBD_THREADS;
      one(i, gv[u].x, gov[u].x, dv[u].x);
      one(i + 1, gv[u].y, gov[u].y, dv[u].y);
    }
    if (HALVES == 1)
      for (int i = tid + NS * 2 * LBD_THREADS; i < n; i += LBD_THREADS) one(i, g[i], g_old[i], d[i]);   // n > 4096: plain loop
    block_sums(v, sh);
    if (tid == 0) {
      dots[5 * M1 + 0] = v[0]; dots[5 * M1 + 1] = v[1]; dots[5 * M1 + 2] = v[4]; dots[5 * M1 + 3] = v[5];
      dots[5 * M1 + 4] = v[6];
      dots[3 * M1 + c] = v[2]; dots[4 * M1 + c] = v[3];
    }
  } else if (pos < len) {
    double v[5] = {0, 0, 0, 0, 0};                // say sya yya sg yg
    auto one = [&](const double gi, const double go, const double di, const double sa, const double ya) {
      const double yc = gi - go, sc = di * t;
      v[0] += sa * yc; v[1] += sc * ya; v[2] += ya * yc; v[3] += sa * gi; v[4] += ya * gi;
    };
#pragma unroll
    for (int u = 0; u < NS; ++u) {                // (elements beyond n hold zeros: no guard needed)
      one(gv[u].x, gov[u].x, dv[u].x, sav[u].x, yav[u].x);
      one(gv[u].y, gov[u].y, dv[u].y, sav[u].y, yav[u].y);
    }
    if (HALVES == 1)
      for (int i = tid + NS * 2 * LBD_THREADS; i < n; i += LBD_THREADS)
        one(g[i], g_old[i], d[i], Sh[(size_t)a * ring_ld(n) + i], Yh[(size_t)a * ring_ld(n) + i]);
    block_sums(v, sh);
    if (tid == 0) {
      dots[a] = v[0]; dots[M1 + a] = v[1]; dots[2 * M1 + a] = v[2];
      dots[3 * M1 + a] = v[3]; dots[4 * M1 + a] = v[4];
    }
  }
}

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }


#ifdef PINN_STAMPS
__device__ long long g_coef_stamps[16];         // s_memtime timeline of the last k_lbc_coef (profiling build)
#define CSTAMP(i) do { if (threadIdx.x == 0 && blockIdx.x == 0) g_coef_stamps[i] = clock64(); } while (0)
#else
#define CSTAMP(i) do { } while (0)
#endif
inline int lbc_ld(int M1) { return M1 | 1; }     // odd leading dimension: column walks hit distinct banks
static_assert((62 | 1) <= 62 + 1 && 64 - 1 < 6 * 64, "k_lbc_coef_apply: unclamped column reads stay inside initialised LDS");
constexpr int LBC_MAXSLOTS = 62;                  // one lane per ring slot

// k_lbc_coef_apply: the scalar two-loop recursion AND the vector update in ONE launch.
// Every workgroup (one per 64 weights) repeats the O(m^2) recursion redundantly -- it is the same
// deterministic code on the same inputs, so all workgroups hold identical coefficients without any
// inter-workgroup communication -- and then updates its own 64 weights.  Workgroup 0 alone writes
// the new optimiser state; because the others may still be reading the old one, state, Gram
// matrices and ro are double buffered (read *_in, write *_out; the host flips per iteration).
//
// The recursion runs in *position* space (p = 0 oldest pair ... len-1 newest; lane = position), on
// three LDS matrices prepared while staging so that a recursion step is exactly
// {broadcast, fma, fma} with immediate-offset operands and no select:
//   sU[p][j] = ro_p (s_p.y_j) for j > p, else 0    backward: b_p -= al_j sU[p][j]; b_p is final (= al_p)
//   sY[p][j] = y_p.y_j                              backward: y_p.q_0 -= al_j sY[p][j]
//   sL[p][j] = ro_p (s_j.y_p) for j < p, else 0    forward:  e_p -= cs_j sL[p][j]; e_p is final (= cs_p)
// (the zeros freeze a lane's value once its own step has passed).  Global reads stay in ring-slot
// order and are issued as one round (wave 0 includes its operands of the update; waves 1-15 fetch theirs while wave 0 runs
// the recursion); the rotation by
// `head` happens in the LDS write addresses.
// d = cg g + sum_j (cy_j y_j + cs_j s_j) is summed over ring *slots* (zero coefficients for slots not
// in use, ring zeroed at begin), 64 elements x 16 slices per workgroup, fixed order.
template <typename real>
__global__ __launch_bounds__(LBC_THREADS) void k_lbc_coef_apply(
    int n, int M1, int m, int max_iter, double lr, double tol_x, double tol_fun, double max_eval,
    int do_post, int n_theta, const LbfgsState* __restrict__ st_in, LbfgsState* __restrict__ st_out,
    const double* __restrict__ gl, const double* __restrict__ pd, int n_part,
    const double* __restrict__ SY_in, const double* __restrict__ YY_in, const double* __restrict__ ro_in,
    double* __restrict__ SY_out, double* __restrict__ YY_out, double* __restrict__ ro_out,
    int* __restrict__ log_iters, double* __restrict__ log_losses,
    const double* __restrict__ Sh, const double* __restrict__ Yh, double* __restrict__ d,
    double* __restrict__ g_old, double* __restrict__ x, double* __restrict__ theta,
    real* __restrict__ theta_r, NetDesc nd, float* __restrict__ img) {
  extern __shared__ double lsh[];
  const int tid = threadIdx.x, lane = tid & 63, wave = uni(tid >> 6);
  const bool writer = blockIdx.x == 0;
  const int LD = M1 | 1;
  double* const sU = lsh;
  double* const sL = sU + M1 * LD;
  double* const sY = sL + M1 * LD;
  double* const sT = sY + M1 * LD;                 // 6 x 64 per-slot vectors: say sya yya sg yg ro
  double* const sC = sT + 6 * 64;                  // cs[64] | cy[64] | {t, cg, apply, will_eval}
  double* const sP = sC + 192;                     // [16][64] partial sums of the update
  double* const sZ = sP + 16 * 64;                 // 64 zeros: the matrix row of the lanes beyond M1
  CSTAMP(0);
  // ---- every global read the recursion waits for, issued as ONE round (a dependent round costs 1.5-2 us; the round itself
  // costs ~20 ticks per vector-memory instruction of the workgroup, so nothing is loaded twice and nothing early)
  const bool in_row = lane < M1;
  const LbfgsState s0 = *st_in;
  int head = uni(s0.hist_head), len = uni(s0.hist_len);
  double Hdiag = s0.Hdiag, f_cur = s0.f;
  // The dot products: one set (k_lbc_dots<1>) or its two halves (k_lbc_dots<2>); waves 0-4 fetch one per-slot vector
  // each, everybody the five scalars.
  // (Predicated loads, not clamped ones: a skipped load costs a branch, a redundant one a slot of the CU's memory
  //  pipeline -- with every lane loading, this round went from 6.5 k to 15 k ticks.)
  // (Built and dropped in round 3: a two-launch tail whose reduction kernel also formed per-tile partial dot products,
  //  summed here -- parity-green, 54.67 vs 54.54 us per iteration, profiles/r03_lbfgs_tail.txt; git history.)
  const int ndp = 5 * M1 + LBC_NSCAL;
  double ys = pd[5 * M1 + 0], yy = pd[5 * M1 + 1], gg = pd[5 * M1 + 2], gabs = pd[5 * M1 + 3], sabs = pd[5 * M1 + 4];
  double qv = (wave < 5 && in_row) ? pd[wave * M1 + lane] : 0.0;
  if (n_part == 2) {                                 // k_lbc_dots<2>: the two halves of every dot product
    const double* __restrict__ p2 = pd + ndp;
    ys += p2[5 * M1 + 0]; yy += p2[5 * M1 + 1]; gg += p2[5 * M1 + 2]; gabs += p2[5 * M1 + 3]; sabs += p2[5 * M1 + 4];
    qv += (wave < 5 && in_row) ? p2[wave * M1 + lane] : 0.0;
  }
  const double ro_l0 = in_row ? ro_in[lane] : 0.0;
  const double f_new = gl[n_theta] + gl[n_theta + 1] + gl[n_theta + 2];
  // (Tried: both Gram matrices read flat, 16 bytes per lane -- 42 load instructions per workgroup instead of 128 --
  //  with the staging done element by element: 53.81 vs 53.59 us per iteration, no gain, reverted.)
  double ra[LBC_ROWS], rb[LBC_ROWS];
#pragma unroll
  for (int u = 0; u < LBC_ROWS; ++u) {
    const int r = wave + 16 * u;
    const bool ok = r < M1 && in_row;
    ra[u] = ok ? SY_in[r * M1 + lane] : 0.0;
    rb[u] = ok ? YY_in[r * M1 + lane] : 0.0;
  }
  // vector operands of the update: element i = 64 blockIdx + lane, slice = wave (slots wave + 16u)
  const int i = blockIdx.x * 64 + lane;
  const bool iok = i < n;
  const double gi = (iok && wave == 0) ? gl[i] : 0.0, xi0 = (iok && wave == 0) ? x[i] : 0.0;
  // the history tile is needed by the update only: wave 0 (which goes straight into the recursion) fetches its
  // slice here, waves 1-15 fetch theirs while wave 0 runs the recursion -- 90 fewer loads in the round every other
  // phase waits for
  double yv[4] = {0.0, 0.0, 0.0, 0.0}, sv[4] = {0.0, 0.0, 0.0, 0.0};
  auto fetch_history = [&]() {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int sl = wave + 16 * u;
      const bool ok = iok && sl < M1;
      yv[u] = ok ? Yh[(size_t)sl * ring_ld(n) + i] : 0.0;
      sv[u] = ok ? Sh[(size_t)sl * ring_ld(n) + i] : 0.0;
    }
  };
  if (wave == 0) fetch_history();
  const int done0 = uni(s0.done);
  if (done0) { if (writer && tid == 0) *st_out = s0; return; }
  CSTAMP(1);
  LbfgsState s1 = s0;                              // the state after this iteration (written by `writer`)
  int dn = 0;
  if (do_post) {                                   // custom_lbfgs.py:185-215 for the last evaluation
    f_cur = f_new;
    if (s0.n_iter == max_iter) dn = 1;
    else if ((double)(s0.func_eval + 1) >= max_eval) dn = 3;
    else if (gabs <= tol_fun) dn = 4;
    else if (sabs <= tol_x) dn = 5;
    else if (fabs(f_cur - s0.f_old) < tol_x) dn = 6;
    s1.f = f_cur; s1.func_eval = s0.func_eval + 1;
    if (dn) s1.done = dn;
    else {                                         // :217-224
      if (writer && tid == 0) { log_iters[s0.n_logged] = s0.n_iter; log_losses[s0.n_logged] = f_cur; }
      s1.n_logged = s0.n_logged + 1;
      if (s0.n_iter == max_iter - 1) s1.final_loss = f_cur;
    }
  }
  if (dn) { if (writer && tid == 0) *st_out = s1; return; }

  const int n_iter = s0.n_iter + 1;
  const bool first = (n_iter == 1);
  int c = head + len; if (c >= M1) c -= M1;
  const bool accept = !first && ys > 1e-10;        // custom_lbfgs.py:102-114
  if (accept) {
    Hdiag = ys / yy;
    if (len == m) { head += 1; if (head >= M1) head -= M1; } else len += 1;
  }
  const double ro_l = (accept && lane == c) ? 1.0 / ys : ro_l0;
  if (wave < 5) sT[wave * 64 + lane] = !in_row ? 0.0 : qv;   // per-slot vectors: say sya yya sg yg
  if (wave == 5) {
    sT[5 * 64 + lane] = ro_l;
    if (writer && in_row) ro_out[lane] = ro_l;
    sZ[lane] = 0.0;
  }
  if (wave == 1 && LD > M1 && in_row) {            // pad column of the three matrices (read, times zero, by the recursion)
    sU[lane * LD + M1] = 0.0; sL[lane * LD + M1] = 0.0; sY[lane * LD + M1] = 0.0;
  }
  lds_barrier();     // LDS-only: must not wait for global stores
  CSTAMP(2);
  {  // patch the candidate row/column, scale, mask, rotate, stage (branch-free per row)
    int pb = lane - head; if (pb < 0) pb += M1;
    const bool vb = in_row && pb < len;
    const bool lc = accept && lane == c;
    const double d_sya = sT[1 * 64 + lane], d_yya = sT[2 * 64 + lane];
    double ro_r[LBC_ROWS], say_r[LBC_ROWS], yya_r[LBC_ROWS];   // LDS reads before LDS writes
#pragma unroll
    for (int u = 0; u < LBC_ROWS; ++u) {
      const int r = wave + 16 * u, rr = r < M1 ? r : 0;
      ro_r[u] = sT[5 * 64 + rr]; say_r[u] = sT[0 * 64 + rr]; yya_r[u] = sT[2 * 64 + rr];
    }
#pragma unroll
    for (int u = 0; u < LBC_ROWS; ++u) {
      const int r = wave + 16 * u;                  // wave-uniform
      if (r < M1) {
        const bool rc = accept && r == c;
        const double sy = rc ? (lc ? ys : d_sya) : (lc ? say_r[u] : ra[u]);   // s_c.y_l | s_r.y_c | stored
        const double y2 = rc ? (lc ? yy : d_yya) : (lc ? yya_r[u] : rb[u]);
        int pa = r - head; if (pa < 0) pa += M1;
        const bool both = vb && pa < len;
        const double vu = (both && pb > pa) ? ro_r[u] * sy : 0.0;
        const double vy = both ? y2 : 0.0;
        const double vl = (both && pa < pb) ? ro_l * sy : 0.0;
        if (in_row) {
          sU[pa * LD + pb] = vu; sY[pa * LD + pb] = vy; sL[pb * LD + pa] = vl;
          if (writer) { SY_out[r * M1 + lane] = sy; YY_out[r * M1 + lane] = y2; }
        }
      }
    }
  }
  lds_barrier();
  if (wave == 0) {
    CSTAMP(3);
    // lane = position p
    int slot = lane + head; if (slot >= M1) slot -= M1;
    const bool valid = lane < len;
    const int sidx = in_row ? slot : 0;
    const double sg_p = valid ? sT[3 * 64 + sidx] : 0.0, yg_p = valid ? sT[4 * 64 + sidx] : 0.0;
    const double ro_p = valid ? sT[5 * 64 + sidx] : 0.0;
    const double* __restrict__ rowU = in_row ? sU + lane * LD : sZ;     // lanes >= M1 read a row of zeros
    const double* __restrict__ rowY = in_row ? sY + lane * LD : sZ;
    const double* __restrict__ rowL = in_row ? sL + lane * LD : sZ;
    // Both loops run in chunks of 8 steps: a chunk is straight-line code (its 8-16 LDS operands are
    // fetched together, ahead of the dependent broadcast->fma chain) and is skipped as a whole when
    // it lies beyond len.  Steps in [len, 64) inside the last chunk are harmless: their lanes hold
    // exact zeros (lanes >= M1 because their operands are forced to zero) and their matrix columns are zero.
    // A step is exactly {v_readlane x2 -> v_fma_f64}: NOTHING scalar sits between the broadcast and the fma.  A
    // select or a branch on the lane index inside the chain costs as much as the broadcast itself
    // (profiles/ubench/chain_latency.hip: 24.8 -> 48.5 ticks per step; the guarded loops ran at 100 / 76).
    // backward loop (custom_lbfgs.py:130-133): al_i = ro_i s_i.q_i, q_i = -g - sum_{j>i} al_j y_j
    double bacc = ro_p * -sg_p, yq0 = -yg_p;
    constexpr int NCH = (LBC_MAXSLOTS + 7) / 8;
    const int top = uni((len + 7) >> 3) - 1;          // last chunk in use (-1: empty history)
    // Operands: two register sets, alternating; those of chunk c8 - 1 are fetched one pair per step INSIDE the chain
    // of chunk c8 (a lone wave issues in order: the fetches fill the slots in which the chain waits for its
    // broadcast; fetched in a block ahead of the chain they cost ~40 ticks per step).  Column indices run to
    // 8 * NCH - 1 = 63 without a clamp (immediate offsets): beyond M1 they read the pad column (zeroed above), the
    // first elements of the next row or of the next staged array -- finite values, multiplied by a lane that holds 0.
    // What that rests on: (1) LD = lbc_ld(M1) = M1 | 1 <= M1 + 1, so a row's overrun [M1, 64) lands in the
    // following rows of the SAME matrix, all of whose cells (pad column included) are written while staging; (2) the
    // staging order sU, sL, sY, sT: the overrun of a matrix's last rows lands in the next matrix, and that of sY in
    // sT, whose 6 x 64 entries are all written (zeros for lanes >= M1) -- 64 - M1 <= 63 < 384; (3) every staged value
    // is finite whenever the history is (ro = 1 / y.s with y.s > 1e-10): a non-finite history has already made the
    // loss non-finite (pinn_get_status reports it), a product 0 x Inf here changes nothing that was still valid.
    double ub[2][8], yb[2][8];
#pragma unroll
    for (int c8 = NCH - 1; c8 >= 0; --c8) {
      if (c8 <= top) {
        if (c8 == top) {
#pragma unroll
          for (int k = 0; k < 8; ++k) { ub[c8 & 1][k] = rowU[8 * c8 + k]; yb[c8 & 1][k] = rowY[8 * c8 + k]; }
        }
#pragma unroll
        for (int k = 7; k >= 0; --k) {
          const double al_i = read_lane(bacc, 8 * c8 + k);
          bacc -= al_i * ub[c8 & 1][k];
          yq0 -= al_i * yb[c8 & 1][k];
          if (c8 > 0) { ub[(c8 - 1) & 1][k] = rowU[8 * (c8 - 1) + k]; yb[(c8 - 1) & 1][k] = rowY[8 * (c8 - 1) + k]; }
          __builtin_amdgcn_sched_group_barrier(0x2, 2, 0);      // broadcast
          __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);    // the two fetches sit in the broadcast's hazard slots
          __builtin_amdgcn_sched_group_barrier(0x2, 2, 0);      // fma, fma
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
    const double al = bacc;
    CSTAMP(4);
    // forward loop (:136-139): be_i = ro_i y_i.(Hdiag q_0 + sum_{j<i} cs_j s_j), cs_i = al_i - be_i
    double eacc = al - ro_p * (Hdiag * yq0);
    double lb[2][8];
    if (top >= 0) {
#pragma unroll
      for (int k = 0; k < 8; ++k) lb[0][k] = rowL[k];
    }
#pragma unroll
    for (int c8 = 0; c8 < NCH; ++c8) {
      if (c8 <= top) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const double c_i = read_lane(eacc, 8 * c8 + k);
          eacc -= c_i * lb[c8 & 1][k];
          if (c8 + 1 < NCH) lb[(c8 + 1) & 1][k] = rowL[8 * (c8 + 1) + k];     // (chunk top + 1: finite, never used)
          __builtin_amdgcn_sched_group_barrier(0x2, 2, 0);
          __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x2, 1, 0);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
    CSTAMP(5);
    const double cs = eacc;
    const double cy = -Hdiag * al;
    const double cg = -Hdiag;
    const double gtd = cg * gg + wave_sum(valid ? (cy * yg_p + cs * sg_p) : 0.0);
    sC[lane] = 0.0; sC[64 + lane] = 0.0;
    if (in_row) { sC[slot] = valid ? cs : 0.0; sC[64 + slot] = valid ? cy : 0.0; }
    if (lane == 0) {
      s1.n_iter = n_iter; s1.hist_len = len; s1.hist_head = head; s1.Hdiag = Hdiag;
      s1.f_old = f_cur;
      double apply = 0.0, will_eval = 0.0, t = s0.t;
      if (gtd > -tol_x) {                          // custom_lbfgs.py:154-156
        s1.done = 2;
      } else {
        if (first) { const double inv = 1.0 / gabs; t = inv < 1.0 ? inv : 1.0; } else t = lr;
        s1.t = t;
        apply = 1.0;
        will_eval = (n_iter != max_iter) ? 1.0 : 0.0;
        if (n_iter == max_iter) s1.done = 1;       // :192
      }
      sC[128] = t; sC[129] = cg; sC[130] = apply; sC[131] = will_eval;
      if (writer) *st_out = s1;
    }
    CSTAMP(6);
  } else {
    fetch_history();
  }
  lds_barrier();
  // ---- the update of this workgroup's 64 elements
  if (sC[130] == 0.0) return;
  double p = 0.0;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int sl = wave + 16 * u;
    if (sl < M1) p += sC[64 + sl] * yv[u] + sC[sl] * sv[u];
  }
  sP[wave * 64 + lane] = p;
  lds_barrier();
  if (wave != 0 || !iok) return;
  double hist = 0.0;
#pragma unroll
  for (int k = 0; k < 16; ++k) hist += sP[k * 64 + lane];
  const double t = sC[128], di = sC[129] * gi + hist;
  d[i] = di;
  g_old[i] = gi;
  const double xi = xi0 + t * di;
  x[i] = xi;
  if (sC[131] != 0.0) { theta[i] = xi; theta_r[i] = (real)xi; pack_store_any(nd, img, i, (float)xi); }
}

inline size_t lbc_coef_apply_lds_bytes(int M1) { return ((size_t)3 * M1 * lbc_ld(M1) + 6 * 64 + 192 + 16 * 64 + 64) * 8; }

}  // namespace pinn
