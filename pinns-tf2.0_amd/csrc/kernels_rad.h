// kernels_rad.h -- residual-based adaptive collocation (RAD, Wu et al. 2023) on the device: pinn_rad_collocation.
//
// A pool P_0..P_{M-1} (points of the M-point Latin hypercube, k_lhs_fill) and its residuals f_i (forward_taylor +
// k_residual, exactly what pinn_residual_at returns) are turned into a sampling density p(x) ~ |f|^k / mean|f|^k + c:
//     a_i = m_i^k            m_i = |f_i| (Schrodinger: sqrt(f_u^2 + f_v^2)); k - 1 products, no contraction;
//                            a non-finite a_i counts as 0
//     A   = max a_i          (non-negative doubles order like their bit patterns: an integer atomic max, order-free)
//     q_i = floor(a_i / A * 2^32)       (A = 0: q_i = 1, r = 0 -- uniform over the pool)
//     r   = floor(c * (double)Q / (double)M),  Q = sum q_i
//     w_i = q_i + r,  cum_i = sum_{l <= i} w_l,  W = cum_{M-1} < 2^63 (M <= 2^24, c <= 64)
// Sample j takes U = Philox4x32-10((j_lo, j_hi, 0, 0x52414421), seed) -> (ctr0 << 32) | ctr1, T = floor(U W / 2^64)
// and the smallest i with cum_i > T: with replacement, so a drawn set may hold a pool point more than once.
// Everything after a_i is integer arithmetic, so no summation order can change a bit: a data-parallel rank draws its
// slice [first, first + count) of the one design without communication.  tests/helpers/rad_ref.py restates it in numpy.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "kernels_sampling.h"

namespace pinn {

constexpr int RAD_BLOCK = 256;        // pool points per workgroup of k_rad_mag / k_rad_q (one block sum each)
constexpr int RAD_SCAN = 1024;        // threads of k_rad_scan
constexpr int64_t RAD_POOL_MAX = 1 << 24;

// device-side totals of one draw
struct RadTotals {
  unsigned long long amax;            // bit pattern of A (zeroed before k_rad_mag)
  unsigned long long Q, r, W;
};

// a_i -> a[i] (bit pattern), A -> t->amax
__global__ __launch_bounds__(RAD_BLOCK) void k_rad_mag(const double* __restrict__ f, int n_out, int64_t M, int k,
                                                       unsigned long long* __restrict__ a, RadTotals* __restrict__ t) {
  // hipcc contracts by default, and the _rn intrinsics are inline operators that carry the contraction flag of their
  // header: f_u^2 + f_v^2 is written out here, under contract(off), so that it stays two roundings
#pragma clang fp contract(off)
  __shared__ unsigned long long red[RAD_BLOCK];
  const int64_t i = (int64_t)blockIdx.x * RAD_BLOCK + threadIdx.x;
  double v = 0.0;
  if (i < M) {
    double m;
    if (n_out == 2) {
      const double fu = f[2 * i], fv = f[2 * i + 1];
      const double uu = fu * fu, vv = fv * fv;
      m = __dsqrt_rn(uu + vv);
    } else {
      m = fabs(f[i]);
    }
    v = m;
    for (int p = 1; p < k; ++p) v = __dmul_rn(v, m);
    if (!isfinite(v)) v = 0.0;
    a[i] = (unsigned long long)__double_as_longlong(v);
  }
  red[threadIdx.x] = (unsigned long long)__double_as_longlong(v);
  __syncthreads();
  for (int s = RAD_BLOCK / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s && red[threadIdx.x + s] > red[threadIdx.x]) red[threadIdx.x] = red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0 && red[0] != 0ull) atomicMax(&t->amax, red[0]);
}

// q_i -> w[i] as the inclusive prefix sum within its block; the block's sum -> bsum[blockIdx.x]
__global__ __launch_bounds__(RAD_BLOCK) void k_rad_q(unsigned long long* __restrict__ w, int64_t M,
                                                     const RadTotals* __restrict__ t,
                                                     unsigned long long* __restrict__ bsum) {
  __shared__ unsigned long long sc[RAD_BLOCK];
  const int64_t i = (int64_t)blockIdx.x * RAD_BLOCK + threadIdx.x;
  const double A = __longlong_as_double((long long)t->amax);
  unsigned long long q = 0;
  if (i < M) {
    if (A == 0.0) {
      q = 1;
    } else {
      const double a = __longlong_as_double((long long)w[i]);
      q = __double2ull_rz(__dmul_rn(__ddiv_rn(a, A), 4294967296.0));
    }
  }
  sc[threadIdx.x] = q;
  __syncthreads();
  for (int s = 1; s < RAD_BLOCK; s <<= 1) {
    const unsigned long long add = (int)threadIdx.x >= s ? sc[threadIdx.x - s] : 0ull;
    __syncthreads();
    sc[threadIdx.x] += add;
    __syncthreads();
  }
  if (i < M) w[i] = sc[threadIdx.x];
  if (threadIdx.x == RAD_BLOCK - 1) bsum[blockIdx.x] = sc[RAD_BLOCK - 1];
}

// one workgroup: bsum[0, nb) -> exclusive prefix sums in place; Q, r, W -> t
__global__ __launch_bounds__(RAD_SCAN) void k_rad_scan(unsigned long long* __restrict__ bsum, int nb, int64_t M,
                                                       double c_add, RadTotals* __restrict__ t) {
  __shared__ unsigned long long sc[RAD_SCAN];
  unsigned long long carry = 0;
  for (int base = 0; base < nb; base += RAD_SCAN) {
    const int b = base + (int)threadIdx.x;
    const unsigned long long v = b < nb ? bsum[b] : 0ull;
    sc[threadIdx.x] = v;
    __syncthreads();
    for (int s = 1; s < RAD_SCAN; s <<= 1) {
      const unsigned long long add = (int)threadIdx.x >= s ? sc[threadIdx.x - s] : 0ull;
      __syncthreads();
      sc[threadIdx.x] += add;
      __syncthreads();
    }
    if (b < nb) bsum[b] = carry + sc[threadIdx.x] - v;
    carry += sc[RAD_SCAN - 1];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const unsigned long long Q = carry;
    unsigned long long r = 0;
    if (t->amax != 0ull) r = __double2ull_rz(__ddiv_rn(__dmul_rn(c_add, __ull2double_rn(Q)), (double)M));
    t->Q = Q;
    t->r = r;
    t->W = Q + (unsigned long long)M * r;
  }
}

// samples [first, first + count): slot s = j - first <- P_idx (compute dtype into xs/ts, float64 into cx/ct)
template <typename real>
__global__ __launch_bounds__(256) void k_rad_select(const real* __restrict__ px, const real* __restrict__ pt,
                                                    const unsigned long long* __restrict__ w,
                                                    const unsigned long long* __restrict__ boff,
                                                    const RadTotals* __restrict__ t, int64_t M, uint64_t first,
                                                    int64_t count, uint32_t seed_lo, uint32_t seed_hi,
                                                    real* __restrict__ xs, real* __restrict__ ts,
                                                    double* __restrict__ cx, double* __restrict__ ct) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= count) return;
  const uint64_t j = first + (uint64_t)s;
  uint32_t ctr[4] = {(uint32_t)j, (uint32_t)(j >> 32), 0u, 0x52414421u};
  philox4x32_10(ctr, seed_lo, seed_hi);
  const unsigned long long U = ((unsigned long long)ctr[0] << 32) | ctr[1];
  const unsigned long long r = t->r;
  const unsigned long long T = __umul64hi(U, t->W);
  // smallest i with cum_i > T, cum_i = w[i] + boff[i / RAD_BLOCK] + (i + 1) r (non-decreasing; cum_{M-1} = W > T)
  int64_t lo = 0, hi = M - 1;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    const unsigned long long cum = w[mid] + boff[mid / RAD_BLOCK] + (unsigned long long)(mid + 1) * r;
    if (cum > T) hi = mid; else lo = mid + 1;
  }
  const real x = px[lo], tt = pt[lo];
  xs[s] = x;
  ts[s] = tt;
  cx[s] = (double)x;
  ct[s] = (double)tt;
}

}  // namespace pinn
