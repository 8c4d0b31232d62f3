// kernels_generic.h -- shape-generic loss+gradient kernels (any uniform hidden width <= 128,
// 1 or 2 outputs, all three PDE kinds).  One lane = one point; weights are wave-uniform and
// are fetched through the scalar cache (s_load) so every FMA is VGPR x SGPR; the per-layer
// Taylor channels (a, z_x, z_t, z_xx) are stashed in an HBM/L2-resident scratch laid out
// [layer][feature][point] so that a wave's access is one contiguous 1 KiB (f32) line.
//
// Math: SURVEY.md Appendix A (4-channel forward A.1, seeds A.2, reverse sweep A.3), which
// is what the reference's nested GradientTapes compute
// (1d-burgers/inf_cont_burgers.py:65-90, utils/neuralnetwork.py:55-59).
#pragma once
#include <type_traits>
#include "pointsets.h"
#include "wave.h"

namespace pinn {

constexpr int MAX_DENSE = 16;   // dense layers incl. the linear output layer
constexpr int MAX_WIDTH = 128;

struct NetDesc {
  int n_hidden;              // H tanh layers, all of width W
  int width;                 // W
  int n_out;                 // 1 (Burgers) or 2 (Schrodinger)
  int off_w[MAX_DENSE];      // offsets into the flat weight vector (reference layout)
  int off_b[MAX_DENSE];
  int n_net;                 // number of network scalars (without lambdas)
  int n_theta;               // n_net (+2 for identification, +6 for PDE_ADR_IDE: pde_n_tail)
  int img_kind;              // packed weight image kept by the optimiser kernels: 0 none, 1 k_fused20m, 2 wide
};

// (SetDesc, the training-set geometry every kernel takes, stands in pointsets.h)

// Template number of the advection-diffusion-reaction kind (PINN_PDE_ADR = 5 of the C interface; the enum's 3 and 4 are the
// discrete-time models of kernels_disc.h, which are no template values of the continuous kernels):
//   f = u_t + (a0 + a1 u) u_x - nu u_xx + r1 u + r2 u^2 + r3 u^3
// Its six run-time coefficients travel where the other kinds pass the scalar nu (pde_coef_t), so the argument list of
// every other instantiation is what it was.  Boundary pairs of this kind are stored pair-interleaved,
// [lo_0, hi_0, lo_1, hi_1, ...]: the partner of point g is g ^ 1.
constexpr int PDE_ADR = 3;
// Template number of the same equation with TRAINABLE coefficients (PINN_PDE_ADR_IDE = 6 of the C interface): the six
// coefficients are the tail of the weight vector, th[n_net + k] = a0, a1, log nu, r1, r2, r3 (nu = exp keeps it positive, as
// PDE == 1 parametrises Burgers' viscosity), read by the kernels where PDE == 1 reads its two lambdas.  In the place of the
// scalar nu travels one int: bit k set = coefficient k is trained; the gradient entry of a frozen coefficient is written
// as exactly 0.0 (the optimisers then leave it where it is: Adam's m and v stay 0, every L-BFGS direction is 0 there).
//   enum -> template value:  PINN_PDE_ADR 5 -> PDE_ADR 3,  PINN_PDE_ADR_IDE 6 -> PDE_ADR_IDE 4
constexpr int PDE_ADR_IDE = 4;
// Template number of PINN_PDE_ADR with Robin points present (pinn_set_robin): PDE_ADR's kernels with a fourth point class,
//   r_j = alpha_j u + beta_j u_x - g_j,   loss part (1 / N_w) sum r_j^2 added to the boundary part.
// The class is a block of its own BEHIND the collocation block, [pairs | data | collocation | robin | pad]: SetDesc and every
// offset of the other classes stay what they are (sd.n_all still ends the collocation block; n_pad covers the Robin block).
// Where PDE_ADR passes its six coefficients travels AdrRobinArg: the coefficients, the (alpha, beta) pairs indexed by point -
// first, the block's first point and length and 1 / N_w; g_j rides in tgt at the point's own index.  A template value of
// its own, not a flag: no instantiation of another kind changes its name, its arguments or an instruction.  The engine
// dispatches here only while the local Robin count is > 0.
constexpr int PDE_ADR_ROBIN = 5;
// Template number of PINN_PDE_ADR with a source term present (pinn_set_source): the residual of collocation point i is
//   f_i = u_t + (a0 + a1 u) u_x - nu u_xx + r1 u + r2 u^2 + r3 u^3 - s_i,
// s_i riding in tgt at the point's own index (data targets and the Robin g_j ride there already; the slots of the
// collocation block are zero otherwise).  No seed formula changes: df/d(u, u_x, u_t, u_xx) do not depend on s.  A superset of
// PDE_ADR_ROBIN -- AdrSrcArg is AdrRobinArg and a source pointer, the Robin count may be 0 -- so a source with Robin walls needs
// no second family.  The subtraction is an operation of its own, never contracted into f: a zero source gives PDE_ADR's bits.
// The engine dispatches here only while a source is present.
constexpr int PDE_ADR_SRC = 6;
// Template number of PINN_PDE_ADR with per-point coefficient fields present (pinn_set_coef_fields): local collocation point i
// has a row of its own, K_i = (a0, a1, nu, r1, r2, r3)_i, and
//   f_i = u_t + (a0_i + a1_i u) u_x - nu_i u_xx + r1_i u + r2_i u^2 + r3_i u^3 - s_i;
// the seeds are PDE_ADR's with K_i where the constants stand.  The table is dense, [n_f][6] in the compute dtype, indexed by
// the point's place in the collocation block (point - 2 n_b - n_u): only a collocation point may read it.  A superset of
// PDE_ADR_SRC -- AdrVarArg is AdrSrcArg and the table's address; the Robin count may be 0 and the collocation slots of tgt are
// zero without a source -- so one family serves fields with or without Robin walls, with or without a source.  The
// expressions are PDE_ADR_SRC's, only the origin of the six operands differs: a table whose every row is the constant set
// gives PDE_ADR_SRC's (and, with no source, PDE_ADR's) bits.  The engine dispatches here only while fields are present.
constexpr int PDE_ADR_VAR = 7;
// Template number of PINN_PDE_ADR in an ensemble launch (pinn_adr_ens_create; k_fused20d's ENS variants
// only): PDE_ADR's equation, seeds and loss-row layout, with the six coefficients read per MEMBER.  Where
// PDE_ADR passes its coefficients by value travels AdrEnsArg, the address of a device table [members][8] -- a0, a1, nu, r1,
// r2, r3 and two pad doubles, so a row is 64 bytes -- and member m = blockIdx.y reads row m, wave-uniform, once in the
// prologue.  The expressions are PDE_ADR's: a member's rows are the bits of a solo PDE_ADR launch with that member's
// coefficients.  No generic-path kernel is instantiated with it.
constexpr int PDE_ADR_ENS = 8;
constexpr int ADR_ENS_ROW = 8;           // doubles per row of the table
// Template number of PINN_PDE_ADR2 = 10 of the C interface: the adr equation with a time-derivative coefficient b and
// u_xx + kappa u_tt carried as ONE Taylor channel,
//   f = b u_t + (a0 + a1 u) u_x - nu (u_xx + kappa u_tt) + r1 u + r2 u^2 + r3 u^3 - s.
// L = d_xx + kappa d_tt passes a tanh layer as L a = d1 L z + d2 (z_x^2 + kappa z_t^2) and a linear layer as z_xx does, so the
// fourth entry of every stash and output vec4 is w = u_xx + kappa u_tt and kappa is read inside every layer of both sweeps
// (channels_of, preact_adjoint).  The point classes are PDE_ADR_SRC's -- pair-interleaved periodic pairs, data, collocation
// points with s in tgt (zero without a source), a wall block behind the collocation block (its count may be 0) -- with
// THREE-term wall points, r_j = alpha_j u + beta_j u_x + gamma_j u_t - g_j.  Every new term is an fma whose multiplicand
// holds the new coefficient, and b u_t is a product of its own: kappa = 0, b = 1, gamma = 0 adds exact zeros and multiplies by
// one, which gives PDE_ADR_SRC's bits.  Not a member of pde_is_adr: no k_fused20d, tile16 or wide kernel has a variant of it; its
// float64 width-20 kernel is the text of k_fused20d under the name k_adr2_20d, in adr2_20d_unit.hip.
constexpr int PDE_ADR2 = 9;
constexpr bool pde_is_adr(int PDE) {
  return PDE == PDE_ADR || PDE == PDE_ADR_IDE || PDE == PDE_ADR_ROBIN || PDE == PDE_ADR_SRC || PDE == PDE_ADR_VAR ||
         PDE == PDE_ADR_ENS;
}
// the kinds whose six coefficients are run-time constants (PDE_ADR_IDE reads them from the weight vector, PDE_ADR_VAR from
// its table): the predicate keeps this meaning, and PDE_ADR_VAR is not among them
constexpr bool pde_adr_fixed(int PDE) { return PDE == PDE_ADR || PDE == PDE_ADR_ROBIN || PDE == PDE_ADR_SRC; }
// the kinds that share k_fused20d's seed block and loss-row layout of PDE_ADR: the fixed ones and PDE_ADR_VAR, whose block
// differs in where a collocation point's six coefficients come from and in nothing else
// (and PDE_ADR_ENS, whose six come from its member's row of a table)
constexpr bool pde_adr_seed_block(int PDE) { return pde_adr_fixed(PDE) || PDE == PDE_ADR_VAR || PDE == PDE_ADR_ENS || PDE == PDE_ADR2; }
// the kinds that carry a Robin block behind the collocation block
constexpr bool pde_adr_robin(int PDE) { return PDE == PDE_ADR_ROBIN || PDE == PDE_ADR_SRC || PDE == PDE_ADR_VAR || PDE == PDE_ADR2; }
// the kinds that subtract s_i = tgt[point] at a collocation point
constexpr bool pde_adr_src(int PDE) { return PDE == PDE_ADR_SRC || PDE == PDE_ADR_VAR || PDE == PDE_ADR2; }
// trailing equation parameters of the weight vector: 2 lambdas (PDE 1), six coefficients (PDE_ADR_IDE)
constexpr int pde_n_tail(int PDE) { return PDE == 1 ? 2 : PDE == PDE_ADR_IDE ? 6 : 0; }
template <typename real> struct AdrCoef { real a0, a1, nu, r1, r2, r3; };
struct AdrIdeArg { int mask; };
template <typename real> struct AdrRobinArg {
  AdrCoef<real> k;
  const real* ab;      // [n][2]: (alpha_j, beta_j) of Robin point first + j
  int first, n;        // the Robin block: points first .. first + n - 1
  real inv_nw;         // 1 / GLOBAL Robin count
};
// PDE_ADR_SRC: AdrRobinArg's content (n may be 0) and, for k_residual alone, the source by SET index -- the training kernels
// read s from their tgt argument.  src == nullptr: the operator part N[u] (residuals at foreign points, pinn_residual_at)
template <typename real> struct AdrSrcArg : AdrRobinArg<real> {
  const real* src;
};
// PDE_ADR_VAR: AdrSrcArg's content (src is the set's tgt, zero in the collocation block without a source) and the
// coefficient table, kf[6 * i + j] = coefficient j of local collocation point i; 16-byte aligned.  The constants k are not
// read at a collocation point.  kf is touched by collocation points only: the table has n_f rows.
template <typename real> struct AdrVarArg : AdrSrcArg<real> {
  const real* kf;
};
// PDE_ADR_ENS: the members' coefficient table, coef[ADR_ENS_ROW * m + j] = coefficient j of member m; 64-byte rows
struct AdrEnsArg {
  const double* coef;
};
// PDE_ADR2: the eight coefficients, the wall rows ab[4 j ..] = (alpha_j, beta_j, gamma_j, 0) of wall point first + j, the
// block's first point and length, 1 / GLOBAL wall count, and the source by SET index for k_residual (nullptr: N[u] alone)
template <typename real> struct Adr2Arg {
  AdrCoef<real> k;
  real b, kappa;
  const real* ab;
  int first, n;
  real inv_nw;
  const real* src;
};
// row i of the table (every load inside the caller's collocation branch)
template <typename real> __device__ __forceinline__ AdrCoef<real> adr_row(const real* __restrict__ kf, int i) {
  const real* __restrict__ r = kf + (size_t)6 * i;
  return AdrCoef<real>{r[0], r[1], r[2], r[3], r[4], r[5]};
}
// What a kernel of kind PDE takes in the place of the scalar nu: the scalar itself, or the adr value's own argument.  A trait
// with one specialisation per value, not a chain of conditions: a kernel's mangled name then spells PdeCoef<real, PDE>::type
// and nothing about which specialisations exist, so a new value adds its line here and renames no kernel.
template <typename real, int PDE> struct PdeCoef { using type = real; };
template <typename real> struct PdeCoef<real, PDE_ADR> { using type = AdrCoef<real>; };
template <typename real> struct PdeCoef<real, PDE_ADR_IDE> { using type = AdrIdeArg; };
template <typename real> struct PdeCoef<real, PDE_ADR_ROBIN> { using type = AdrRobinArg<real>; };
template <typename real> struct PdeCoef<real, PDE_ADR_SRC> { using type = AdrSrcArg<real>; };
template <typename real> struct PdeCoef<real, PDE_ADR_VAR> { using type = AdrVarArg<real>; };
template <typename real> struct PdeCoef<real, PDE_ADR_ENS> { using type = AdrEnsArg; };
template <typename real> struct PdeCoef<real, PDE_ADR2> { using type = Adr2Arg<real>; };
template <typename real, int PDE> using pde_coef_t = typename PdeCoef<real, PDE>::type;
template <typename real> __device__ __forceinline__ real coef_nu(real nu) { return nu; }
template <typename real> __device__ __forceinline__ real coef_nu(const AdrCoef<real>& k) { return k.nu; }
template <typename real> __device__ __forceinline__ real coef_nu(const AdrIdeArg&) { return real(0); }
template <typename real> __device__ __forceinline__ real coef_nu(const AdrRobinArg<real>& a) { return a.k.nu; }
template <typename real> __device__ __forceinline__ real coef_nu(const Adr2Arg<real>& a) { return a.k.nu; }
template <typename real> __device__ __forceinline__ AdrCoef<real> coef_adr(real) { return AdrCoef<real>{0, 0, 0, 0, 0, 0}; }
template <typename real> __device__ __forceinline__ AdrCoef<real> coef_adr(const AdrCoef<real>& k) { return k; }
// the current coefficients of PDE_ADR_IDE from the tail of the weight vector
template <typename real> __device__ __forceinline__ AdrCoef<real> coef_adr_tail(const real* __restrict__ tail) {
  return AdrCoef<real>{tail[0], tail[1], exp(tail[2]), tail[3], tail[4], tail[5]};
}
// residual of the new kind from the four Taylor channels of a point
template <typename real>
__device__ __forceinline__ real adr_residual(const AdrCoef<real>& k, const vec4<real>& o) {
  const real u = o.x;
  return o.z + (k.a0 + k.a1 * u) * o.y - k.nu * o.w + u * (k.r1 + u * (k.r2 + k.r3 * u));
}

template <typename real> __device__ __forceinline__ real tanh_r(real z);
template <> __device__ __forceinline__ float tanh_r<float>(float z) { return tanhf(z); }
template <> __device__ __forceinline__ double tanh_r<double>(double z) { return tanh(z); }

// ---------------------------------------------------------------------------------------------
// Forward sweep: Taylor channels through every layer for points [base, base+gridDim*64).
//   S[(d*W + k)*n_pad + pt] = (a, zp, zq, zr) of dense layer d, feature k      (d < H)
//   O[o*n_pad + pt]         = (u_o, d/dx, d/dt, d2/dx2) of output o
// ---------------------------------------------------------------------------------------------
// (k_forward_adr2 below is this text with one more term in the fourth channel: a change here belongs there too)
template <typename real, int JT>
__global__ __launch_bounds__(64) void k_forward(NetDesc nd, const real* __restrict__ th,
                                                const real* __restrict__ xs,
                                                const real* __restrict__ ts, int base, int n_pad,
                                                int s_pad, real lbx, real lbt, real sx, real st,
                                                vec4<real>* __restrict__ S,
                                                vec4<real>* __restrict__ O) {
  const int lp = blockIdx.x * 64 + threadIdx.x;   // point index inside the chunk (stash index)
  const int pt = base + lp;                        // index into the point arrays
  const int W = nd.width, H = nd.n_hidden;
  const real x = xs[pt], t = ts[pt];
  const real hx = sx * (x - lbx) - real(1), ht = st * (t - lbt) - real(1);

  {  // dense 0: inputs are (hx, ht); p0 = (sx, 0), q0 = (0, st), r0 = 0
    const real* __restrict__ W0 = th + nd.off_w[0];
    const real* __restrict__ b0 = th + nd.off_b[0];
    for (int j = 0; j < W; ++j) {
      const real w0 = W0[j], w1 = W0[W + j];
      const real z = hx * w0 + ht * w1 + b0[j];
      S[(size_t)j * s_pad + lp] = vec4<real>{tanh_r(z), sx * w0, st * w1, real(0)};
    }
  }
  for (int d = 1; d < H; ++d) {
    const real* __restrict__ Wd = th + nd.off_w[d];
    const real* __restrict__ bd = th + nd.off_b[d];
    const vec4<real>* __restrict__ Sin = S + (size_t)(d - 1) * W * s_pad + lp;
    vec4<real>* __restrict__ Sout = S + (size_t)d * W * s_pad + lp;
    for (int j0 = 0; j0 < W; j0 += JT) {
      real az[JT], ap[JT], aq[JT], ar[JT];
#pragma unroll
      for (int jj = 0; jj < JT; ++jj) {
        az[jj] = (j0 + jj < W) ? bd[j0 + jj] : real(0);
        ap[jj] = aq[jj] = ar[jj] = real(0);
      }
      for (int k = 0; k < W; ++k) {
        const vec4<real> s = Sin[(size_t)k * s_pad];
        const real a = s.x, d1 = real(1) - a * a, d2 = real(-2) * a * d1;
        const real p = d1 * s.y, q = d1 * s.z, r = d2 * s.y * s.y + d1 * s.w;
#pragma unroll
        for (int jj = 0; jj < JT; ++jj) {
          if (j0 + jj < W) {
            const real w = Wd[k * W + j0 + jj];
            az[jj] += a * w; ap[jj] += p * w; aq[jj] += q * w; ar[jj] += r * w;
          }
        }
      }
#pragma unroll
      for (int jj = 0; jj < JT; ++jj)
        if (j0 + jj < W)
          Sout[(size_t)(j0 + jj) * s_pad] = vec4<real>{tanh_r(az[jj]), ap[jj], aq[jj], ar[jj]};
    }
  }
  {  // linear output layer (dense H)
    const real* __restrict__ WL = th + nd.off_w[H];
    const real* __restrict__ bL = th + nd.off_b[H];
    const vec4<real>* __restrict__ Sin = S + (size_t)(H - 1) * W * s_pad + lp;
    real oz[2] = {bL[0], nd.n_out > 1 ? bL[1] : real(0)};
    real op[2] = {0, 0}, oq[2] = {0, 0}, orr[2] = {0, 0};
    for (int k = 0; k < W; ++k) {
      const vec4<real> s = Sin[(size_t)k * s_pad];
      const real a = s.x, d1 = real(1) - a * a, d2 = real(-2) * a * d1;
      const real p = d1 * s.y, q = d1 * s.z, r = d2 * s.y * s.y + d1 * s.w;
#pragma unroll
      for (int o = 0; o < 2; ++o) {
        if (o < nd.n_out) {
          const real w = WL[k * nd.n_out + o];
          oz[o] += a * w; op[o] += p * w; oq[o] += q * w; orr[o] += r * w;
        }
      }
    }
    for (int o = 0; o < nd.n_out; ++o)
      O[(size_t)o * n_pad + pt] = vec4<real>{oz[o], op[o], oq[o], orr[o]};
  }
}

// PDE_ADR2's forward sweep, O[pt] = (u, u_x, u_t, u_xx + kap u_tt): k_forward with the kappa term of every layer's fourth
// channel added by an fma on top of k_forward's own expression (kap = 0: an exact zero, k_forward's bits).  A kernel text of
// its own and not a shared body: k_forward through a shared inline function compiles to other instructions than it had.
template <typename real, int JT>
__global__ __launch_bounds__(64) void k_forward_adr2(NetDesc nd, const real* __restrict__ th,
                                                const real* __restrict__ xs,
                                                const real* __restrict__ ts, int base, int n_pad,
                                                int s_pad, real lbx, real lbt, real sx, real st,
                                                vec4<real>* __restrict__ S,
                                                vec4<real>* __restrict__ O, real kap) {
  const int lp = blockIdx.x * 64 + threadIdx.x;   // point index inside the chunk (stash index)
  const int pt = base + lp;                        // index into the point arrays
  const int W = nd.width, H = nd.n_hidden;
  const real x = xs[pt], t = ts[pt];
  const real hx = sx * (x - lbx) - real(1), ht = st * (t - lbt) - real(1);

  {  // dense 0: inputs are (hx, ht); p0 = (sx, 0), q0 = (0, st), r0 = 0
    const real* __restrict__ W0 = th + nd.off_w[0];
    const real* __restrict__ b0 = th + nd.off_b[0];
    for (int j = 0; j < W; ++j) {
      const real w0 = W0[j], w1 = W0[W + j];
      const real z = hx * w0 + ht * w1 + b0[j];
      S[(size_t)j * s_pad + lp] = vec4<real>{tanh_r(z), sx * w0, st * w1, real(0)};
    }
  }
  for (int d = 1; d < H; ++d) {
    const real* __restrict__ Wd = th + nd.off_w[d];
    const real* __restrict__ bd = th + nd.off_b[d];
    const vec4<real>* __restrict__ Sin = S + (size_t)(d - 1) * W * s_pad + lp;
    vec4<real>* __restrict__ Sout = S + (size_t)d * W * s_pad + lp;
    for (int j0 = 0; j0 < W; j0 += JT) {
      real az[JT], ap[JT], aq[JT], ar[JT];
#pragma unroll
      for (int jj = 0; jj < JT; ++jj) {
        az[jj] = (j0 + jj < W) ? bd[j0 + jj] : real(0);
        ap[jj] = aq[jj] = ar[jj] = real(0);
      }
      for (int k = 0; k < W; ++k) {
        const vec4<real> s = Sin[(size_t)k * s_pad];
        const real a = s.x, d1 = real(1) - a * a, d2 = real(-2) * a * d1;
        const real p = d1 * s.y, q = d1 * s.z, r = fma(kap * d2 * s.z, s.z, d2 * s.y * s.y + d1 * s.w);
#pragma unroll
        for (int jj = 0; jj < JT; ++jj) {
          if (j0 + jj < W) {
            const real w = Wd[k * W + j0 + jj];
            az[jj] += a * w; ap[jj] += p * w; aq[jj] += q * w; ar[jj] += r * w;
          }
        }
      }
#pragma unroll
      for (int jj = 0; jj < JT; ++jj)
        if (j0 + jj < W)
          Sout[(size_t)(j0 + jj) * s_pad] = vec4<real>{tanh_r(az[jj]), ap[jj], aq[jj], ar[jj]};
    }
  }
  {  // linear output layer (dense H)
    const real* __restrict__ WL = th + nd.off_w[H];
    const real* __restrict__ bL = th + nd.off_b[H];
    const vec4<real>* __restrict__ Sin = S + (size_t)(H - 1) * W * s_pad + lp;
    real oz[2] = {bL[0], nd.n_out > 1 ? bL[1] : real(0)};
    real op[2] = {0, 0}, oq[2] = {0, 0}, orr[2] = {0, 0};
    for (int k = 0; k < W; ++k) {
      const vec4<real> s = Sin[(size_t)k * s_pad];
      const real a = s.x, d1 = real(1) - a * a, d2 = real(-2) * a * d1;
      const real p = d1 * s.y, q = d1 * s.z, r = fma(kap * d2 * s.z, s.z, d2 * s.y * s.y + d1 * s.w);
#pragma unroll
      for (int o = 0; o < 2; ++o) {
        if (o < nd.n_out) {
          const real w = WL[k * nd.n_out + o];
          oz[o] += a * w; op[o] += p * w; oq[o] += q * w; orr[o] += r * w;
        }
      }
    }
    for (int o = 0; o < nd.n_out; ++o)
      O[(size_t)o * n_pad + pt] = vec4<real>{oz[o], op[o], oq[o], orr[o]};
  }
}

// Point class of global point index g.
enum { CLS_BLO = 0, CLS_BHI = 1, CLS_DATA = 2, CLS_COL = 3, CLS_PAD = 4 };
__device__ __forceinline__ int point_class(const SetDesc& sd, int g) {
  if (g < sd.n_b) return CLS_BLO;
  if (g < 2 * sd.n_b) return CLS_BHI;
  if (g < 2 * sd.n_b + sd.n_u) return CLS_DATA;
  if (g < sd.n_all) return CLS_COL;
  return CLS_PAD;
}

// the same for the pair-interleaved boundary block of PDE_ADR: lo points at even, hi points at odd indices below 2 n_b
__device__ __forceinline__ int point_class_adr(const SetDesc& sd, int g) {
  if (g < 2 * sd.n_b) return (g & 1) ? CLS_BHI : CLS_BLO;
  if (g < 2 * sd.n_b + sd.n_u) return CLS_DATA;
  if (g < sd.n_all) return CLS_COL;
  return CLS_PAD;
}

// Per-point loss contributions and output adjoints.
//   sb[o] <- (h_bar, p_bar, q_bar, r_bar) of output o;  lt[0..2] <- (f, data, boundary) loss parts
//   dl[0..1] <- d/d lambda_1, d/d lambda_2 contributions (identification only); PDE_ADR_IDE: dl[0..5] <- d/d (a0, a1,
//   log nu, r1, r2, r3), the caller's array holds six
// point_seeds_own: the same with the point's OWN outputs handed in (ou, and ov for two-output nets) instead of read from
// O -- a fused kernel has them on chip; O is read only for the partner of a periodic-boundary pair
template <typename real, int PDE>
__device__ __forceinline__ void point_seeds_own(const SetDesc& sd, int g, int n_pad, const vec4<real>& ou,
                                                const vec4<real>& ov, const vec4<real>* __restrict__ O,
                                                const real* __restrict__ tgt, real c1, real c2,
                                                vec4<real> sb[2], real lt[3], real dl[2],
                                                const AdrCoef<real>& k = AdrCoef<real>{0, 0, 0, 0, 0, 0},
                                                const AdrRobinArg<real>* rb = nullptr, const real* __restrict__ kf = nullptr);
template <typename real, int PDE>
__device__ __forceinline__ void point_seeds(const SetDesc& sd, int g, int n_pad,
                                            const vec4<real>* __restrict__ O,
                                            const real* __restrict__ tgt, real c1, real c2,
                                            vec4<real> sb[2], real lt[3], real dl[2],
                                            const AdrCoef<real>& k = AdrCoef<real>{0, 0, 0, 0, 0, 0},
                                            const AdrRobinArg<real>* rb = nullptr, const real* __restrict__ kf = nullptr) {
  const vec4<real> ou = O[g], ov = PDE == 2 ? O[(size_t)n_pad + g] : vec4<real>{0, 0, 0, 0};
  point_seeds_own<real, PDE>(sd, g, n_pad, ou, ov, O, tgt, c1, c2, sb, lt, dl, k, rb, kf);
}
template <typename real, int PDE>
__device__ __forceinline__ void point_seeds_own(const SetDesc& sd, int g, int n_pad, const vec4<real>& ou,
                                                const vec4<real>& ov, const vec4<real>* __restrict__ O,
                                                const real* __restrict__ tgt, real c1, real c2,
                                                vec4<real> sb[2], real lt[3], real dl[2], const AdrCoef<real>& k_arg,
                                                const AdrRobinArg<real>* rb, const real* __restrict__ kf) {
  const int cls = pde_is_adr(PDE) ? point_class_adr(sd, g) : point_class(sd, g);
  sb[0] = sb[1] = vec4<real>{0, 0, 0, 0};
  lt[0] = lt[1] = lt[2] = real(0);
  dl[0] = dl[1] = real(0);
  if constexpr (PDE == PDE_ADR_IDE) dl[2] = dl[3] = dl[4] = dl[5] = real(0);
  if constexpr (pde_adr_robin(PDE)) {     // the Robin block stands behind the collocation block (CLS_PAD by sd's counts)
    const int j = g - rb->first;
    if ((unsigned)j < (unsigned)rb->n) {  // r = alpha u + beta u_x - g; its square counts in the boundary part
      const real al = rb->ab[2 * j], be = rb->ab[2 * j + 1];
      const real r = al * ou.x + be * ou.y - tgt[g];
      lt[2] = r * r * rb->inv_nw;
      sb[0].x = real(2) * r * al * rb->inv_nw; sb[0].y = real(2) * r * be * rb->inv_nw;
      return;
    }
  }
  if (cls == CLS_PAD) return;
  const real inv_nf = (real)sd.inv_nf, inv_nu = (real)sd.inv_nu, inv_nb = (real)sd.inv_nb;
  if constexpr (pde_is_adr(PDE)) {   // advection-diffusion-reaction, run-time coefficients, periodic pairs (g, g ^ 1)
    const vec4<real> o = ou;
    if (cls == CLS_COL) {
      // PDE_ADR_VAR: the point's own row of the table (kf), read here and nowhere else -- the table ends with the block
      const AdrCoef<real> k = PDE == PDE_ADR_VAR ? adr_row<real>(kf, g - 2 * sd.n_b - sd.n_u) : k_arg;
      const real u = o.x, adv = k.a0 + k.a1 * u;
      real f = adr_residual(k, o);
      if constexpr (pde_adr_src(PDE)) {        // minus the source, an operation of its own (s = 0: PDE_ADR's bits)
#pragma clang fp contract(off)
        f = f - tgt[g];
      }
      const real fb = real(2) * f * inv_nf;
      lt[0] = f * f * inv_nf;
      sb[0].x = fb * (k.a1 * o.y + k.r1 + u * (real(2) * k.r2 + real(3) * k.r3 * u));
      sb[0].y = fb * adv; sb[0].z = fb; sb[0].w = -k.nu * fb;
      if constexpr (PDE == PDE_ADR_IDE) {      // f is linear in a0, a1, r1, r2, r3; d nu / d log nu = nu
        dl[0] = fb * o.y; dl[1] = fb * u * o.y; dl[2] = -fb * k.nu * o.w;
        dl[3] = fb * u; dl[4] = fb * u * u; dl[5] = fb * u * u * u;
      }
    } else if (cls == CLS_DATA) {
      const real dd = o.x - tgt[g];
      lt[1] = dd * dd * inv_nu;
      sb[0].x = real(2) * dd * inv_nu;
    } else {                        // own minus partner: +2 (lo - hi) / n_b at lo, -2 (lo - hi) / n_b at hi
      const vec4<real> pr = O[g ^ 1];
      const real du = o.x - pr.x, dp = o.y - pr.y;
      if (cls == CLS_BLO) lt[2] = (du * du + dp * dp) * inv_nb;
      sb[0].x = real(2) * du * inv_nb; sb[0].y = real(2) * dp * inv_nb;
    }
  } else if (PDE == 0 || PDE == 1) {   // Burgers (inference / identification)
    const vec4<real> o = ou;
    const bool res = (PDE == 0) ? (cls == CLS_COL) : (cls == CLS_DATA);
    if (res) {
      const real f = o.z + c1 * o.x * o.y - c2 * o.w;       // u_t + c1 u u_x - c2 u_xx
      const real fb = real(2) * f * ((PDE == 0) ? inv_nf : inv_nu);
      lt[0] = f * f * ((PDE == 0) ? inv_nf : inv_nu);
      sb[0].x = fb * c1 * o.y; sb[0].y = fb * c1 * o.x; sb[0].z = fb; sb[0].w = -c2 * fb;
      if (PDE == 1) { dl[0] = fb * o.x * o.y; dl[1] = -fb * c2 * o.w; }
    }
    if (cls == CLS_DATA) {
      const real dd = o.x - tgt[g];
      lt[1] = dd * dd * inv_nu;
      sb[0].x += real(2) * dd * inv_nu;
    }
  } else {                      // Schrodinger
    if (cls == CLS_COL) {
      const real u = ou.x, v = ov.x, h2 = u * u + v * v;
      const real fu = ou.z + real(0.5) * ov.w + h2 * v;     // u_t + v_xx/2 + |h|^2 v
      const real fv = ov.z - real(0.5) * ou.w - h2 * u;     // v_t - u_xx/2 - |h|^2 u
      lt[0] = (fu * fu + fv * fv) * inv_nf;
      const real gu = real(2) * fu * inv_nf, gv = real(2) * fv * inv_nf;
      sb[0].x = gu * real(2) * u * v - gv * (real(3) * u * u + v * v);
      sb[1].x = gu * (u * u + real(3) * v * v) - gv * real(2) * u * v;
      sb[0].z = gu; sb[1].z = gv;
      sb[0].w = real(-0.5) * gv; sb[1].w = real(0.5) * gu;
    } else if (cls == CLS_DATA) {
      const real du = ou.x - tgt[g], dv = ov.x - tgt[(size_t)n_pad + g];
      lt[1] = (du * du + dv * dv) * inv_nu;
      sb[0].x = real(2) * du * inv_nu; sb[1].x = real(2) * dv * inv_nu;
    } else {                    // periodic boundary pair (g in lo  <->  g + n_b in hi)
      const int lo = (cls == CLS_BLO) ? g : g - sd.n_b, hi = lo + sd.n_b;
      const bool is_lo = cls == CLS_BLO;
      const vec4<real> ul = is_lo ? ou : O[lo], uh = is_lo ? O[hi] : ou;
      const vec4<real> vl = is_lo ? ov : O[(size_t)n_pad + lo], vh = is_lo ? O[(size_t)n_pad + hi] : ov;
      const real dhu = ul.x - uh.x, dhv = vl.x - vh.x, dpu = ul.y - uh.y, dpv = vl.y - vh.y;
      const real sg = (cls == CLS_BLO) ? real(2) * inv_nb : real(-2) * inv_nb;
      if (cls == CLS_BLO) lt[2] = (dhu * dhu + dhv * dhv + dpu * dpu + dpv * dpv) * inv_nb;
      sb[0].x = sg * dhu; sb[1].x = sg * dhv; sb[0].y = sg * dpu; sb[1].y = sg * dpv;
    }
  }
}

// PDE_ADR2: loss parts and output adjoints of point g from its own outputs o = (u, u_x, u_t, w), w = u_xx + kappa u_tt; O
// is read for the partner of a periodic pair only.  PDE_ADR_SRC's expressions with b u_t in the place of u_t (a product of its
// own, never contracted: b = 1 gives u_t) and gamma u_t added to a wall residual by an fma (gamma = 0 adds an exact zero)
template <typename real>
__device__ __forceinline__ void adr2_point_seeds(const SetDesc& sd, int g, const vec4<real>* __restrict__ O,
                                                 const real* __restrict__ tgt, const Adr2Arg<real>& a, vec4<real>& sb,
                                                 real lt[3]) {
  const vec4<real> o = O[g];
  sb = vec4<real>{0, 0, 0, 0};
  lt[0] = lt[1] = lt[2] = real(0);
  const int j = g - a.first;
  if ((unsigned)j < (unsigned)a.n) {        // the wall block stands behind the collocation block
    const vec4<real> w = *reinterpret_cast<const vec4<real>*>(a.ab + 4 * (size_t)j);
    const real r = fma(w.z, o.z, w.x * o.x + w.y * o.y) - tgt[g];
    lt[2] = r * r * a.inv_nw;
    sb.x = real(2) * r * w.x * a.inv_nw; sb.y = real(2) * r * w.y * a.inv_nw; sb.z = real(2) * r * w.z * a.inv_nw;
    return;
  }
  const int cls = point_class_adr(sd, g);
  if (cls == CLS_PAD) return;
  const real inv_nf = (real)sd.inv_nf, inv_nu = (real)sd.inv_nu, inv_nb = (real)sd.inv_nb;
  if (cls == CLS_COL) {
    const AdrCoef<real>& k = a.k;
    const real u = o.x, adv = k.a0 + k.a1 * u;
    real bz, f;
    {
#pragma clang fp contract(off)
      bz = a.b * o.z;
    }
    f = adr_residual(k, vec4<real>{o.x, o.y, bz, o.w});
    {
#pragma clang fp contract(off)
      f = f - tgt[g];
    }
    const real fb = real(2) * f * inv_nf;
    lt[0] = f * f * inv_nf;
    sb.x = fb * (k.a1 * o.y + k.r1 + u * (real(2) * k.r2 + real(3) * k.r3 * u));
    sb.y = fb * adv; sb.z = fb * a.b; sb.w = -k.nu * fb;
  } else if (cls == CLS_DATA) {
    const real dd = o.x - tgt[g];
    lt[1] = dd * dd * inv_nu;
    sb.x = real(2) * dd * inv_nu;
  } else {                          // own minus partner, as PDE_ADR
    const vec4<real> pr = O[g ^ 1];
    const real du = o.x - pr.x, dp = o.y - pr.y;
    if (cls == CLS_BLO) lt[2] = (du * du + dp * dp) * inv_nb;
    sb.x = real(2) * du * inv_nb; sb.y = real(2) * dp * inv_nb;
  }
}

template <typename real>
__device__ __forceinline__ real dot4(const vec4<real>& a, const vec4<real>& b) {
  return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
}

// layer-input channels (h,p,q,r) and tanh derivative factors from a stash entry
template <typename real>
__device__ __forceinline__ vec4<real> channels_of(const vec4<real>& s, real& d1, real& d2) {
  const real a = s.x;
  d1 = real(1) - a * a;
  d2 = real(-2) * a * d1;
  return vec4<real>{a, d1 * s.y, d1 * s.z, d2 * s.y * s.y + d1 * s.w};
}

// adjoint of the pre-activation channels from the adjoint of the output channels (A.3)
template <typename real>
__device__ __forceinline__ vec4<real> preact_adjoint(const vec4<real>& s, const vec4<real>& ob) {
  const real a = s.x, d1 = real(1) - a * a, d2 = real(-2) * a * d1;
  const real d3 = real(-2) * d1 * (real(1) - real(3) * a * a);
  vec4<real> zb;
  zb.x = d1 * ob.x + d2 * (s.y * ob.y + s.z * ob.z + s.w * ob.w) + d3 * s.y * s.y * ob.w;
  zb.y = d1 * ob.y + real(2) * d2 * s.y * ob.w;
  zb.z = d1 * ob.z;
  zb.w = d1 * ob.w;
  return zb;
}

// The two functions above as a trait of PDE: every existing kind gets them as they are; PDE_ADR2 adds its kappa terms by an
// fma on top of each (kappa = 0: an exact zero)
template <int PDE, typename real>
__device__ __forceinline__ vec4<real> channels_pde(const vec4<real>& s, real& d1, real& d2, real kap) {
  vec4<real> in = channels_of(s, d1, d2);
  if constexpr (PDE == PDE_ADR2) in.w = fma(kap * d2 * s.z, s.z, in.w);
  return in;
}
template <int PDE, typename real>
__device__ __forceinline__ vec4<real> preact_adjoint_pde(const vec4<real>& s, const vec4<real>& ob, real kap) {
  vec4<real> zb = preact_adjoint(s, ob);
  if constexpr (PDE == PDE_ADR2) {
    const real a = s.x, d1 = real(1) - a * a, d2 = real(-2) * a * d1;
    const real d3 = real(-2) * d1 * (real(1) - real(3) * a * a);
    zb.x = fma(kap * d3 * s.z * s.z, ob.w, zb.x);
    zb.z = fma(real(2) * d2 * kap * s.z, ob.w, zb.z);
  }
  return zb;
}
template <typename real, typename Coef> __device__ __forceinline__ real coef_kappa(const Coef&) { return real(0); }
template <typename real> __device__ __forceinline__ real coef_kappa(const Adr2Arg<real>& a) { return a.kappa; }

// ---------------------------------------------------------------------------------------------
// Reverse sweep for one wave of 64 points.  Emits one partial-gradient row per wave:
//   part[row*R + i], i < n_theta : sum over the wave's points of dL/dtheta_i
//   part[row*R + n_theta + {0,1,2}] : loss parts (residual, data, boundary)
// Rows are summed in fixed order by k_reduce_rows -> deterministic gradients.
// ---------------------------------------------------------------------------------------------
template <typename real, int PDE, int KT>
__global__ __launch_bounds__(64) void k_backward(NetDesc nd, SetDesc sd,
                                                 const real* __restrict__ th,
                                                 const real* __restrict__ xs,
                                                 const real* __restrict__ ts,
                                                 const real* __restrict__ tgt, int base, int n_pad,
                                                 int s_pad, real lbx, real lbt, real sx, real st,
                                                 pde_coef_t<real, PDE> nu, const vec4<real>* __restrict__ S,
                                                 const vec4<real>* __restrict__ O,
                                                 vec4<real>* __restrict__ ZA,
                                                 vec4<real>* __restrict__ ZB,
                                                 real* __restrict__ part, int R, int accumulate) {
  const int lane = threadIdx.x;
  const int lp = blockIdx.x * 64 + lane;
  const int pt = base + lp;
  const int W = nd.width, H = nd.n_hidden, NO = nd.n_out;
  real* __restrict__ row = part + (size_t)blockIdx.x * R;

  real c1 = real(1), c2 = coef_nu<real>(nu);
  if (PDE == 1) { c1 = th[nd.n_net]; c2 = exp(th[nd.n_net + 1]); }

  const real kap = coef_kappa<real>(nu);
  vec4<real> sb[2];
  real lt[3], dl[PDE == PDE_ADR_IDE ? 6 : 2];
  if constexpr (PDE == PDE_ADR2) { sb[1] = vec4<real>{0, 0, 0, 0}; adr2_point_seeds<real>(sd, pt, O, tgt, nu, sb[0], lt); }
  else if constexpr (PDE == PDE_ADR) point_seeds<real, PDE>(sd, pt, n_pad, O, tgt, c1, c2, sb, lt, dl, coef_adr<real>(nu));
  else if constexpr (PDE == PDE_ADR_VAR) point_seeds<real, PDE>(sd, pt, n_pad, O, tgt, c1, c2, sb, lt, dl, nu.k, &nu, nu.kf);
  else if constexpr (pde_adr_robin(PDE)) point_seeds<real, PDE>(sd, pt, n_pad, O, tgt, c1, c2, sb, lt, dl, nu.k, &nu);
  else if constexpr (PDE == PDE_ADR_IDE) point_seeds<real, PDE>(sd, pt, n_pad, O, tgt, c1, c2, sb, lt, dl, coef_adr_tail<real>(th + nd.n_net));
  else point_seeds<real, PDE>(sd, pt, n_pad, O, tgt, c1, c2, sb, lt, dl);

  auto put = [&](int idx, real v) {   // lane-uniform idx; executed by one lane
    row[idx] = accumulate ? row[idx] + v : v;
  };
  {
    const real l0 = wave_sum(lt[0]), l1 = wave_sum(lt[1]), l2 = wave_sum(lt[2]);
    if (lane == 0) { put(nd.n_theta + 0, l0); put(nd.n_theta + 1, l1); put(nd.n_theta + 2, l2); }
    if (PDE == 1) {
      const real g1 = wave_sum(dl[0]), g2 = wave_sum(dl[1]);
      if (lane == 0) { put(nd.n_net, g1); put(nd.n_net + 1, g2); }
    }
    if constexpr (PDE == PDE_ADR_IDE) {      // the six tail entries; a frozen coefficient's is exactly 0.0
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        const real gk = wave_sum(dl[k]);
        if (lane == 0) put(nd.n_net + k, ((nu.mask >> k) & 1) ? gk : real(0));
      }
    }
  }

  vec4<real>* __restrict__ Zcur = ZA;
  vec4<real>* __restrict__ Znxt = ZB;

  {  // dense H (linear output): z_bar = seeds
    const real* __restrict__ WL = th + nd.off_w[H];
    const vec4<real>* __restrict__ Sin = S + (size_t)(H - 1) * W * s_pad + lp;
    real keep[4] = {0, 0, 0, 0};      // lane l keeps entries l, l+64, l+128, l+192 of W*NO (<= 256)
    for (int k = 0; k < W; ++k) {
      const vec4<real> s = Sin[(size_t)k * s_pad];
      real d1, d2;
      const vec4<real> in = channels_pde<PDE>(s, d1, d2, kap);
      vec4<real> ob{0, 0, 0, 0};
#pragma unroll
      for (int o = 0; o < 2; ++o) {
        if (o < NO) {
          const real g = wave_sum(dot4(in, sb[o]));
          const int e = k * NO + o;
#pragma unroll
          for (int q = 0; q < 4; ++q) if ((e >> 6) == q && (e & 63) == lane) keep[q] = g;
          const real w = WL[k * NO + o];
          ob.x += sb[o].x * w; ob.y += sb[o].y * w; ob.z += sb[o].z * w; ob.w += sb[o].w * w;
        }
      }
      Zcur[(size_t)k * s_pad + lp] = preact_adjoint_pde<PDE>(s, ob, kap);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) if (q * 64 + lane < W * NO) put(nd.off_w[H] + q * 64 + lane, keep[q]);
    for (int o = 0; o < NO; ++o) {
      const real g = wave_sum(sb[o].x);
      if (lane == 0) put(nd.off_b[H] + o, g);
    }
  }

  for (int d = H - 1; d >= 1; --d) {
    const real* __restrict__ Wd = th + nd.off_w[d];
    const vec4<real>* __restrict__ Sin = S + (size_t)(d - 1) * W * s_pad + lp;
    for (int k0 = 0; k0 < W; k0 += KT) {
      vec4<real> sk[KT], in[KT], acc[KT];
      real keep0[KT], keep1[KT], keepb0 = 0, keepb1 = 0;
#pragma unroll
      for (int kk = 0; kk < KT; ++kk) {
        const int k = (k0 + kk < W) ? k0 + kk : W - 1;
        sk[kk] = Sin[(size_t)k * s_pad];
        real d1, d2;
        in[kk] = channels_pde<PDE>(sk[kk], d1, d2, kap);
        acc[kk] = vec4<real>{0, 0, 0, 0};
        keep0[kk] = keep1[kk] = real(0);
      }
      for (int j = 0; j < W; ++j) {
        const vec4<real> zb = Zcur[(size_t)j * s_pad + lp];
        const bool mine = ((j & 63) == lane);
        if (k0 == 0) {
          const real g = wave_sum(zb.x);
          if (mine) { if (j < 64) keepb0 = g; else keepb1 = g; }
        }
#pragma unroll
        for (int kk = 0; kk < KT; ++kk) {
          if (k0 + kk < W) {
            const real g = wave_sum(dot4(in[kk], zb));
            if (mine) { if (j < 64) keep0[kk] = g; else keep1[kk] = g; }
            const real w = Wd[(k0 + kk) * W + j];
            acc[kk].x += zb.x * w; acc[kk].y += zb.y * w; acc[kk].z += zb.z * w; acc[kk].w += zb.w * w;
          }
        }
      }
#pragma unroll
      for (int kk = 0; kk < KT; ++kk) {
        if (k0 + kk < W) {
          const int o = nd.off_w[d] + (k0 + kk) * W;
          if (lane < W) put(o + lane, keep0[kk]);
          if (lane + 64 < W) put(o + lane + 64, keep1[kk]);
          Znxt[(size_t)(k0 + kk) * s_pad + lp] = preact_adjoint_pde<PDE>(sk[kk], acc[kk], kap);
        }
      }
      if (k0 == 0) {
        if (lane < W) put(nd.off_b[d] + lane, keepb0);
        if (lane + 64 < W) put(nd.off_b[d] + lane + 64, keepb1);
      }
    }
    vec4<real>* tmp = Zcur; Zcur = Znxt; Znxt = tmp;
  }

  {  // dense 0: inputs (hx, ht), p0 = (sx, 0), q0 = (0, st), r0 = 0
    const real x = xs[pt], t = ts[pt];
    const real hx = sx * (x - lbx) - real(1), ht = st * (t - lbt) - real(1);
    real kx0 = 0, kx1 = 0, kt0 = 0, kt1 = 0, kb0 = 0, kb1 = 0;
    for (int j = 0; j < W; ++j) {
      const vec4<real> zb = Zcur[(size_t)j * s_pad + lp];
      const real gx = wave_sum(hx * zb.x + sx * zb.y);
      const real gt = wave_sum(ht * zb.x + st * zb.z);
      const real gb = wave_sum(zb.x);
      if ((j & 63) == lane) {
        if (j < 64) { kx0 = gx; kt0 = gt; kb0 = gb; } else { kx1 = gx; kt1 = gt; kb1 = gb; }
      }
    }
    if (lane < W) { put(nd.off_w[0] + lane, kx0); put(nd.off_w[0] + W + lane, kt0); put(nd.off_b[0] + lane, kb0); }
    if (lane + 64 < W) { put(nd.off_w[0] + lane + 64, kx1); put(nd.off_w[0] + W + lane + 64, kt1); put(nd.off_b[0] + lane + 64, kb1); }
  }
}

// PDE residual at stored points from the forward outputs (f_model()).
template <typename real, int PDE>
__global__ void k_residual(int first, int n, int n_pad, const vec4<real>* __restrict__ O,
                           const real* __restrict__ th, int n_net, pde_coef_t<real, PDE> nu,
                           double* __restrict__ f, int n_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int g = first + i;
  if constexpr (PDE == PDE_ADR) {
    f[i] = (double)adr_residual(nu, O[g]);
  } else if constexpr (PDE == PDE_ADR_SRC) {
    real r = adr_residual(nu.k, O[g]);
    if (nu.src) {
#pragma clang fp contract(off)
      r = r - nu.src[g];
    }
    f[i] = (double)r;
  } else if constexpr (PDE == PDE_ADR_VAR) {   // over the set only (first = the collocation block's first point): row i, s by set index
    real r = adr_residual(adr_row<real>(nu.kf, i), O[g]);
    {
#pragma clang fp contract(off)
      r = r - nu.src[g];
    }
    f[i] = (double)r;
  } else if constexpr (PDE == PDE_ADR2) {      // O's fourth entry is u_xx + kappa u_tt (k_forward_adr2)
    const vec4<real> o = O[g];
    real bz, r;
    {
#pragma clang fp contract(off)
      bz = nu.b * o.z;
    }
    r = adr_residual(nu.k, vec4<real>{o.x, o.y, bz, o.w});
    if (nu.src) {
#pragma clang fp contract(off)
      r = r - nu.src[g];
    }
    f[i] = (double)r;
  } else if constexpr (PDE == PDE_ADR_IDE) {
    f[i] = (double)adr_residual(coef_adr_tail<real>(th + n_net), O[g]);
  } else if (PDE == 2) {
    const vec4<real> ou = O[g], ov = O[(size_t)n_pad + g];
    const real u = ou.x, v = ov.x, h2 = u * u + v * v;
    f[(size_t)i * 2 + 0] = (double)(ou.z + real(0.5) * ov.w + h2 * v);
    f[(size_t)i * 2 + 1] = (double)(ov.z - real(0.5) * ou.w - h2 * u);
  } else {
    real c1 = real(1), c2 = coef_nu<real>(nu);
    if (PDE == 1) { c1 = th[n_net]; c2 = exp(th[n_net + 1]); }
    const vec4<real> o = O[g];
    f[i] = (double)(o.z + c1 * o.x * o.y - c2 * o.w);
  }
}

// Robin residuals r_j = alpha_j u + beta_j u_x - g_j at the stored Robin points from the forward outputs
// (pinn_robin_residual): forward only, no seeds
template <typename real>
__global__ void k_robin_residual(AdrRobinArg<real> rb, const vec4<real>* __restrict__ O, const real* __restrict__ tgt,
                                 double* __restrict__ out) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= rb.n) return;
  const vec4<real> o = O[rb.first + j];
  out[j] = (double)(rb.ab[2 * j] * o.x + rb.ab[2 * j + 1] * o.y - tgt[rb.first + j]);
}

// the three-term wall residuals of PDE_ADR2, r_j = alpha_j u + beta_j u_x + gamma_j u_t - g_j
template <typename real>
__global__ void k_robin3_residual(Adr2Arg<real> rb, const vec4<real>* __restrict__ O, const real* __restrict__ tgt,
                                 double* __restrict__ out) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= rb.n) return;
  const vec4<real> o = O[rb.first + j];
  const vec4<real> w = *reinterpret_cast<const vec4<real>*>(rb.ab + 4 * (size_t)j);
  out[j] = (double)(fma(w.z, o.z, w.x * o.x + w.y * o.y) - tgt[rb.first + j]);
}

}  // namespace pinn
