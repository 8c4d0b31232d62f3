// pointsets.h -- the training set on the host, stated once: its geometry (SetDesc, which the kernels take too), the sets as
// handed over (PointSets), the assembly of one set into the layout every kernel reads, and the affine map of the inputs.
// Plain C++: no HIP include and no kernel code, so a host compiler alone builds it (tests/host/pointsets_check.cpp).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace pinn {

// Training-set geometry for one evaluation.  Points are stored in class order
// [boundary-lo | boundary-hi | data | collocation | pad].  (PDE_ADR_ROBIN: a Robin block stands between the collocation block
// and the padding; it is not counted here -- n_all ends the collocation block, n_pad covers the Robin block -- see AdrRobinArg.)
struct SetDesc {
  int n_b, n_u, n_f;         // local counts
  int n_all;                 // 2*n_b + n_u + n_f
  int n_pad;                 // rounded up to a multiple of 64
  double inv_nb, inv_nu, inv_nf;   // 1 / GLOBAL set sizes (mean() denominators)
};

// first point of the data block, of the collocation block and of the adr kind's Robin block (host only)
inline int data_first(const SetDesc& sd) { return 2 * sd.n_b; }
inline int colloc_first(const SetDesc& sd) { return 2 * sd.n_b + sd.n_u; }
inline int robin_first(const SetDesc& sd) { return sd.n_all; }

// The geometry of local counts under global totals (a total of 0: that class's mean is 0, not a division).  The Robin count
// enters n_pad only.
inline SetDesc make_set_desc(int n_b, int n_u, int n_f, int64_t nb_total, int64_t nu_total, int64_t nf_total, int n_robin) {
  SetDesc sd{};
  sd.n_b = n_b; sd.n_u = n_u; sd.n_f = n_f;
  sd.n_all = 2 * n_b + n_u + n_f;
  sd.n_pad = (sd.n_all + n_robin + 63) / 64 * 64;
  sd.inv_nb = nb_total > 0 ? 1.0 / (double)nb_total : 0.0;
  sd.inv_nu = nu_total > 0 ? 1.0 / (double)nu_total : 0.0;
  sd.inv_nf = nf_total > 0 ? 1.0 / (double)nf_total : 0.0;
  return sd;
}

// the point sets as handed over (float64): collocation [n_f][2], data [n_u][2] with targets [n_u][n_out], pairs [n_b][2] each
struct PointSets {
  std::vector<double> Xf, Xu, U, Xlo, Xhi;
};
using PointField = std::vector<double> PointSets::*;

// one field of every entry <- the same n doubles / entry k <- row k of a [K][n] array
inline void broadcast_field(std::vector<PointSets>& sets, PointField f, const double* v, size_t n) {
  for (PointSets& ps : sets) (ps.*f).assign(v, v + n);
}
inline void slice_field(std::vector<PointSets>& sets, PointField f, const double* v, size_t n) {
  for (size_t k = 0; k < sets.size(); ++k) (sets[k].*f).assign(v + k * n, v + (k + 1) * n);
}

// whether ps holds exactly sd's counts (a collocation block filled on the device has no host points to count)
inline bool has_counts(const PointSets& ps, const SetDesc& sd, int n_out, bool device_colloc) {
  const size_t n_b = sd.n_b, n_u = sd.n_u, n_f = sd.n_f;
  return ps.Xlo.size() == 2 * n_b && ps.Xhi.size() == 2 * n_b && ps.Xu.size() == 2 * n_u && ps.U.size() == n_u * n_out &&
         (device_colloc || ps.Xf.size() == 2 * n_f);
}

// One set in the layout the kernels read: x[n_pad], t[n_pad], tg[n_out][n_pad] <- [pairs | data | collocation | pad] of ps,
// which holds sd's counts.  interleaved: the pairs stand as [lo_0, hi_0, lo_1, hi_1, ...] (the adr family: the partner of
// point g is g ^ 1), otherwise lo block, hi block.  device_colloc: the collocation block is filled on the device afterwards and
// gets lb as a placeholder.  Everything behind the collocation block is inert lb padding, and every tg entry that is no data
// target is zero; what else a caller keeps there (a Robin block, a source term) it lays on top.
inline void assemble_set(const PointSets& ps, const SetDesc& sd, int n_out, bool interleaved, bool device_colloc,
                         const double lb[2], double* x, double* t, double* tg) {
  const size_t n_pad = sd.n_pad;
  std::fill(tg, tg + (size_t)n_out * n_pad, 0.0);
  for (int i = 0; i < sd.n_b; ++i) {
    const int lo = interleaved ? 2 * i : i, hi = interleaved ? lo + 1 : sd.n_b + i;
    x[lo] = ps.Xlo[2 * i]; t[lo] = ps.Xlo[2 * i + 1];
    x[hi] = ps.Xhi[2 * i]; t[hi] = ps.Xhi[2 * i + 1];
  }
  for (int i = 0, g = data_first(sd); i < sd.n_u; ++i, ++g) {
    x[g] = ps.Xu[2 * i]; t[g] = ps.Xu[2 * i + 1];
    for (int o = 0; o < n_out; ++o) tg[(size_t)o * n_pad + g] = ps.U[(size_t)i * n_out + o];
  }
  const int first_pad = device_colloc ? colloc_first(sd) : sd.n_all;
  if (!device_colloc)
    for (int i = 0, g = colloc_first(sd); i < sd.n_f; ++i, ++g) { x[g] = ps.Xf[2 * i]; t[g] = ps.Xf[2 * i + 1]; }
  for (int g = first_pad; g < sd.n_pad; ++g) { x[g] = lb[0]; t[g] = lb[1]; }
}

// The affine map of the inputs to [-1, 1] in the compute type, x -> sx (x - lbx) - 1, and the box's two extents in float64
// (the device's Latin hypercube spreads its design over them).  Every launch takes its map from here.
template <typename real>
struct InMap {
  real lbx, lbt, sx, st;
  double ex, et;
  InMap(const double lb[2], const double ub[2])
      : lbx((real)lb[0]), lbt((real)lb[1]), sx(scale(lb[0], ub[0])), st(scale(lb[1], ub[1])), ex(ub[0] - lb[0]),
        et(ub[1] - lb[1]) {}

 private:
  static real scale(double lb, double ub) { return (real)(2.0 / (ub - lb)); }
};

}  // namespace pinn
