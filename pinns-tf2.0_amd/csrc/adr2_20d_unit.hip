// adr2_20d_unit.hip -- translation unit of k_adr2_20d: the text of k_fused20d (kernels_fused20d_kernel.h) under a name and in
// a code object of its own, for the adr2 kind (PDE_ADR2, kernels_generic.h: u_xx + kappa u_tt as the fourth Taylor channel,
// three-term wall points).  PDE_ADR_SRC's variant of the text -- wall block behind the collocation block, source in tgt, both
// counts may be 0 -- with kappa read inside every layer of both sweeps.  Depths 4, 6 and 8, one tile per workgroup and tile loop.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-slp-vectorize -mllvm -amdgpu-mfma-vgpr-form=1 -fPIC -c adr2_20d_unit.hip
#include "kernels_fused20d.h"

namespace pinn {

#define PINN_F20D_SPLIT 0
#define PINN_F20D_KERNEL k_adr2_20d
#include "kernels_fused20d_kernel.h"
#undef PINN_F20D_KERNEL
#undef PINN_F20D_SPLIT

// fused20d_launch's plan for k_adr2_20d<PDE_ADR2, H, .>: the one-tile instantiation when each tile has a workgroup of its own,
// the tile loop otherwise
template <int H>
static int adr2_20d_launch(const F20dLaunch& a, const Adr2Arg<double>& nu) {
  if (!w20_layout_ok(a.nd, H, 0) || a.n_members != 1 || a.split) return (int)hipErrorInvalidValue;
  const size_t lds = fused20d_lds_bytes(H, a.nd.n_theta);
  static unsigned long long attr_set = 0;
  if (first_call_on_device(attr_set)) {
    hipError_t e = hipFuncSetAttribute((const void*)&k_adr2_20d<PDE_ADR2, H, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e == hipSuccess)
      e = hipFuncSetAttribute((const void*)&k_adr2_20d<PDE_ADR2, H, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  const int n_tiles = a.sd.n_pad / 64;
  auto* const kern = a.n_wg >= n_tiles ? &k_adr2_20d<PDE_ADR2, H, true> : &k_adr2_20d<PDE_ADR2, H, false>;
  const dim3 grid(a.n_wg, 1);
  if (a.ev_start && a.ev_stop)
    hipExtLaunchKernelGGL(kern, grid, dim3(256), lds, a.stream, a.ev_start, a.ev_stop, 0, a.th, a.xs, a.ts, a.tgt, a.part,
                          a.row_index, a.R, n_tiles, a.lbx, a.lbt, a.sx, a.st, nu, a.sd, a.stamps, w20_desc(H, 0));
  else
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, a.stream, a.th, a.xs, a.ts, a.tgt, a.part, a.row_index, a.R, n_tiles,
                       a.lbx, a.lbt, a.sx, a.st, nu, a.sd, a.stamps, w20_desc(H, 0));
  return (int)hipGetLastError();
}

int adr2_20d_launch_any(const F20dLaunch& a, const Adr2Arg<double>& k) {
  switch (a.nd.n_hidden) {
    case 4: return adr2_20d_launch<4>(a, k);
    case 6: return adr2_20d_launch<6>(a, k);
    case 8: return adr2_20d_launch<8>(a, k);
    default: return (int)hipErrorInvalidValue;
  }
}

}  // namespace pinn
