// fused20d_unit.hip -- translation unit of k_fused20d (see fused20d_api.h for why it is separate).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-slp-vectorize -mllvm -amdgpu-mfma-vgpr-form=1 -fPIC -c fused20d_unit.hip
#include "kernels_fused20d.h"

namespace pinn {

// entry e = 16 * block + 4 * i + j of a wave's block list -> flat parameter index (reference layout), -1 = padding
void fused20d_row_index(const NetDesc& nd, int H, int* out) {
  const int NBLK = fused20d_blocks(H), BLK_H = 5 + (H - 1) * 30;
  for (int e = 0; e < NBLK * 16; ++e) {
    const int blk = e >> 4, i = (e >> 2) & 3, j = e & 3;
    int idx = -1;
    if (blk < 5) {                                   // dense 0: rows (w0x, w0t, b0)
      const int f = 4 * blk + j;
      idx = i == 0 ? nd.off_w[0] + f : i == 1 ? nd.off_w[0] + FW + f : i == 2 ? nd.off_b[0] + f : -1;
    } else if (blk < BLK_H) {                        // hidden layer d: 25 weight blocks (m, n), 5 bias blocks
      const int r = blk - 5, d = 1 + r / 30, mn = r - (d - 1) * 30;
      if (mn < 25) { const int m = mn / 5, n = mn - 5 * m; idx = nd.off_w[d] + (4 * m + i) * FW + 4 * n + j; }
      else if (i == 0) idx = nd.off_b[d] + 4 * (mn - 25) + j;
    } else if (j == 0) {                             // dense H: one output column
      const int m = blk - BLK_H;
      idx = m < 5 ? nd.off_w[H] + 4 * m + i : (i == 0 ? nd.off_b[H] : -1);
    }
    out[e] = idx;
  }
}

// k_fused20d<PDE, H, ., ENS, SETS, SAW> at the depth of the net
template <int PDE, bool ENS, bool SETS, bool SAW>
static int launch_depth(const F20dLaunch& a, const f20d_slot_t<PDE, SETS, SAW>& nu) {
  switch (a.nd.n_hidden) {     // the AGPR stash holds (H - 2) x 40 registers: depths up to 8 fit the 256 of a wave
    case 4: return fused20d_launch<PDE, 4, ENS, SETS, SAW>(a, nu);
    case 6: return fused20d_launch<PDE, 6, ENS, SETS, SAW>(a, nu);
    case 8: return fused20d_launch<PDE, 8, ENS, SETS, SAW>(a, nu);
    default: return (int)hipErrorInvalidValue;
  }
}
// the Burgers kinds share their entry points (and their slot's type): pde 0 or 1 at run time
template <bool ENS, bool SETS>
static int launch_burgers(int pde, const F20dLaunch& a, const f20d_slot_t<0, SETS, false>& nu) {
  return pde == 1 ? launch_depth<1, ENS, SETS, false>(a, nu) : launch_depth<0, ENS, SETS, false>(a, nu);
}

int fused20d_launch_any(int pde, const F20dLaunch& a, double nu) { return launch_burgers<false, false>(pde, a, nu); }
int fused20d_ens_launch_any(int pde, const F20dLaunch& a, double nu) { return launch_burgers<true, false>(pde, a, nu); }
int fused20d_ens_launch_any(int pde, const F20dLaunch& a, const double* nu_k) { return launch_burgers<true, true>(pde, a, nu_k); }
// solo launches only: the weighted loss of pde 0, the adr kind, its trainable coefficients, its per-point weights, its Robin points, its source term, its coefficient fields
int fused20d_launch_any(const F20dLaunch& a, const SaArgs& sa) { return launch_depth<0, false, false, true>(a, sa); }
int fused20d_launch_any(const F20dLaunch& a, const AdrCoef<double>& k) { return launch_depth<PDE_ADR, false, false, false>(a, k); }
int fused20d_launch_any(const F20dLaunch& a, const AdrIdeArg& k) { return launch_depth<PDE_ADR_IDE, false, false, false>(a, k); }
int fused20d_launch_any(const F20dLaunch& a, const AdrPwArgs& k) { return launch_depth<PDE_ADR, false, false, true>(a, k); }
int fused20d_launch_any(const F20dLaunch& a, const AdrRobinArg<double>& k) { return launch_depth<PDE_ADR_ROBIN, false, false, false>(a, k); }
int fused20d_launch_any(const F20dLaunch& a, const AdrSrcArg<double>& k) { return launch_depth<PDE_ADR_SRC, false, false, false>(a, k); }
int fused20d_launch_any(const F20dLaunch& a, const AdrVarArg<double>& k) { return launch_depth<PDE_ADR_VAR, false, false, false>(a, k); }
// the adr kind's ensemble launch: a row of coefficients per member, the point set shared or one per member
int fused20d_ens_launch_any(const F20dLaunch& a, const AdrEnsArg& k, bool sets) {
  return sets ? launch_depth<PDE_ADR_ENS, true, true, false>(a, k) : launch_depth<PDE_ADR_ENS, true, false, false>(a, k);
}

}  // namespace pinn
