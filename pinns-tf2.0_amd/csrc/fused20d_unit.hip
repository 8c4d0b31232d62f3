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

// variant (ENS, SETS, SAW, ADR) at the depth of the net: PDE_ADR, pde 0 (the weighted loss) or pde 0 / 1
template <int H, bool ENS, bool SETS, bool SAW, bool ADR>
static int launch_h(int pde, const F20dLaunch& a, const f20d_nu_t<SETS, SAW, ADR ? PDE_ADR : 0>& nu) {
  if constexpr (ADR) return fused20d_launch<PDE_ADR, H, ENS, SETS, SAW>(a, nu);
  else if constexpr (SAW) return fused20d_launch<0, H, ENS, SETS, SAW>(a, nu);
  else return pde == 1 ? fused20d_launch<1, H, ENS, SETS, SAW>(a, nu) : fused20d_launch<0, H, ENS, SETS, SAW>(a, nu);
}
template <bool ENS, bool SETS, bool SAW, bool ADR>
static int launch_depth(int pde, const F20dLaunch& a, const f20d_nu_t<SETS, SAW, ADR ? PDE_ADR : 0>& nu) {
  switch (a.nd.n_hidden) {     // the AGPR stash holds (H - 2) x 40 registers: depths up to 8 fit the 256 of a wave
    case 4: return launch_h<4, ENS, SETS, SAW, ADR>(pde, a, nu);
    case 6: return launch_h<6, ENS, SETS, SAW, ADR>(pde, a, nu);
    case 8: return launch_h<8, ENS, SETS, SAW, ADR>(pde, a, nu);
    default: return (int)hipErrorInvalidValue;
  }
}

int fused20d_launch_any(int pde, const F20dLaunch& a, double nu) { return launch_depth<false, false, false, false>(pde, a, nu); }
int fused20d_ens_launch_any(int pde, const F20dLaunch& a, double nu) { return launch_depth<true, false, false, false>(pde, a, nu); }
int fused20d_ens_launch_any(int pde, const F20dLaunch& a, const double* nu_k) { return launch_depth<true, true, false, false>(pde, a, nu_k); }
int fused20d_launch_any(const F20dLaunch& a, const SaArgs& sa) { return launch_depth<false, false, true, false>(0, a, sa); }
int fused20d_launch_any(const F20dLaunch& a, const AdrCoef<double>& k) { return launch_depth<false, false, false, true>(0, a, k); }
// the trainable-coefficient kind: solo launch only
int fused20d_launch_any(const F20dLaunch& a, const AdrIdeArg& k) {
  switch (a.nd.n_hidden) {
    case 4: return fused20d_launch<PDE_ADR_IDE, 4, false, false, false>(a, k);
    case 6: return fused20d_launch<PDE_ADR_IDE, 6, false, false, false>(a, k);
    case 8: return fused20d_launch<PDE_ADR_IDE, 8, false, false, false>(a, k);
    default: return (int)hipErrorInvalidValue;
  }
}

// the adr kind with per-point loss weights: solo launch only
int fused20d_launch_any(const F20dLaunch& a, const AdrPwArgs& k) {
  switch (a.nd.n_hidden) {
    case 4: return fused20d_launch<PDE_ADR, 4, false, false, true>(a, k);
    case 6: return fused20d_launch<PDE_ADR, 6, false, false, true>(a, k);
    case 8: return fused20d_launch<PDE_ADR, 8, false, false, true>(a, k);
    default: return (int)hipErrorInvalidValue;
  }
}

}  // namespace pinn
