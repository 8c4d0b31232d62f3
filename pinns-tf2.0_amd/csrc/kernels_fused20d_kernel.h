// kernels_fused20d_kernel.h -- the body of k_fused20d.  The text is one and the name is one: every kind and variant is a set
// of template arguments <PDE, H, ONE_TILE, ENS, SETS, SAW> of k_fused20d, and the type of its coefficient slot comes from the
// trait F20dArg (kernels_fused20d.h).  A new variant is a new set of arguments under the same name -- a new template value,
// a specialisation of the trait where its slot differs -- and never one more inclusion.  It has to show, in the device-code
// listing (tests/helpers/isa_lint.py --listing) before and after, that every earlier line is unchanged, and it adds its row
// to the variant table of tests/test_isa_hazards.py, which pins the set of instantiations by their arguments.
// kernels_fused20d.h includes the text a second time with PINN_F20D_SPLIT = 1, as k_split20d: the one-tile kernel of pde 0
// and 1 with two roles compiled in (fused20d_api.h: the split launch), a preprocessor switch because the roles differ in
// text.  The reverse sweep stands in kernels_fused20d_reverse.h, included below once per role; with PINN_F20D_SPLIT = 0 it
// is included once, as the whole sweep.  (Not a __device__ body called from two kernels: such a wrapper changed the schedule
// of the instantiations.)  No include guard: it is meant to be included twice.
template <int PDE, int H, bool ONE_TILE, bool ENS = false, bool SETS = false, bool SAW = false>
__global__ __launch_bounds__(256) void PINN_F20D_KERNEL(const double* __restrict__ th, const double* __restrict__ xs,
                                                  const double* __restrict__ ts, const double* __restrict__ tgt,
                                                  double* __restrict__ part, const int* __restrict__ row_index, int R,
                                                  int n_tiles, double lbx, double lbt, double sx, double st,
                                                  f20d_slot_t<PDE, SETS, SAW> nu, SetDesc sd,
                                                  long long* __restrict__ stamps, W20Desc nd_arg) {
  static_assert(ENS || !SETS, "per-member point sets are an ensemble launch");
  static_assert(!pde_is_adr(PDE) || PDE == PDE_ADR_ENS || (!ENS && !SETS && (!SAW || PDE == PDE_ADR)),
                "advection-diffusion-reaction: solo launch; point weights for the fixed-coefficient kind only");
  static_assert(PDE != PDE_ADR_ENS || (ENS && !SAW && !PINN_F20D_SPLIT),
                "adr ensemble members: an ensemble launch, shared or per-member point sets, no point weights");
  static_assert(!SAW || ((PDE == 0 || PDE == PDE_ADR) && !ENS), "point weights: Burgers inference or adr, solo launch");
  static_assert(PDE != PDE_ADR_ROBIN || (!ENS && !SETS && !SAW),
                "Robin points: the fixed-coefficient adr kind only, solo launch, no point weights");
  static_assert(PDE != PDE_ADR_SRC || (!ENS && !SETS && !SAW),
                "source term: the fixed-coefficient adr kind only, solo launch, no point weights");
  static_assert(PDE != PDE_ADR2 || (!ENS && !SETS && !SAW && !PINN_F20D_SPLIT),
                "adr2 (u_xx + kappa u_tt as one channel): solo launch, no point weights");
  static_assert(PDE != PDE_ADR_VAR || (!ENS && !SETS && !SAW),
                "coefficient fields: the adr kind only, solo launch, no point weights (no SAW)");
  // weight offsets: compile-time constants in the one-tile variant (immediate operands; Adam step 41.9 -> 40.8 us with
  // the preloaded pointers); the tile-loop variant keeps them in SGPRs -- with immediates its schedule came out 9 %
  // slower (N_f = 10^6: 2104 vs 1930 us per step, same box)
  constexpr W20Desc nd_const = w20_desc(H, pde_n_tail(PDE));
  const W20Desc nd = ONE_TILE ? nd_const : nd_arg;
  constexpr int NBLK = fused20d_blocks(H);
  constexpr int BLK_H = 5 + (H - 1) * 30;            // first block of dense H
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  double* const wl = reinterpret_cast<double*>(lds_raw);
  const int nwp = (nd.n_theta + 127) / 128 * 128;
  if constexpr (ENS) {
    th += (size_t)blockIdx.y * nwp;
    part += (size_t)blockIdx.y * gridDim.x * R;
    if constexpr (SETS) {                             // before the first tile's coordinate prefetch below
      const size_t po = (size_t)blockIdx.y * sd.n_pad;
      xs += po; ts += po; tgt += po;
    }
  }
  // PDE_ADR_ENS: this member's row of the coefficient table, wave-uniform, read here -- in front of everything that writes
  // memory -- so that the six arrive by scalar loads and stand in scalar registers as PDE_ADR's by-value AdrCoef does
  f20d_ens_coef_t<PDE> ens_k;
  if constexpr (PDE == PDE_ADR_ENS) {
    const double* __restrict__ const kr = nu.coef + (size_t)blockIdx.y * ADR_ENS_ROW;
    ens_k = AdrCoef<double>{kr[0], kr[1], kr[2], kr[3], kr[4], kr[5]};
  }
  (void)ens_k;
  double* const gacc_all = wl + nwp;                  // tile loop: 4 x NBLK x 16 accumulators; one tile: 2 staging buffers
  double* const lacc_all = gacc_all + (ONE_TILE ? fused20d_stage_doubles(H) : 4 * NBLK * 16);

#define PINN_TO_POINTS(X) mfma444((X), ident, 0.0)
  STAMP(0);
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // per-lane indices as a macro: derived here for the prologue and the epilogue, and again inside the tile loop (declared
  // once in front of the loop instead, the same values, every instantiation comes out with another schedule)
#define PINN_LANE_INDICES(L)                                                                                          \
  const int lane = (L);                                                                                                \
  const int q = lane & 15;                 /* point of this wave's 16 */                                              \
  const int s = lane >> 4;                 /* feature slot: feature = 4 * group + s */                                \
  const int i4 = lane & 3;                 /* row / column slot of the A patterns and of the gradient blocks */       \
  const int pf = s * FW + i4;              /* forward pattern:  W[4m + s][4n + i4] */                                 \
  const int pr = i4 * FW + s;              /* reverse pattern:  W[4m + i4][4n + s] */                                 \
  const double ident = s == i4 ? 1.0 : 0.0;                    /* 4 x 4 identity as a B operand: the transposing matrix instruction */ \
  const int ge = s * 4 + i4;               /* this lane's entry (i, j) of a gradient block */                         \
  double* const lacc = lacc_all + wave * 256 + lane;                        /* [k * 64]: l_res, l_dat, dl0, dl1 */     \
  const int sput = (s * 4 + i4) * 4 + ((lane >> 2) & 3);   /* one-tile staging slot: entry-major, the four blocks of an entry adjacent */ \
  const double onesA = i4 == 0 ? 1.0 : 0.0;                     /* rotated "ones" in-group: row 0 = 1 (bias gradients) */ \
  (void)q; (void)pf; (void)pr; (void)ident; (void)ge; (void)lacc; (void)onesA; (void)s; (void)sput
  PINN_LANE_INDICES(tid & 63);
  double* const gacc = gacc_all + wave * (NBLK * 16);

  // first tile's coordinates: issued ahead of the weight staging, so the two round trips overlap
  int tile = blockIdx.x;
#if PINN_F20D_SPLIT
  // Two roles, chosen per workgroup (wave-uniform): blocks [0, n_tiles) are the main workgroups of tile blockIdx.x, block
  // n_tiles + j is a helper that serves tile 2 j and then tile 2 j + 1 (where there is one).  A helper recomputes the tile's
  // forward sweep and seeds from the kernel's inputs -- the same instructions, hence the same bits -- and writes the columns of
  // the tile's gradient row that f20d_split_owner (fused20d_api.h) gives it; the main workgroup writes the others.  Neither
  // waits for the other or reads what it wrote.
  static_assert(ONE_TILE && !ENS && !SETS && !SAW && (PDE == 0 || PDE == 1) && PINN_ONETILE_SUM == 0,
                "the split launch: one tile per workgroup, solo, Burgers kinds, unfolded phase sums");
  static_assert(f20d_split_ok(H, pde_n_tail(PDE)), "every column of a gradient row has exactly one owner");
  const bool helper = (int)blockIdx.x >= n_tiles;
  if (helper) tile = 2 * ((int)blockIdx.x - n_tiles);
#endif
  double x = 0.0, t = 0.0;
  if (tile < n_tiles) { x = xs[tile * 64 + wave * 16 + q]; t = ts[tile * 64 + wave * 16 + q]; }

  // ---- flat weight vector -> LDS by asynchronous LDS-DMA (global_load_lds_dwordx4: 1 KiB per wave instruction, no
  // registers; the engine pads the vector's allocation to whole pieces), gradient accumulators <- 0 meanwhile
  for (int c = wave; c < nwp / 128; c += 4)
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(th + c * 128 + lane * 2),
                                     (__attribute__((address_space(3))) void*)(wl + c * 128), 16, 0, 0);
  {
    typedef double d2 __attribute__((ext_vector_type(2)));
    if (ONE_TILE) {                                    // the staging buffers are written before they are read: loss parts only
      d2* const z = reinterpret_cast<d2*>(lacc_all);
      for (int i = tid; i < 2 * 256; i += 256) z[i] = d2{0.0, 0.0};
    } else {
      d2* const z = reinterpret_cast<d2*>(gacc_all);
      for (int i = tid; i < 2 * NBLK * 16 + 2 * 256; i += 256) z[i] = d2{0.0, 0.0};   // + the loss-part slots behind them
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  double c1 = 1.0, c2 = f20d_nu(nu);
  if (PDE == 1) { c1 = wl[nd.n_net]; c2 = exp(wl[nd.n_net + 1]); }
  // PDE_ADR2: kappa is read inside every layer of both sweeps (channels_pde_d, preact_adjoint_pde_d): a scalar pair
  const double kap = f20d_kappa(nu);
  (void)kap;
  // SAW, tile loop: the weight array and the ascent step size are held in vector registers (an opaque move): the tile-loop
  // variants use 96 of the 106 scalar registers already, and with these four more they spilled 2-4 of them
  double* sa_lam_p = nullptr;
  double sa_alpha = 0.0;
  if constexpr (SAW) {
    sa_lam_p = nu.lam;
    if constexpr (PDE == PDE_ADR) sa_alpha = nu.bc; else sa_alpha = nu.alpha;
    if constexpr (!ONE_TILE) asm volatile("" : "+v"(sa_lam_p), "+v"(sa_alpha));
  }
  const double inv_nf = sd.inv_nf, inv_nu = sd.inv_nu;
  // PDE_ADR, tile loop: the six coefficients and 1 / n_b would take 14 more scalar registers than the 96 of 106 these
  // variants use already (6 of them spilled): every wave parks its own copy in the fourth quarter of its loss-part slots
  // (lacc[192..], used when PDE == 1 only) and reads it back per tile through an opaque address, wave-uniform.  One tile
  // per workgroup: they stay in scalar registers.
  double* adr_park = nullptr;
  if constexpr (PDE == PDE_ADR && !ONE_TILE && !SAW) {
    adr_park = lacc_all + wave * 256 + 192;
    if ((tid & 63) == 0) {
      adr_park[0] = nu.a0; adr_park[1] = nu.a1; adr_park[2] = nu.nu; adr_park[3] = nu.r1; adr_park[4] = nu.r2;
      adr_park[5] = nu.r3; adr_park[6] = sd.inv_nb;
    }
  }
  // PDE_ADR_ENS, tile loop: the same seven, the six from the member's row
  if constexpr (PDE == PDE_ADR_ENS && !ONE_TILE) {
    adr_park = lacc_all + wave * 256 + 192;
    if ((tid & 63) == 0) {
      adr_park[0] = ens_k.a0; adr_park[1] = ens_k.a1; adr_park[2] = ens_k.nu; adr_park[3] = ens_k.r1; adr_park[4] = ens_k.r2;
      adr_park[5] = ens_k.r3; adr_park[6] = sd.inv_nb;
    }
  }
  // PDE_ADR_ROBIN, PDE_ADR_SRC and PDE_ADR_VAR, tile loop: the same seven and the Robin block's first point, length and 1 / N_w; the (alpha, beta) array's
  // address in vector registers (an opaque move), as SAW holds its array's
  const double* rb_ab = nullptr;
  if constexpr (pde_adr_robin(PDE)) {
    rb_ab = nu.ab;
    if constexpr (!ONE_TILE) {
      asm volatile("" : "+v"(rb_ab));
      adr_park = lacc_all + wave * 256 + 192;
      if ((tid & 63) == 0) {
        adr_park[0] = nu.k.a0; adr_park[1] = nu.k.a1; adr_park[2] = nu.k.nu; adr_park[3] = nu.k.r1; adr_park[4] = nu.k.r2;
        adr_park[5] = nu.k.r3; adr_park[6] = sd.inv_nb; adr_park[7] = (double)nu.first; adr_park[8] = (double)nu.n;
        adr_park[9] = nu.inv_nw;
        if constexpr (PDE == PDE_ADR2) adr_park[10] = nu.b;     // b beside the other ten (kappa: above)
      }
    }
  }
  (void)rb_ab;
  // PDE_ADR_VAR: the coefficient table's address; tile loop: in vector registers too (the src variants sit at 104 of the 106
  // scalar registers)
  const double* kf_tab = nullptr;
  if constexpr (PDE == PDE_ADR_VAR) {
    kf_tab = nu.kf;
    if constexpr (!ONE_TILE) asm volatile("" : "+v"(kf_tab));
  }
  (void)kf_tab;
  if constexpr (PDE == PDE_ADR_IDE) {
    adr_park = lacc_all + wave * 256 + 192;
    if ((tid & 63) == 0) {
      const double* const tail = wl + nd.n_theta - 6;
      adr_park[0] = tail[0]; adr_park[1] = tail[1]; adr_park[2] = exp(tail[2]); adr_park[3] = tail[3]; adr_park[4] = tail[4];
      adr_park[5] = tail[5]; adr_park[6] = sd.inv_nb; adr_park[7] = (double)nu.mask;
    }
  }
  // PDE_ADR with point weights, both variants: the same seven, and behind them the array's header (beta1, beta2, eps and the
  // ascent rates by point class, fused20d_api.h PW_CONST) -- a lane picks its class's rate by one LDS read
  if constexpr (PDE == PDE_ADR && SAW) {
    adr_park = lacc_all + wave * 256 + 192;
    const AdrCoef<double> k0 = nu.k;
    if ((tid & 63) == 0) {
      adr_park[0] = k0.a0; adr_park[1] = k0.a1; adr_park[2] = k0.nu; adr_park[3] = k0.r1; adr_park[4] = k0.r2;
      adr_park[5] = k0.r3; adr_park[6] = sd.inv_nb;
    }
    if ((tid & 63) < PW_CONST) adr_park[8 + (tid & 63)] = sa_lam_p[tid & 63];
  }
  (void)adr_park;
  // per-lane partial sums of the loss parts and of the two lambda gradients (slot-0 lanes only) live in LDS, four
  // slots per lane behind the gradient accumulators: one read-modify-write per tile instead of eight registers held
  // across the whole kernel (which cost the identification variant 20 B of scratch per lane)

  // Gradient blocks.  D = this lane's partial sum over the four points of its block b.  Tile loop: the four blocks of an
  // entry are folded with DPP row rotations and added into the wave's accumulator by ds_add_f64 (grad_store / gacc_flush
  // below; PINN_GACC_ATOMIC = 0: the old accumulator values are fetched BEFORE the matrix instructions that produce D,
  // grad_fetch, and old + D is written back).  One tile: parked, and summed by the whole workgroup (phase_issue / phase_finish).
  // (Tried in round 2: ds_add_f64 with the four lanes of an entry hitting one address, no fold, no read-modify-write --
  //  221 instructions instead of ~3000, bit-reproducible over 200 runs, and 14 % SLOWER: 49.8 vs 43.7 us per step.)

  STAMP(1);

  for (; tile < n_tiles; tile += PINN_F20D_SPLIT ? 1 : gridDim.x) {
#if PINN_F20D_SPLIT
    // the helper's second tile makes this a real loop: the thread index is re-read through an opaque move once per tile, so
    // that the per-lane addresses derived from it are formed inside the loop, not held (and spilled) across it
    int tid_tile = threadIdx.x;
    asm volatile("" : "+v"(tid_tile));
    const int tid = tid_tile;
#endif
    PINN_LANE_INDICES(tid & 63);
    auto grad_fetch = [&](const int blk) { return (ONE_TILE || PINN_GACC_ATOMIC) ? 0.0 : gacc[blk * 16 + ge]; };
    // One tile per workgroup: nothing is accumulated, so the four blocks are not folded in registers (2 x 2 DPP moves + 2
    // adds per block, 1 300 instructions per tile): every lane parks its own partial in the phase's staging buffer
    // (entry-major: the four blocks of an entry adjacent), and phase_issue / phase_finish add blocks and waves with the whole
    // workgroup.  (PINN_ONETILE_SUM = 1, 2, measured and dropped: ROR4 then ROR8, block 1 parks (b1 + b0) + (b3 + b2).)
    int phase_first = 0;
    constexpr int PARK_BLOCK = 1;
    // phase p of the reverse sweep (0: dense H, H - d: layer d's 30 blocks, H: dense 0) -> its first block / its staging area
    // (the waves are FUSED20D_STAGE_WAVE apart when every lane parks, adjacent doubles when the totals do)
    constexpr int STAGE_WAVE_STRIDE = PINN_ONETILE_SUM ? 1 : FUSED20D_STAGE_WAVE;
#if PINN_ONETILE_SUM == 2
#define PINN_PHASE_STAGE(P) ((P) == 0 ? BLK_H : (P) == H ? 0 : 5 + (H - (P) - 1) * 30) * 64
#else
#define PINN_PHASE_STAGE(P) ((P) & 1) * FUSED20D_STAGE_BUF
#endif
    double* stage_w = gacc_all + wave * STAGE_WAVE_STRIDE;
    // Tile loop (PINN_GACC_ATOMIC): after PINN_FOLD_STAGES DPP folds the lanes of blocks 0 and 1 (one fold: two lanes per address, resolved in
    // lane order) or of block 0 (two folds: one adder per address and tile) add the total into the wave's accumulator with
    // ONE ds_add_f64.  A group's stores share one hand-set execution-mask region: as `if (block 0) atomic` every store became its own basic block (two scalar
    // instructions each, and the stash reads the compiler shares between a layer's rotated inputs and the next layer's
    // adjoints were issued twice: 9 233 -> 9 766 instructions).  LDS operations the compiler does not see only make its own
    // lgkmcnt waits conservative (the queue is in order).  (The UNFOLDED form -- four lanes per address -- was 14 % slower
    // in round 2; this one follows the fold.)
    constexpr unsigned long long FOLD_LANES = PINN_FOLD_STAGES == 2 ? 0x000f000f000f000full : 0x00ff00ff00ff00ffull;
    double pend_D[6] = {0, 0, 0, 0, 0, 0};
    int pend_off[6] = {0, 0, 0, 0, 0, 0}, pend_n = 0;
    auto gacc_flush = [&]() {
#if PINN_GACC_ATOMIC
      if constexpr (!ONE_TILE) {
        const unsigned addr = (unsigned)(uintptr_t)(__attribute__((address_space(3))) void*)(gacc + ge);
        unsigned long long saved;
        if (pend_n == 6)
          asm volatile("s_mov_b64 %[sv], exec\n\ts_mov_b64 exec, %[mk]\n\t"
                       "ds_add_f64 %[a], %[d0] offset:%[o0]\n\tds_add_f64 %[a], %[d1] offset:%[o1]\n\t"
                       "ds_add_f64 %[a], %[d2] offset:%[o2]\n\tds_add_f64 %[a], %[d3] offset:%[o3]\n\t"
                       "ds_add_f64 %[a], %[d4] offset:%[o4]\n\tds_add_f64 %[a], %[d5] offset:%[o5]\n\t"
                       "s_mov_b64 exec, %[sv]"
                       : [sv] "=&s"(saved)
                       : [a] "v"(addr), [mk] "s"(FOLD_LANES), [d0] "v"(pend_D[0]), [d1] "v"(pend_D[1]),
                         [d2] "v"(pend_D[2]), [d3] "v"(pend_D[3]), [d4] "v"(pend_D[4]), [d5] "v"(pend_D[5]),
                         [o0] "i"(pend_off[0]), [o1] "i"(pend_off[1]), [o2] "i"(pend_off[2]), [o3] "i"(pend_off[3]),
                         [o4] "i"(pend_off[4]), [o5] "i"(pend_off[5])
                       : "memory");
        else
          asm volatile("s_mov_b64 %[sv], exec\n\ts_mov_b64 exec, %[mk]\n\t"
                       "ds_add_f64 %[a], %[d0] offset:%[o0]\n\tds_add_f64 %[a], %[d1] offset:%[o1]\n\t"
                       "ds_add_f64 %[a], %[d2] offset:%[o2]\n\tds_add_f64 %[a], %[d3] offset:%[o3]\n\t"
                       "ds_add_f64 %[a], %[d4] offset:%[o4]\n\t"
                       "s_mov_b64 exec, %[sv]"
                       : [sv] "=&s"(saved)
                       : [a] "v"(addr), [mk] "s"(FOLD_LANES), [d0] "v"(pend_D[0]), [d1] "v"(pend_D[1]),
                         [d2] "v"(pend_D[2]), [d3] "v"(pend_D[3]), [d4] "v"(pend_D[4]),
                         [o0] "i"(pend_off[0]), [o1] "i"(pend_off[1]), [o2] "i"(pend_off[2]), [o3] "i"(pend_off[3]),
                         [o4] "i"(pend_off[4])
                       : "memory");
      }
#endif
#if PINN_ONETILE_SUM
      if constexpr (ONE_TILE) {
        const unsigned addr = (unsigned)(uintptr_t)(__attribute__((address_space(3))) void*)(stage_w + ge * 4);
        constexpr unsigned long long park = 0x000f000f000f000full << (4 * PARK_BLOCK);
        unsigned long long saved;
        if (pend_n == 6)
          asm volatile("s_mov_b64 %[sv], exec\n\ts_mov_b64 exec, %[mk]\n\t"
                       "ds_write2st64_b64 %[a], %[d0], %[d1] offset0:%[o0] offset1:%[o1]\n\t"
                       "ds_write2st64_b64 %[a], %[d2], %[d3] offset0:%[o2] offset1:%[o3]\n\t"
                       "ds_write2st64_b64 %[a], %[d4], %[d5] offset0:%[o4] offset1:%[o5]\n\t"
                       "s_mov_b64 exec, %[sv]"
                       : [sv] "=&s"(saved)
                       : [a] "v"(addr), [mk] "s"(park), [d0] "v"(pend_D[0]), [d1] "v"(pend_D[1]),
                         [d2] "v"(pend_D[2]), [d3] "v"(pend_D[3]), [d4] "v"(pend_D[4]), [d5] "v"(pend_D[5]),
                         [o0] "i"(pend_off[0]), [o1] "i"(pend_off[1]), [o2] "i"(pend_off[2]), [o3] "i"(pend_off[3]),
                         [o4] "i"(pend_off[4]), [o5] "i"(pend_off[5])
                       : "memory");
        else
          asm volatile("s_mov_b64 %[sv], exec\n\ts_mov_b64 exec, %[mk]\n\t"
                       "ds_write2st64_b64 %[a], %[d0], %[d1] offset0:%[o0] offset1:%[o1]\n\t"
                       "ds_write2st64_b64 %[a], %[d2], %[d3] offset0:%[o2] offset1:%[o3]\n\t"
                       "ds_write_b64 %[a], %[d4] offset:%[o4] * 512\n\t"
                       "s_mov_b64 exec, %[sv]"
                       : [sv] "=&s"(saved)
                       : [a] "v"(addr), [mk] "s"(park), [d0] "v"(pend_D[0]), [d1] "v"(pend_D[1]),
                         [d2] "v"(pend_D[2]), [d3] "v"(pend_D[3]), [d4] "v"(pend_D[4]),
                         [o0] "i"(pend_off[0]), [o1] "i"(pend_off[1]), [o2] "i"(pend_off[2]), [o3] "i"(pend_off[3]),
                         [o4] "i"(pend_off[4])
                       : "memory");
      }
#endif
      pend_n = 0;
    };
    auto grad_store = [&](double D, const double old, const int blk) {
#if PINN_ONETILE_SUM
      if (ONE_TILE) {
        D += dpp_mov<DPP_ROW_ROR4>(D);
        D += dpp_mov<DPP_ROW_ROR8>(D);
        pend_D[pend_n] = D; pend_off[pend_n] = blk - phase_first; ++pend_n;   // in blocks of 64 doubles (ds_write2st64_b64), parked by gacc_flush below
        return;
      }
#else
      if (ONE_TILE) { stage_w[(blk - phase_first) * 64 + sput] = D; return; }
#endif
      D += dpp_mov<DPP_ROW_ROR8>(D);
#if PINN_GACC_ATOMIC
      if (PINN_FOLD_STAGES == 2) D += dpp_mov<DPP_ROW_ROR4>(D);       // (1: the LDS adder does the rest of the fold)
      pend_D[pend_n] = D; pend_off[pend_n] = blk * 128; ++pend_n;      // added by gacc_flush below, one execution-mask region per group
      (void)old;
#else
      D += dpp_mov<DPP_ROW_ROR4>(D);
      gacc[blk * 16 + ge] = old + D;
#endif
    };
    // entries of a hidden layer's 30 blocks, relative to the layer's first weight: the same for every layer, derived once.
    // Thread t owns entries t and t + 256 of a phase.
    int rel_hidden[2] = {-1, -1};
    if (ONE_TILE) {
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int e = tid + 256 * k, bl = e >> 4, i = (e >> 2) & 3, j = e & 3;
        if (bl < 25) { const int m = bl / 5, n = bl - 5 * m; rel_hidden[k] = (4 * m + i) * FW + 4 * n + j; }
        else if (bl < 30 && i == 0) rel_hidden[k] = FW * FW + 4 * (bl - 25) + j;       // the bias row follows the kernel
      }
    }
    double* __restrict__ const row1 = part + (size_t)(PINN_F20D_SPLIT ? tile : blockIdx.x) * R;
    // sum of one phase p: all four waves have parked its blocks in the phase's staging area; entry e of the phase = 4 waves x 4
    // blocks in fixed order -> its place in the workgroup's gradient row.  to_index(e) = flat parameter index or -1.
    //   phase_issue   barrier (all four waves have parked the phase) + the 16 reads of this thread's two entries
    //   phase_finish  4 waves x 4 blocks added in fixed order, stored at the entry's place in the workgroup's gradient row
    // Threads without a second entry read a clamped address and store nothing (no divergent branch around the reads).
    // Folded settings: an entry is the four waves' totals, ps_lo[k][0] = (w0, w1), ps_hi[k][0] = (w2, w3), 4 reads; their
    // parking stores are inline asm, which hipcc's wait-count pass does not count, so the wait in front of the barrier is
    // written out; with PINN_ONETILE_SUM = 2 issue and finish do nothing and all phases are summed behind the sweep.
    typedef double d2 __attribute__((ext_vector_type(2)));
    constexpr int PS_W = PINN_ONETILE_SUM ? 1 : 4;
    d2 ps_lo[2][PS_W], ps_hi[2][PS_W];
    auto phase_reads = [&](const int n_entries, const int p) {
      const double* __restrict__ const sb = gacc_all + PINN_PHASE_STAGE(p);
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        if (256 * k >= n_entries) continue;
        const int e = tid + 256 * k < n_entries ? tid + 256 * k : n_entries - 1;
#if PINN_ONETILE_SUM
        ps_lo[k][0] = *reinterpret_cast<const d2*>(sb + 4 * e);
        ps_hi[k][0] = *reinterpret_cast<const d2*>(sb + 4 * e + 2);
#else
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          ps_lo[k][w] = *reinterpret_cast<const d2*>(sb + w * FUSED20D_STAGE_WAVE + 4 * e);
          ps_hi[k][w] = *reinterpret_cast<const d2*>(sb + w * FUSED20D_STAGE_WAVE + 4 * e + 2);
        }
#endif
      }
    };
    auto parked_barrier = [&]() {
      if (PINN_ONETILE_SUM) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __syncthreads();
    };
    auto phase_issue = [&](const int n_entries, const int p) {
      if (PINN_ONETILE_SUM == 2) return;                 // summed behind the sweep
      parked_barrier();
      phase_reads(n_entries, p);
    };
    auto phase_adds = [&](const int n_entries, auto to_index) {
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        if (256 * k >= n_entries) continue;
        const int e = tid + 256 * k;
        const int idx = e < n_entries ? to_index(e, k) : -1;
        double v = 0.0;
#if PINN_ONETILE_SUM
        v = ((ps_lo[k][0].x + ps_lo[k][0].y) + ps_hi[k][0].x) + ps_hi[k][0].y;
#else
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          const double t = (ps_lo[k][w].x + ps_lo[k][w].y) + (ps_hi[k][w].x + ps_hi[k][w].y);
          v = w == 0 ? t : v + t;
        }
#endif
        // (as a nontemporal store -- the row streaming past the L2 -- the Adam step was 0.6 us LONGER,
        //  profiles/r06_ab_loopvariants.txt; written through, it is shorter: PINN_ROW_STORE_WT)
#if PINN_ROW_STORE_WT
        if (idx >= 0) __hip_atomic_store(row1 + idx, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
        if (idx >= 0) row1[idx] = v;
#endif
      }
    };
    auto phase_finish = [&](const int n_entries, auto to_index) {
      if (PINN_ONETILE_SUM == 2) return;
      phase_adds(n_entries, to_index);
    };
    auto idx_dense_h = [&](const int e, int) {
      const int m = e >> 4, i = (e >> 2) & 3, j = e & 3;
      return j != 0 ? -1 : m < 5 ? nd.off_w[H] + 4 * m + i : (i == 0 ? nd.off_b[H] : -1);
    };
    const int pt = tile * 64 + wave * 16 + q;
    // SAW: this point's weight (and, in an Adam step, its moments), requested here so that the forward sweep hides the
    // round trip
    double sa_lam = 1.0, sa_m = 0.0, sa_v = 0.0;
    double* sa_row = nullptr;
    if constexpr (SAW && PDE == PDE_ADR) {   // indexed by the point; both points of a periodic pair read the lo point's entry
      const int e = pt < sd.n_all ? pt : 0;
      sa_row = sa_lam_p + PW_CONST + 3 * (e < 2 * sd.n_b ? e & ~1 : e);
      sa_lam = sa_row[0]; sa_m = sa_row[1]; sa_v = sa_row[2];
    } else
    if constexpr (SAW) {      // (padding lanes read point 0's entry, unused: no branch, no saved execution mask)
      sa_row = sa_lam_p + SA_CONST + 3 * (pt < sd.n_all ? pt : 0);
      sa_lam = sa_row[0]; sa_m = sa_row[1]; sa_v = sa_row[2];
    }
    const double hx = __builtin_fma(sx, x - lbx, -1.0), ht = __builtin_fma(st, t - lbt, -1.0);
    {
      const int nt = tile + gridDim.x;
      if (!ONE_TILE && nt < n_tiles) { x = xs[nt * 64 + wave * 16 + q]; t = ts[nt * 64 + wave * 16 + q]; }
    }

    // ------------------------------------------------------------------ forward
    double in[4][5];                         // [channel h,p,q,r][group]: outputs of the layer below, own (slot, point)
    double a0[5];                            // layer 0: tanh outputs (its z_x, z_t are weight constants, z_xx = 0)
    agd stash[H][5][4];                      // AGPR-resident, layers 1..H-2
    double top[5][4];                        // last hidden layer's stash entry, live across the seeds
#pragma unroll
    for (int n = 0; n < 5; ++n) {            // dense 0: p0 = (sx, 0), q0 = (0, st), r0 = 0
      const int f = 4 * n + s;
      const double w0x = wl[nd.off_w[0] + f], w0t = wl[nd.off_w[0] + FW + f], b0 = wl[nd.off_b[0] + f];
      const double a = tanh_d(__builtin_fma(hx, w0x, __builtin_fma(ht, w0t, b0)));
      a0[n] = a;
      channels_pde_d<PDE>(a, sx * w0x, st * w0t, 0.0, kap, in[0][n], in[1][n], in[2][n], in[3][n]);
    }
#pragma unroll
    for (int d = 1; d < H; ++d) {
      const double* __restrict__ wd = wl + nd.off_w[d] + pf;
      double acc[4][5];
#pragma unroll
      for (int n = 0; n < 5; ++n) {
        acc[0][n] = wl[nd.off_b[d] + 4 * n + s];
        acc[1][n] = acc[2][n] = acc[3][n] = 0.0;
      }
      // The 25 weight patterns of the layer are requested from LDS TWO steps ahead of the four matrix instructions that
      // consume them (sched_barrier pins the order).  Left to itself hipcc sinks every ds_read next to its consumer --
      // `ds_read2_b64; s_waitcnt lgkmcnt(0); v_mfma` 259 times per tile (round-4 ISA count) -- and a lone wave then
      // sits out the LDS latency in front of each group of matrix instructions.
      {
        // (requested in PAIRS -- steps t + 2 and t + 3 at every even t -- so that two patterns travel in one ds_read2_b64:
        //  13 LDS instructions per GEMV instead of 25)
        auto fpat = [&](const int t) { return wd[80 * (t % 5) + 4 * (t / 5)]; };
        double Aq[4] = {fpat(0), fpat(1), 0.0, 0.0};
#pragma unroll
        for (int t = 0; t < 25; ++t) {
          const int n = t / 5, m = t - 5 * n;
          const double A = Aq[t & 3];
          if ((t & 1) == 0) {
            if (t + 2 < 25) Aq[(t + 2) & 3] = fpat(t + 2);
            if (t + 3 < 25) Aq[(t + 3) & 3] = fpat(t + 3);
          }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int c = 0; c < 4; ++c) acc[c][n] = mfma444(A, in[c][m], acc[c][n]);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      STAMP2(d == 4, 29);
#pragma unroll
      for (int n = 0; n < 5; ++n) {
        const double a = tanh_d(acc[0][n]);
        channels_pde_d<PDE>(a, acc[1][n], acc[2][n], acc[3][n], kap, in[0][n], in[1][n], in[2][n], in[3][n]);
        if (d < H - 1) {       // a is a VALU result; z_x, z_t, z_xx are raw matrix results (see agd_put_after)
          stash[d][n][0] = agd_put(a); stash[d][n][1] = agd_put_after(acc[1][n], in[1][n]);
          stash[d][n][2] = agd_put_after(acc[2][n], in[2][n]); stash[d][n][3] = agd_put_after(acc[3][n], in[3][n]);
        } else {
          top[n][0] = a; top[n][1] = acc[1][n]; top[n][2] = acc[2][n]; top[n][3] = acc[3][n];
        }
      }
      STAMP(1 + d);
    }
    // linear output layer: the pattern does not depend on the row, so all four slot lanes of a point get
    // o = (u, u_x, u_t, u_xx)
    double o[4] = {wl[nd.off_b[H]], 0.0, 0.0, 0.0};
#pragma unroll
    for (int m = 0; m < 5; ++m) {
      const double A = wl[nd.off_w[H] + 4 * m + s];
#pragma unroll
      for (int c = 0; c < 4; ++c) o[c] = mfma444(A, in[c][m], o[c]);
    }

    // ------------------------------------------------------------------ seeds + loss parts
    double sb[4] = {0.0, 0.0, 0.0, 0.0};
    if constexpr (PDE == PDE_ADR && SAW) {
      // PDE_ADR's seeds with inv_n * lambda^2 where inv_n stands (a product of its own, never contracted into a neighbour:
      // lambda = 1 gives the plain kernel's bits); a pair's two lanes hold the pair's one lambda
      const double pu = dpp_mov<DPP_QUAD_XOR1>(o[0]), pp = dpp_mov<DPP_QUAD_XOR1>(o[1]);
      const double* kp = adr_park;
      asm volatile("" : "+v"(kp));
      const AdrCoef<double> kc{kp[0], kp[1], kp[2], kp[3], kp[4], kp[5]};
      const int cls = point_class_adr(sd, pt);
      double wf, wu, wb, r2 = 0.0;
      {
#pragma clang fp contract(off)
        const double l2 = sa_lam * sa_lam;
        wf = inv_nf * l2; wu = inv_nu * l2; wb = kp[6] * l2;
      }
      if (cls == CLS_COL) {
        const double u = o[0], adv = kc.a0 + kc.a1 * u;
        const double f = o[2] + adv * o[1] - kc.nu * o[3] + u * (kc.r1 + u * (kc.r2 + kc.r3 * u));
        const double fbar = 2.0 * f * wf;
        if (s == 0) lacc[0] += f * f * wf;
        sb[0] = fbar * (kc.a1 * o[1] + kc.r1 + u * (2.0 * kc.r2 + 3.0 * kc.r3 * u));
        sb[1] = fbar * adv; sb[2] = fbar; sb[3] = -kc.nu * fbar;
        r2 = f * f * inv_nf;
      } else if (cls == CLS_DATA) {
        const double dd = o[0] - tgt[pt];
        if (s == 0) lacc[64] += dd * dd * wu;
        sb[0] = 2.0 * dd * wu;
        r2 = dd * dd * inv_nu;
      } else if (cls != CLS_PAD) {
        const double du = o[0] - pu, dp = o[1] - pp;
        if (s == 0 && cls == CLS_BLO) lacc[128] += (du * du + dp * dp) * wb;
        sb[0] = 2.0 * du * wb; sb[1] = 2.0 * dp * wb;
        r2 = (du * du + dp * dp) * kp[6];
      }
      // one Adam ascent step on lambda from this evaluation (TF form, as k_reduce_adam steps theta): the slot-0 lane of a
      // data or collocation point and of a pair's lo point.  The header holds the rate at 3 + class, 0.0 for hi points and
      // padding, so a class with rate 0 is never written
      if (sa_alpha != 0.0) {
        const double step = sa_alpha * kp[8 + 3 + cls];
        if (step != 0.0 && s == 0) {
          const double g = 2.0 * sa_lam * r2;
          const double mi = sa_m + (1.0 - kp[8]) * (g - sa_m);
          const double vi = sa_v + (1.0 - kp[9]) * (g * g - sa_v);
          sa_row[0] = sa_lam + step * mi / (sqrt(vi) + kp[10]);
          sa_row[1] = mi;
          sa_row[2] = vi;
        }
      }
    } else if constexpr (pde_adr_seed_block(PDE)) {
      // (the weighted block above is this block's twin, seed for seed: a change to the seeds here belongs there too)
      // partner of a boundary pair: pt ^ 1 is lane ^ 1 (pt = tile * 64 + wave * 16 + q), same slot.  The moves are
      // unconditional (no divergent branch around a cross-lane move); their results count in the boundary class only.
      const double pu = dpp_mov<DPP_QUAD_XOR1>(o[0]), pp = dpp_mov<DPP_QUAD_XOR1>(o[1]);
      AdrCoef<double> kc;
      double inv_nb;
      int rb_j = -1, rb_n = 0;               // PDE_ADR_ROBIN, _SRC, _VAR: this point's place in the Robin block, the block's length
      double inv_nw = 0.0;
      double adr2_b = 1.0;                   // PDE_ADR2: the coefficient of u_t
      if constexpr (ONE_TILE) {
        if constexpr (PDE == PDE_ADR2) adr2_b = nu.b;
        if constexpr (pde_adr_robin(PDE)) { kc = nu.k; rb_j = pt - nu.first; rb_n = nu.n; inv_nw = nu.inv_nw; }
        else if constexpr (PDE == PDE_ADR_ENS) kc = ens_k;
        else kc = nu;
        inv_nb = sd.inv_nb;
      } else {
        const double* kp = adr_park;
        asm volatile("" : "+v"(kp));
        kc = AdrCoef<double>{kp[0], kp[1], kp[2], kp[3], kp[4], kp[5]};
        inv_nb = kp[6];
        if constexpr (pde_adr_robin(PDE)) { rb_j = pt - (int)kp[7]; rb_n = (int)kp[8]; inv_nw = kp[9]; }
        if constexpr (PDE == PDE_ADR2) adr2_b = kp[10];
      }
      (void)rb_j; (void)rb_n; (void)inv_nw; (void)adr2_b;
      const int cls = point_class_adr(sd, pt);
      if (cls == CLS_COL) {
        if constexpr (PDE == PDE_ADR_VAR) {
          // the point's own six coefficients: row pt - 2 n_b - n_u of the table, three 16-byte loads issued here (the one-tile
          // adr variants have no vector registers to hold six doubles across the forward sweep).  Inside this branch only:
          // the table has n_f rows, no other lane may touch it.  The constants read above are dead in this variant.
          typedef double d2 __attribute__((ext_vector_type(2)));
          const d2* const kr = reinterpret_cast<const d2*>(kf_tab + 6 * (size_t)(pt - 2 * sd.n_b - sd.n_u));
          const d2 k01 = kr[0], k23 = kr[1], k45 = kr[2];
          kc = AdrCoef<double>{k01.x, k01.y, k23.x, k23.y, k45.x, k45.y};
        }
        const double u = o[0], adv = kc.a0 + kc.a1 * u;
        double ut = o[2];
        if constexpr (PDE == PDE_ADR2) {     // b u_t, a product of its own: b = 1 gives u_t
#pragma clang fp contract(off)
          ut = adr2_b * o[2];
        }
        double f = ut + adv * o[1] - kc.nu * o[3] + u * (kc.r1 + u * (kc.r2 + kc.r3 * u));
        if constexpr (pde_adr_src(PDE)) {
          // minus the source s_i = tgt[pt], loaded here (the one-tile adr variants have no vector registers to hold it across
          // the forward sweep) and subtracted as an operation of its own: a zero source gives PDE_ADR's bits
#pragma clang fp contract(off)
          f = f - tgt[pt];
        }
        const double fbar = 2.0 * f * inv_nf;
        if (s == 0) lacc[0] += f * f * inv_nf;
        sb[0] = fbar * (kc.a1 * o[1] + kc.r1 + u * (2.0 * kc.r2 + 3.0 * kc.r3 * u));
        sb[1] = fbar * adv; sb[2] = fbar; sb[3] = -kc.nu * fbar;
        if constexpr (PDE == PDE_ADR2) sb[2] = fbar * adr2_b;
      } else if (cls == CLS_DATA) {
        const double dd = o[0] - tgt[pt];
        if (s == 0) lacc[64] += dd * dd * inv_nu;
        sb[0] = 2.0 * dd * inv_nu;
      } else if (cls != CLS_PAD) {       // own minus partner: +2 (lo - hi) / n_b at lo, -2 (lo - hi) / n_b at hi
        const double du = o[0] - pu, dp = o[1] - pp;
        if (s == 0 && cls == CLS_BLO) lacc[128] += (du * du + dp * dp) * inv_nb;
        sb[0] = 2.0 * du * inv_nb; sb[1] = 2.0 * dp * inv_nb;
      } else if constexpr (pde_adr_robin(PDE)) {
        // the Robin block stands behind the collocation block (CLS_PAD by sd's counts): r = alpha u + beta u_x - g
        if ((unsigned)rb_j < (unsigned)rb_n) {
          typedef double d2 __attribute__((ext_vector_type(2)));
          if constexpr (PDE == PDE_ADR2) {   // rows (alpha, beta, gamma, 0): two 16-byte loads; + gamma u_t by an fma (gamma = 0: an exact zero)
            const d2* const row = reinterpret_cast<const d2*>(rb_ab + 4 * rb_j);
            const d2 ab = row[0], gz = row[1];
            const double r = __builtin_fma(gz.x, o[2], ab.x * o[0] + ab.y * o[1]) - tgt[pt];
            if (s == 0) lacc[128] += r * r * inv_nw;
            sb[0] = 2.0 * r * ab.x * inv_nw; sb[1] = 2.0 * r * ab.y * inv_nw; sb[2] = 2.0 * r * gz.x * inv_nw;
          } else {
            const d2 ab = *reinterpret_cast<const d2*>(rb_ab + 2 * rb_j);
            const double r = ab.x * o[0] + ab.y * o[1] - tgt[pt];
            if (s == 0) lacc[128] += r * r * inv_nw;
            sb[0] = 2.0 * r * ab.x * inv_nw; sb[1] = 2.0 * r * ab.y * inv_nw;
          }
        }
      }
    } else if constexpr (PDE == PDE_ADR_IDE) {
      // PDE_ADR's seeds with the parked coefficients; slot lanes 1-3 of a collocation point add its six coefficient
      // derivatives where only the slot-0 lane adds a loss part (selects, no branch on the slot)
      const double pu = dpp_mov<DPP_QUAD_XOR1>(o[0]), pp = dpp_mov<DPP_QUAD_XOR1>(o[1]);
      const double* kp = adr_park;
      asm volatile("" : "+v"(kp));
      const AdrCoef<double> kc{kp[0], kp[1], kp[2], kp[3], kp[4], kp[5]};
      const double inv_nb = kp[6];
      const int cls = point_class_adr(sd, pt);
      if (cls == CLS_COL) {
        const double u = o[0], adv = kc.a0 + kc.a1 * u;
        const double f = o[2] + adv * o[1] - kc.nu * o[3] + u * (kc.r1 + u * (kc.r2 + kc.r3 * u));
        const double fbar = 2.0 * f * inv_nf;
        const double fu = fbar * u;
        // (picked by bit masks of the slot, not by compares: three more condition masks in scalar registers made the
        //  tile-loop variants spill)
        const int m0 = ((s ^ 0) - 1) >> 31, m1 = ((s ^ 1) - 1) >> 31, m2 = ((s ^ 2) - 1) >> 31;      // -1 where s == k
        lacc[0] += bit_pick(m0, f * f * inv_nf, bit_pick(m1, fbar * o[1], bit_pick(m2, fu * o[1], -(fbar * kc.nu) * o[3])));
        lacc[64] += bit_pick(m0, 0.0, bit_pick(m1, fu, bit_pick(m2, fu * u, fu * u * u)));
        sb[0] = fbar * (kc.a1 * o[1] + kc.r1 + u * (2.0 * kc.r2 + 3.0 * kc.r3 * u));
        sb[1] = fbar * adv; sb[2] = fbar; sb[3] = -kc.nu * fbar;
      } else if (cls == CLS_DATA) {
        const double dd = o[0] - tgt[pt];
        if (s == 0) lacc[64] += dd * dd * inv_nu;
        sb[0] = 2.0 * dd * inv_nu;
      } else if (cls != CLS_PAD) {
        const double du = o[0] - pu, dp = o[1] - pp;
        if (s == 0 && cls == CLS_BLO) lacc[128] += (du * du + dp * dp) * inv_nb;
        sb[0] = 2.0 * du * inv_nb; sb[1] = 2.0 * dp * inv_nb;
      }
    } else {
      // (SAW: pde 0 has no boundary pairs; classing without n_b saves the tile-loop variants a scalar register)
      const int cls = SAW ? (pt < sd.n_u ? CLS_DATA : pt < sd.n_all ? CLS_COL : CLS_PAD) : point_class(sd, pt);
      const bool res = (PDE == 0) ? (cls == CLS_COL) : (cls == CLS_DATA);
      // SAW: inv_n * lambda^2 as a product of its own (never contracted into a neighbour), so lambda = 1 gives inv_n itself
      // and every bit downstream is the plain kernel's
      double wf = inv_nf, wu = inv_nu, r2 = 0.0;
      if constexpr (SAW) {
#pragma clang fp contract(off)
        const double l2 = sa_lam * sa_lam;
        wf = inv_nf * l2; wu = inv_nu * l2;
      }
      if (res) {
        const double wgt = (PDE == 0) ? wf : inv_nu;
        const double f = o[2] + c1 * o[0] * o[1] - c2 * o[3];
        const double fbar = 2.0 * f * wgt;
        if (s == 0) {
          lacc[0] += f * f * wgt;
          if (PDE == 1) { lacc[128] += fbar * o[0] * o[1]; lacc[192] -= fbar * c2 * o[3]; }
        }
        sb[0] = fbar * c1 * o[1]; sb[1] = fbar * c1 * o[0]; sb[2] = fbar; sb[3] = -c2 * fbar;
        if constexpr (SAW) r2 = f * f;
      }
      if (cls == CLS_DATA) {
        const double dd = o[0] - tgt[pt];
        if (s == 0) lacc[64] += dd * dd * wu;
        sb[0] += 2.0 * dd * wu;
        if constexpr (SAW) r2 = dd * dd;
      }
      if constexpr (SAW) {
        // one Adam ascent step on lambda from this evaluation (TF form, as k_reduce_adam steps theta), slot-0 lane only
        if (sa_alpha != 0.0 && s == 0 && pt < sd.n_all) {
          const double* const k = sa_lam_p;                        // beta1, beta2, eps
          const double g = 2.0 * sa_lam * r2 * (cls == CLS_DATA ? inv_nu : inv_nf);
          const double mi = sa_m + (1.0 - k[0]) * (g - sa_m);
          const double vi = sa_v + (1.0 - k[1]) * (g * g - sa_v);
          sa_row[0] = sa_lam + sa_alpha * mi / (sqrt(vi) + k[2]);
          sa_row[1] = mi;
          sa_row[2] = vi;
        }
      }
    }

    // ------------------------------------------------------------------ reverse sweep (kernels_fused20d_reverse.h)
#if PINN_F20D_SPLIT
    if (helper) {
#define PINN_F20D_ROLE 2
#include "kernels_fused20d_reverse.h"
#undef PINN_F20D_ROLE
    } else {
#define PINN_F20D_ROLE 1
#include "kernels_fused20d_reverse.h"
#undef PINN_F20D_ROLE
    }
    if (helper && !(tile & 1)) continue;               // a helper's second tile (the loop's own test ends it where there is none)
#else
#define PINN_F20D_ROLE 0
#include "kernels_fused20d_reverse.h"
#undef PINN_F20D_ROLE
#endif
    if (ONE_TILE) break;
  }
  STAMP(2 * H + 1);
#if PINN_F20D_SPLIT
  if (helper) return;                                  // a helper writes no loss parts (the whole workgroup leaves: no barrier is split)
#endif
#undef PINN_LANE_INDICES
#undef PINN_TO_POINTS
#undef PINN_PHASE_STAGE

  // -------------------------------------------------------------------- one gradient row per workgroup
  {
    // row_index[e]: flat parameter index of entry e of the block list (-1: padding), built once on the host;
    // fetched first so that its (cold) latency hides under the wave sums and the two barriers  (it does: prefetching
    // the table into LDS with the weights' DMA changed nothing -- Adam step 40.79 vs 40.81 us, same box)
    constexpr int NE = NBLK * 16, NIT = ONE_TILE ? 1 : (NE + 255) / 256;   // (one tile: the row was written phase by phase)
    int idx[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int e = tid + 256 * it;
      idx[it] = (!ONE_TILE && e < NE) ? row_index[e] : -1;
    }
    // PDE_ADR_IDE: quarters 0 and 1 hold four sums each, one per DPP row (= slot): [loss_f, a0, a1, log nu], [data, r1, r2, r3]
    const double t0 = PDE == PDE_ADR_IDE ? row16_sum(lacc[0]) : wave_sum(lacc[0]);
    const double t1 = PDE == PDE_ADR_IDE ? row16_sum(lacc[64]) : wave_sum(lacc[64]);
    const double t2 = (PDE == 1 || pde_is_adr(PDE) || PDE == PDE_ADR2) ? wave_sum(lacc[128]) : 0.0, t3 = PDE == 1 ? wave_sum(lacc[192]) : 0.0;
    double ide_mask = 0.0;
    if constexpr (PDE == PDE_ADR_IDE) ide_mask = lacc_all[wave * 256 + 192 + 7];      // this wave's own parked copy
    __syncthreads();                                   // every wave's accumulators are final
    double* const scal = wl;                           // the weight copy is dead: 4 x 4 loss / lambda partials (PDE_ADR_IDE: 4 x 9)
    if constexpr (PDE == PDE_ADR_IDE) {                // per wave: loss_f, data, pairs, then the six coefficient sums
      const int sl = lane >> 4;
      if ((lane & 15) == 0) {
        if (sl == 0) { scal[wave * 9 + 0] = t0; scal[wave * 9 + 1] = t1; scal[wave * 9 + 2] = t2; }
        else { scal[wave * 9 + 2 + sl] = t0; scal[wave * 9 + 5 + sl] = t1; }
      }
    } else
    if (lane == 0) { scal[wave * 4 + 0] = t0; scal[wave * 4 + 1] = t1; scal[wave * 4 + 2] = t2; scal[wave * 4 + 3] = t3; }
    __syncthreads();
    double* __restrict__ row = part + (size_t)blockIdx.x * R;
    if (!ONE_TILE) {
      double v[NIT];
#pragma unroll
      for (int it = 0; it < NIT; ++it) {
        const int e = tid + 256 * it;
        const int ee = e < NE ? e : 0;
        v[it] = ((gacc_all[ee] + gacc_all[NE + ee]) + gacc_all[2 * NE + ee]) + gacc_all[3 * NE + ee];
      }
#pragma unroll
      for (int it = 0; it < NIT; ++it)
        if (idx[it] >= 0) row[idx[it]] = v[it];
    } else if (blockIdx.x >= n_tiles) {                // (cannot happen: the launch plan gives every workgroup a tile)
      for (int i = tid; i < nd.n_theta; i += 256) row[i] = 0.0;
    }
    if constexpr (PDE == PDE_ADR_IDE) {
      if (tid < 9) {
        const double v = ((scal[tid] + scal[9 + tid]) + scal[18 + tid]) + scal[27 + tid];
        if (tid < 3) row[nd.n_theta + tid] = v;
        else row[nd.n_theta - 9 + tid] = (((int)ide_mask >> (tid - 3)) & 1) ? v : 0.0;     // a frozen coefficient: exactly 0.0
      }
    } else
    if (tid < 4) {
      const double v = ((scal[tid] + scal[4 + tid]) + scal[8 + tid]) + scal[12 + tid];
      if (tid == 0) { row[nd.n_theta + 0] = v; if (!pde_adr_seed_block(PDE)) row[nd.n_theta + 2] = 0.0; }
      if (tid == 1) row[nd.n_theta + 1] = v;
      if (pde_adr_seed_block(PDE) && tid == 2) row[nd.n_theta + 2] = v;     // the periodic pairs' part (+ the Robin part)
      if (PDE == 1 && tid == 2) row[nd.n_net] = v;
      if (PDE == 1 && tid == 3) row[nd.n_net + 1] = v;
    }
  }
  STAMP(2 * H + 2);
}
