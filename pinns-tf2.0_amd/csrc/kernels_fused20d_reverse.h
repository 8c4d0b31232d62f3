// kernels_fused20d_reverse.h -- the reverse sweep of kernels_fused20d_kernel.h's tile loop, included there once per ROLE
// (PINN_F20D_ROLE): 0 = the whole sweep (every kernel but k_split20d), 1 = the main workgroup of a split launch, 2 = its
// helper.  One text, so the roles' arithmetic is the plain sweep's, expression for expression; a role leaves out the
// gradient blocks, operand moves, parking stores and phase sums of the columns it does not own (PINN_ROLE_OWNS, from
// f20d_split_owner of fused20d_api.h), and the helper leaves out the reverse GEMV, which only the layers below need.  With
// ROLE 0 every role condition is the constant true: the text the compiler sees is the one it saw before the split.
// No include guard: it is meant to be included more than once.
#define PINN_ROLE_OWNS(COL)                                                                                           \
  (PINN_F20D_ROLE == 0 || f20d_split_owner((COL), H, pde_n_tail(PDE)) == (PINN_F20D_ROLE == 2 ? F20D_HELPER : F20D_MAIN))
    // ------------------------------------------------------------------ reverse sweep
    double ob[4][5];                         // adjoint of the outputs of the layer below, own (slot, point)
    if (PINN_F20D_ROLE == 2) {               // the helper's second tile: coordinates requested here, one top phase ahead
      const int nt = tile + 1;
      if (!(tile & 1) && nt < n_tiles) { x = xs[nt * 64 + wave * 16 + q]; t = ts[nt * 64 + wave * 16 + q]; }
    }
    {  // dense H (linear, one output): z_bar = sb.  dW_H[k] = sum IN_c[k] sb_c, db_H = sum sb_h
      if (PINN_ROLE_OWNS(nd_const.off_w[H])) {
      double sbT[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) sbT[c] = PINN_TO_POINTS(s == 0 ? sb[c] : 0.0);     // column 0 only
      {
        double D[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, old[6];
#pragma unroll
        for (int m = 0; m < 6; ++m) old[m] = grad_fetch(BLK_H + m);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
#pragma unroll
          for (int m = 0; m < 5; ++m) D[m] = mfma444(PINN_TO_POINTS(in[c][m]), sbT[c], D[m]);
        }
        D[5] = mfma444(onesA, sbT[0], 0.0);
        phase_first = BLK_H;                                   // phase 0 of the reverse sweep: buffer 0
        stage_w = gacc_all + PINN_PHASE_STAGE(0) + wave * STAGE_WAVE_STRIDE;
#pragma unroll
        for (int m = 0; m < 6; ++m) grad_store(D[m], old[m], BLK_H + m);
        gacc_flush();
      }
      }
#pragma unroll
      for (int n = 0; n < 5; ++n) {
        const double w = wl[nd.off_w[H] + 4 * n + s];
#pragma unroll
        for (int c = 0; c < 4; ++c) ob[c][n] = sb[c] * w;
      }
    }
    STAMP(H + 1);
#pragma unroll
    for (int d = H - 1; d >= (PINN_F20D_ROLE == 2 ? H - 1 : 1); --d) {
      // (split launch: the phase in front of this layer is summed by the role that parked it; this layer's gradient blocks,
      //  with their operand moves, belong to the role that owns its columns)
      const bool prev_here = PINN_ROLE_OWNS(nd_const.off_w[d + 1]), dw_here = PINN_ROLE_OWNS(nd_const.off_w[d]);
      // pre-activation adjoints of layer d; their point-major (moved) copies for the weight gradient are made inside the GEMV.
      // One tile: the barrier and the 16 reads of the previous phase's sum stand in front of the adjoint arithmetic (pure
      // VALU), which hides their LDS round trip.
      double zb[4][5], zbT[4][5];
      if constexpr (ONE_TILE) { if (prev_here) phase_issue(d == H - 1 ? 6 * 16 : 30 * 16, H - d - 1); }
#pragma unroll
      for (int n = 0; n < 5; ++n) {
        double a, zp, zq, zr;
        if (d == H - 1) { a = top[n][0]; zp = top[n][1]; zq = top[n][2]; zr = top[n][3]; }
        else { a = agd_get(stash[d][n][0]); zp = agd_get(stash[d][n][1]); zq = agd_get(stash[d][n][2]); zr = agd_get(stash[d][n][3]); }
        preact_adjoint_pde_d<PDE>(a, zp, zq, zr, kap, ob[0][n], ob[1][n], ob[2][n], ob[3][n], zb[0][n], zb[1][n], zb[2][n], zb[3][n]);
      }
      STAMP2(d == 4, 20);
      // One tile: the phase before this one is summed HERE, not where its last block was parked -- the stash entries of
      // layer d, read a first time for that phase's rotated inputs, are still in registers for the adjoints above (a
      // barrier in between would end their basic block and cost a second v_accvgpr_read each).
      // The LDS pipe is the second bottleneck of this kernel (a ds_read_b128 costs a wave ~53 cycles of it with four waves on
      // the CU: profiles/r01_ubench_lds_rates.txt, r06_stamps2_new.txt), and it runs beside the matrix pipe: the adds and
      // stores of the sum stand in front of the reverse GEMV, and this layer's 40 operand moves -- needed only by the
      // weight-gradient blocks behind the GEMV -- are issued one per pinned GEMV step.
      // (finish_prev stays a lambda: written out in place, the one-tile instantiations come out 14-19 instructions longer)
      auto finish_prev = [&]() {
        if (d == H - 1) phase_finish(6 * 16, idx_dense_h);
        else phase_finish(30 * 16, [&](int, const int k) { return rel_hidden[k] < 0 ? -1 : nd.off_w[d + 1] + rel_hidden[k]; });
      };
      if constexpr (ONE_TILE) { if (prev_here) finish_prev(); }
      STAMP2(d == 4, 21);
      // the first in-group's inputs of the weight-gradient blocks: formed here, moved in the last steps of the GEMV
      double cur[4] = {0.0, 0.0, 0.0, 0.0}, first_nat[4] = {0.0, 0.0, 0.0, 0.0};
      if (dw_here) {
        double a_, zp_, zq_, zr_;
        if (d - 1 == 0) {
          a_ = a0[0]; zp_ = sx * wl[nd.off_w[0] + s]; zq_ = st * wl[nd.off_w[0] + FW + s]; zr_ = 0.0;
        } else {
          a_ = agd_get(stash[d - 1][0][0]); zp_ = agd_get(stash[d - 1][0][1]);
          zq_ = agd_get(stash[d - 1][0][2]); zr_ = agd_get(stash[d - 1][0][3]);
        }
        channels_pde_d<PDE>(a_, zp_, zq_, zr_, kap, first_nat[0], first_nat[1], first_nat[2], first_nat[3]);
      }
      // adjoint of the layer-(d-1) outputs: in_bar[4m + i] = sum_j z_bar_j W_d[4m + i][j]
      const double* __restrict__ wd = wl + nd.off_w[d] + pr;
#pragma unroll
      for (int m = 0; m < 5; ++m) {
        ob[0][m] = ob[1][m] = ob[2][m] = ob[3][m] = 0.0;
      }
      {
        auto rpat = [&](const int t) { return wd[80 * (t / 5) + 4 * (t % 5)]; };
        double Aq[4] = {rpat(0), rpat(1), 0.0, 0.0};
#pragma unroll
        for (int t = 0; t < 25; ++t) {
          const int m = t / 5, n = t - 5 * m;
          const double A = Aq[t & 3];
          if ((t & 1) == 0) {
            if (t + 2 < 25) Aq[(t + 2) & 3] = rpat(t + 2);
            if (t + 3 < 25) Aq[(t + 3) & 3] = rpat(t + 3);
          }
          if (t < 20 && dw_here) zbT[t / 5][t % 5] = PINN_TO_POINTS(zb[t / 5][t % 5]);   // one operand move per step
          if (t >= 20 && t < 24 && dw_here) cur[t - 20] = PINN_TO_POINTS(first_nat[t - 20]);
          __builtin_amdgcn_sched_barrier(0);
          if (PINN_F20D_ROLE != 2) {             // (the helper stops at this layer: nothing below reads its ob)
#pragma unroll
          for (int c = 0; c < 4; ++c) ob[c][m] = mfma444(A, zb[c][n], ob[c][m]);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      STAMP2(d == 4, 22);
      // dW_d[4m + i][4n + j]: the A operands are the layer-(d-1) output channels, rotated -- produced one in-group
      // ahead of the matrix instructions that consume them (20 values live instead of 40: the kernel sits at the
      // 256-VGPR limit, and with all of them live hipcc sank the accumulator fetches next to their uses)
      if (dw_here) {
      const int base = 5 + (d - 1) * 30;
      phase_first = base;                                      // phase H - d: buffers alternate
      stage_w = gacc_all + PINN_PHASE_STAGE(H - d) + wave * STAGE_WAVE_STRIDE;
#define PINN_ROTATED_INPUTS(M, O4)                                                                          \
  do {                                                                                                      \
    double a_, zp_, zq_, zr_;                                                                               \
    if (d - 1 == 0) {                                                                                       \
      const int f_ = 4 * (M) + s;                                                                           \
      a_ = a0[M]; zp_ = sx * wl[nd.off_w[0] + f_]; zq_ = st * wl[nd.off_w[0] + FW + f_]; zr_ = 0.0;         \
    } else {                                                                                                \
      a_ = agd_get(stash[d - 1][M][0]); zp_ = agd_get(stash[d - 1][M][1]);                                  \
      zq_ = agd_get(stash[d - 1][M][2]); zr_ = agd_get(stash[d - 1][M][3]);                                 \
    }                                                                                                       \
    double h_, p_, q_, r_;                                                                                  \
    channels_pde_d<PDE>(a_, zp_, zq_, zr_, kap, h_, p_, q_, r_);                                                      \
    O4[0] = PINN_TO_POINTS(h_); O4[1] = PINN_TO_POINTS(p_);                                             \
    O4[2] = PINN_TO_POINTS(q_); O4[3] = PINN_TO_POINTS(r_);                                             \
  } while (0)
#pragma unroll
      for (int m = 0; m < 5; ++m) {          // five independent accumulator chains per in-group
        double D[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, old[5], nxt[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int n = 0; n < 5; ++n) old[n] = grad_fetch(base + m * 5 + n);
        if (m + 1 < 5) PINN_ROTATED_INPUTS((m + 1 < 5 ? m + 1 : 4), nxt);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
#pragma unroll
          for (int n = 0; n < 5; ++n) D[n] = mfma444(cur[c], zbT[c][n], D[n]);
        }
#pragma unroll
        for (int n = 0; n < 5; ++n) grad_store(D[n], old[n], base + m * 5 + n);
        gacc_flush();
#pragma unroll
        for (int c = 0; c < 4; ++c) cur[c] = nxt[c];
        STAMP2(d == 4, 23 + m);
      }
#undef PINN_ROTATED_INPUTS
      {
        double D[5], old[5];
#pragma unroll
        for (int n = 0; n < 5; ++n) old[n] = grad_fetch(base + 25 + n);
#pragma unroll
        for (int n = 0; n < 5; ++n) D[n] = mfma444(onesA, zbT[0][n], 0.0);
#pragma unroll
        for (int n = 0; n < 5; ++n) grad_store(D[n], old[n], base + 25 + n);
        gacc_flush();
      }
      }
      STAMP(2 * H + 1 - d);
    }
    if (PINN_F20D_ROLE == 2) {               // the helper's last phase: layer H - 1's blocks, summed as the plain sweep sums them
      phase_issue(30 * 16, 1);
      phase_finish(30 * 16, [&](int, const int k) { return rel_hidden[k] < 0 ? -1 : nd.off_w[H - 1] + rel_hidden[k]; });
      STAMP((tile & 1) ? 31 : 19);
    }
    if (PINN_F20D_ROLE != 2) {  // dense 0: inputs (hx, ht, 1) in channel h, (sx, 0, 0) in channel p, (0, st, 0) in channel q
      const double hxT = PINN_TO_POINTS(hx), htT = PINN_TO_POINTS(ht);
      const double Ah = i4 == 0 ? hxT : i4 == 1 ? htT : i4 == 2 ? 1.0 : 0.0;
      const double Ap = i4 == 0 ? sx : 0.0, Aq = i4 == 1 ? st : 0.0;
      double bT[3][5];
#pragma unroll
      for (int n = 0; n < 5; ++n) {
        const int f = 4 * n + s;
        double bh, bp, bq, br;
        preact_adjoint_pde_d<PDE>(a0[n], sx * wl[nd.off_w[0] + f], st * wl[nd.off_w[0] + FW + f], 0.0, kap, ob[0][n], ob[1][n],
                         ob[2][n], ob[3][n], bh, bp, bq, br);
        bT[0][n] = PINN_TO_POINTS(bh); bT[1][n] = PINN_TO_POINTS(bp); bT[2][n] = PINN_TO_POINTS(bq);
      }
      if constexpr (ONE_TILE) {                                // layer 1's phase
        static_assert(PINN_F20D_ROLE == 2 || (PINN_ROLE_OWNS(nd_const.off_w[1]) && PINN_ROLE_OWNS(nd_const.off_w[0])), "the bottom of the sweep is the main role's");
        phase_issue(30 * 16, H - 1);
        phase_finish(30 * 16, [&](int, const int k) { return rel_hidden[k] < 0 ? -1 : nd.off_w[1] + rel_hidden[k]; });
      }
      double D[5], old[5];
#pragma unroll
      for (int n = 0; n < 5; ++n) old[n] = grad_fetch(n);
#pragma unroll
      for (int n = 0; n < 5; ++n) D[n] = mfma444(Ah, bT[0][n], 0.0);
#pragma unroll
      for (int n = 0; n < 5; ++n) D[n] = mfma444(Ap, bT[1][n], D[n]);
#pragma unroll
      for (int n = 0; n < 5; ++n) D[n] = mfma444(Aq, bT[2][n], D[n]);
      phase_first = 0;                                         // phase H
      stage_w = gacc_all + PINN_PHASE_STAGE(H) + wave * STAGE_WAVE_STRIDE;
#pragma unroll
      for (int n = 0; n < 5; ++n) grad_store(D[n], old[n], n);
      gacc_flush();
      if constexpr (ONE_TILE) {
        auto idx_dense_0 = [&](const int e, int) {
          const int f = 4 * (e >> 4) + (e & 3), i = (e >> 2) & 3;
          return i == 0 ? nd.off_w[0] + f : i == 1 ? nd.off_w[0] + FW + f : i == 2 ? nd.off_b[0] + f : -1;
        };
        phase_issue(5 * 16, H);
        phase_finish(5 * 16, idx_dense_0);
        if constexpr (PINN_ONETILE_SUM == 2) {           // every phase is parked in its own region: one barrier, H + 1 sums
          parked_barrier();
          phase_reads(6 * 16, 0);
          phase_adds(6 * 16, idx_dense_h);
#pragma unroll
          for (int d = H - 1; d >= 1; --d) {
            phase_reads(30 * 16, H - d);
            phase_adds(30 * 16, [&](int, const int k) { return rel_hidden[k] < 0 ? -1 : nd.off_w[d] + rel_hidden[k]; });
          }
          phase_reads(5 * 16, H);
          phase_adds(5 * 16, idx_dense_0);
        }
      }
    }
#undef PINN_ROLE_OWNS
