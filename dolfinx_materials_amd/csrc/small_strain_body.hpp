// The tile body of the small-strain update kernels: NOT a header of its own.  small_strain.hpp includes this text inside the braces
// of small_strain_kernel (FIELDS = false) and of small_strain_field_kernel (FIELDS = true); each defines, just before the include,
//   constexpr bool FIELDS    and    pf (ParamStreams: the kernel's argument, or an all-null constant that only discarded code names)
//   constexpr bool CLEAN     and    stamps, stamp (small_strain_clean.hip: the per-tile stamps of the handle and the value that means
//                                   "this tile's bytes are the same in both state buffers"; null constants elsewhere, as for pf)
//   constexpr int PACKED     and    pack_mask, pack_buf (small_strain_packed.hip: the packed copy of s0, one 64-bit mask per tile and the
//                                   non-zero points' slots at the tile's pitch of 7 x 64 doubles; 0 the old state comes from s0, 1 it
//                                   does and the copy is built from it, 2 it comes from the copy; 0 and null constants elsewhere)
// beside the common arguments (prm, n, eps, s0, s1, ld, sig, ct, stats, src) and template parameters (LAW, TL, GRAD).  Shared as
// text and not through a function: see the comment at the top of small_strain.hpp.
  __shared__ __attribute__((aligned(16))) double lds_all[WAVES_PER_BLOCK * SS_LDS_PER_WAVE];
  __shared__ unsigned long long red[4 * WAVES_PER_BLOCK];

  int lane = threadIdx.x & (WAVE - 1);
  // (not made scalar with readfirstlane as in fefp.hpp: measured in one process, three handles each, that build is
  // 0.45 % slower -- 96 instead of 103 VGPRs makes a fifth wave per SIMD resident, which this kernel does not like)
  const int wid = threadIdx.x >> 6;
  double* stage = lds_all + wid * SS_LDS_PER_WAVE;
  double* coef = stage + SS_STAGE;
  double2_t* stage2 = reinterpret_cast<double2_t*>(stage);

  const int64_t ntiles = (n + WAVE - 1) / WAVE;
  const int64_t tile_stride = (int64_t)gridDim.x * WAVES_PER_BLOCK;

  unsigned long long c_plastic = 0, c_notconv = 0, c_nan = 0, c_maxit = 0;

  const double lambda_u = prm.lambda, mu_u = prm.mu;

  for (int64_t tile = (int64_t)blockIdx.x * WAVES_PER_BLOCK + wid; tile < ntiles;
       tile += tile_stride) {
    const int64_t base = tile * WAVE;
    const int npts = (n - base) < WAVE ? (int)(n - base) : WAVE;
    if constexpr (FIELDS || LAW == LAW_J2_VOCE || LAW == LAW_RAMBERG_OSGOOD) {
      // the lane index is re-read through an opaque copy once per tile: per-lane invariants hoisted out of the
      // tile loop otherwise push the Voce kernels over their 128-register budget (2-8 spilled VGPRs; the fused
      // Ramberg-Osgood kernels, whose inlined exp / log are live at the same time, 2-16).  FIELDS: for both laws
      asm volatile("" : "+v"(lane));
      lane &= WAVE - 1;
    }
    const bool valid = lane < npts;
    const int64_t gi = base + lane;
    [[maybe_unused]] uint32_t tile_stamp = 0;     // CLEAN only
    [[maybe_unused]] bool any_plastic = true;     // CLEAN only: some valid lane of the tile yields, i.e. s1 gets bits that s0 does not hold

    double e[6];
    double p_n = 0.0, ep[6] = {0, 0, 0, 0, 0, 0};
    if constexpr (GRAD == 0) {
      // ---- 1. coalesced strain load (3 x 1 KiB per wave) into LDS ------------------------------
#include "tile_rows6_load.hpp"
      // ---- old state, SoA (issued before the LDS round trip completes) -------------------------
      if constexpr (ss_has_state<LAW> && PACKED == 2) {
        // PACKED use: the tile's mask says which points hold a slot that is not bit-zero (one word per wave, made scalar like the
        // stamp); those k points read their seven slots from the packed copy, slot c of the r-th of them at c k + r of the tile's
        // pitch, the others keep zeros.  A tile of never-yielded points (k = 0) issues no state load.
        const unsigned long long mv = pack_mask[tile];
        // (the builtin returns an int: through unsigned, or bit 31 of the low word would fill the high one)
        const unsigned long long msk = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((unsigned)(mv >> 32)) << 32) |
                                       (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((unsigned)mv);
        if (msk != 0ull) {
          if ((msk >> lane) & 1ull) {
            const int k = __popcll(msk);
            const double* q = pack_buf + tile * (int64_t)(7 * WAVE) +
                              __builtin_amdgcn_mbcnt_hi((unsigned)(msk >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)msk, 0u));
            p_n = stream_load<3>(q);
#pragma unroll
            for (int c = 0; c < 6; ++c) ep[c] = stream_load<3>(q + (1 + c) * k);
          }
        }
      } else if constexpr (ss_has_state<LAW>) {
        if (valid) {
          p_n = stream_load<3>(s0 + gi);
#pragma unroll
          for (int c = 0; c < 6; ++c) ep[c] = stream_load<3>(s0 + (int64_t)(1 + c) * ld + gi);
        }
      }
      // CLEAN: the tile's stamp travels with the old state (one word per wave, made scalar: the skip below is a uniform branch)
      if constexpr (CLEAN) tile_stamp = __builtin_amdgcn_readfirstlane(stamps[tile]);
      wave_lds_sync();
      // ---- 2. my point's strain ----------------------------------------------------------------
#include "tile_rows6_take.hpp"
      wave_lds_sync();  // staging region is reused for the stress below
      if constexpr (ss_has_state<LAW> && PACKED == 1) {
        // PACKED build: the copy the use form reads, made of what was just loaded (here, where the update waits for the old state
        // anyway).  A test on the bits: -0.0 and NaN are kept and come back as they are; a lane past the end holds zeros.
        unsigned long long bits = (unsigned long long)__double_as_longlong(p_n);
#pragma unroll
        for (int c = 0; c < 6; ++c) bits |= (unsigned long long)__double_as_longlong(ep[c]);
        const unsigned long long msk = __ballot(bits != 0ull);
        if (bits != 0ull) {
          const int k = __popcll(msk);
          double* q = pack_buf + tile * (int64_t)(7 * WAVE) +
                      __builtin_amdgcn_mbcnt_hi((unsigned)(msk >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)msk, 0u));
          stream_store<1>(q, p_n);
#pragma unroll
          for (int c = 0; c < 6; ++c) stream_store<1>(q + (1 + c) * k, ep[c]);
        }
        if (lane == 0) pack_mask[tile] = msk;
      }
    } else {
      double Hd[9];
      if constexpr (GRAD == 1) {
        // ---- 1'. one (cell, corner) per lane: node -> wave-private record in the coefficient region
        {
          const int64_t cell = ((src.point0 + base) >> 3) + (lane >> 3);
          double2_t r0 = {0.0, 0.0}, r1 = {0.0, 0.0}, r2 = {0.0, 0.0};
          if (cell < src.ncells) {
            const int64_t nd = src.conn[cell * 8 + (lane & 7)];
            r0 = double2_t{src.coords[3 * nd], src.coords[3 * nd + 1]};
            r1 = double2_t{src.coords[3 * nd + 2], src.u[3 * nd]};
            r2 = double2_t{src.u[3 * nd + 1], src.u[3 * nd + 2]};
          }
          double2_t* d = reinterpret_cast<double2_t*>(coef + (lane >> 3) * HEX_FUSED_REC + (lane & 7) * 6);
          d[0] = r0; d[1] = r1; d[2] = r2;
        }
        wave_lds_sync();
        // ---- 2'. displacement gradient at my Gauss point (point q = lane & 7 of cell lane >> 3) -----
        {
          const double2_t* rec = reinterpret_cast<const double2_t*>(coef + (lane >> 3) * HEX_FUSED_REC);
          auto node = [&](int m, double* X, double* U) {
            const double2_t a = rec[m * 3], b = rec[m * 3 + 1], c = rec[m * 3 + 2];
            X[0] = a.x; X[1] = a.y; X[2] = b.x;
            U[0] = b.y; U[1] = c.x; U[2] = c.y;
          };
          const int q = lane & 7;
          if (valid) {
            hex8_disp_grad(src.xi[q][0], src.xi[q][1], src.xi[q][2], node, Hd);
          } else {
#pragma unroll
            for (int k = 0; k < 9; ++k) Hd[k] = 0.0;
          }
        }
        wave_lds_sync();  // the coefficient region is rewritten in step 5
      } else {
        if (valid) {
          const int64_t cell = (src.point0 + gi) / src.nqp;
          if constexpr (GRAD == 2) tet4_cell_disp_grad(src.coords, src.conn, src.u, cell, Hd);
          else simplex_disp_grad(src, cell, (int)(src.point0 + gi - cell * src.nqp), Hd);
        } else {
#pragma unroll
          for (int k = 0; k < 9; ++k) Hd[k] = 0.0;
        }
      }
      {
        const double r = 0.70710678118654752440;
        e[0] = Hd[0]; e[1] = Hd[4]; e[2] = Hd[8];
        e[3] = r * (Hd[1] + Hd[3]); e[4] = r * (Hd[2] + Hd[6]); e[5] = r * (Hd[5] + Hd[7]);
      }
      // old state only now: 14 registers fewer live through the gradient evaluation
      if constexpr (ss_has_state<LAW>) {
        if (valid) {
          p_n = stream_load<3>(s0 + gi);
#pragma unroll
          for (int c = 0; c < 6; ++c) ep[c] = stream_load<3>(s0 + (int64_t)(1 + c) * ld + gi);
        }
      }
    }

    // ---- 3. constitutive update --------------------------------------------------------------
    double lambda = lambda_u, mu = mu_u;
    // lp, this point's parameters as the update reads them: the kernel's own (an alias, not a copy: a copy changes the uniform
    // kernels' code), or with FIELDS the copy lp_point that the bound streams overwrite (unused and without code otherwise)
    LawParams lp_point;
    const LawParams& lp = FIELDS ? lp_point : prm;
    if constexpr (FIELDS) {
      lp_point = prm;
      // bound streams: 8 B per lane at gi, like the state slots (a lane past the end keeps the uniform values)
      if (pf.p[PF_LAMBDA] && valid) lambda = stream_load<3>(pf.p[PF_LAMBDA] + gi);
      if (pf.p[PF_MU] && valid) mu = stream_load<3>(pf.p[PF_MU] + gi);
      if (pf.p[PF_SIG0] && valid) lp_point.sig0 = stream_load<3>(pf.p[PF_SIG0] + gi);
      if (pf.p[PF_H1] && valid) lp_point.h1 = stream_load<3>(pf.p[PF_H1] + gi);
      if constexpr (LAW == LAW_J2_VOCE) {
        if (pf.p[PF_H2] && valid) lp_point.h2 = stream_load<3>(pf.p[PF_H2] + gi);
        // the Newton tolerance of dxmat.hip::build_params, per point
        if (pf.p[PF_SIG0] || pf.p[PF_MU]) lp_point.tol = prm.rtol * fmax(fabs(lp.sig0), 2e-8 * mu);
      }
    }
    double c1 = lambda, c2 = 2.0 * mu, c3 = 0.0;
    double wn = 0.0;   // n = dev(sigma) wn: the direction the tangent is built with (0 for an elastic point)
    double p_new = p_n;
    if constexpr (ss_has_state<LAW>) {
      // trial elastic strain                                   mfront:52  eel += deto
#pragma unroll
      for (int c = 0; c < 6; ++c) e[c] -= ep[c];
      const double tr = e[0] + e[1] + e[2];
      const double third = tr / 3.0;
      double se[6];
      se[0] = 2.0 * mu * (e[0] - third);
      se[1] = 2.0 * mu * (e[1] - third);
      se[2] = 2.0 * mu * (e[2] - third);
      se[3] = 2.0 * mu * e[3];
      se[4] = 2.0 * mu * e[4];
      se[5] = 2.0 * mu * e[5];                                // mfront:53
      double nrm2 = 0.0;
#pragma unroll
      for (int c = 0; c < 6; ++c) nrm2 += se[c] * se[c];
      const double seq = sqrt(1.5 * nrm2);                    // mfront:54
      const double f = seq - hardening_R<LAW>(lp, p_n);       // mfront:55
      if (f > 0.0) {
        double dp;
        unsigned iters = 0;
        if constexpr (LAW == LAW_J2_LINEAR) {
          dp = f / (lp.h1 + 3.0 * mu);                        // mfront:62-63
        } else {
          // r(dp) = seq - 3 mu dp - R(p_n + dp) = 0, monotone Newton from dp = 0
          // tolerance relative to the larger of the yield stress and the trial stress the residual is made of
          dp = 0.0;
          const double tolp = fmax(lp.tol, prm.rtol * seq);
          for (int it = 0;; ++it) {
            const double r = seq - 3.0 * mu * dp - hardening_R<LAW>(lp, p_n + dp);
            if (fabs(r) <= tolp) break;
            if (it >= prm.maxit) { if (valid) ++c_notconv; break; }
            const double dr = -3.0 * mu - hardening_dR<LAW>(lp, p_n + dp);
            dp -= r / dr;
            ++iters;
          }
        }
        const double iseq = 1.0 / seq;
        double nn[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) nn[c] = 1.5 * se[c] * iseq;   // mfront:61
        const double beta = dp * iseq;
        // The return is radial: dev(sigma) = (1 - 3 mu beta) s_e, so n = 3/2 s_e / seq = dev(sigma) wn with
        // wn = 3/2 / (seq (1 - 3 mu beta)).  The TANGENT is built with n in that form (step 5), so that whoever holds
        // the stress and wn holds n, to the bit.
        {
          const double rho = 1.0 - 3.0 * mu * beta;
          wn = rho > 0.0 ? 1.5 * iseq / rho : 0.0;   // (a division: with the 5-instruction reciprocal the fused tet4 Voce variant spills 2 registers)
          // rho = R(p) / seq of the returned state: <= 0 only for a yield stress that is not positive there (a softening law
          // driven to zero, an overshooting iterate).  The direction is then undefined (wn = 0 drops the n x n term): reported
          // as a point that did not converge, never silently.  Linear hardening can get there with H < 0 only: one scalar
          // compare on the kernel's parameters keeps the per-lane test out of the H >= 0 launches (the headline); FIELDS: per
          // lane where H is a stream
          if constexpr (LAW != LAW_J2_LINEAR) { if (valid && !(rho > 0.0)) ++c_notconv; }
          else if ((FIELDS && pf.p[PF_H1]) ? lp.h1 < 0.0 : prm.h1 < 0.0) { if (valid && !(rho > 0.0)) ++c_notconv; }
        }
        const double gamma = 1.0 / (hardening_dR<LAW>(lp, p_n + dp) + 3.0 * mu);
        // Dt = lambda IxI + 2mu Id - 4mu^2 [beta (M - n^n) + gamma n^n]      mfront:66-69
        c1 = lambda + 2.0 * mu * mu * beta;
        c2 = 2.0 * mu - 6.0 * mu * mu * beta;
        c3 = 4.0 * mu * mu * (beta - gamma);
        p_new = p_n + dp;
#pragma unroll
        for (int c = 0; c < 6; ++c) {
          ep[c] += dp * nn[c];
          e[c] -= dp * nn[c];                                  // mfront:64
        }
        if (valid) {
          ++c_plastic;
          c_maxit = iters > c_maxit ? iters : c_maxit;
        }
      }
      if constexpr (CLEAN) any_plastic = __ballot(valid && f > 0.0) != 0;
    }
    // sigma = lambda tr(eel) 1 + 2 mu eel                                      mfront:76
    const double ltr = lambda * (e[0] + e[1] + e[2]);
    double s[6];
    if constexpr (LAW == LAW_RAMBERG_OSGOOD) {
      // no state: stress and tangent coefficients of the total strain
      ramberg_osgood_update(prm, mu, e, stage2 + lane * 3, s, c1, c2, c3, wn, valid, c_plastic, c_notconv, c_maxit);
    } else {
    s[0] = ltr + 2.0 * mu * e[0];
    s[1] = ltr + 2.0 * mu * e[1];
    s[2] = ltr + 2.0 * mu * e[2];
    s[3] = 2.0 * mu * e[3];
    s[4] = 2.0 * mu * e[4];
    s[5] = 2.0 * mu * e[5];
    }
    {
      // stress, p and what the tangent is made of (quadrature_map.py:322-324 asserts on flux, state and Ct): a hardening
      // slope that is not finite at the returned state leaves the stress finite and c3 not
      const double chk = s[0] + s[1] + s[2] + s[3] + s[4] + s[5] + p_new + ((c1 + c2) + (c3 + wn));
      if (valid && !(fabs(chk) <= 1.79769313486231570e308)) ++c_nan;
    }

    // ---- 4. new state, SoA -------------------------------------------------------------------
    // CLEAN: a tile without a yielding lane stores into s1 the bits it read from s0 (p_new = p_n, ep untouched); where the
    // stamp says that s1 holds them already, the seven stores are skipped.  The stamp follows what was stored: a tile that
    // yielded is no longer the same in both buffers (0 is never current), one that did not is from now on.
    if constexpr (ss_has_state<LAW>) {
      if (CLEAN ? (valid && (any_plastic || tile_stamp != stamp)) : valid) {
        stream_store<1>(s1 + gi, p_new);
#pragma unroll
        for (int c = 0; c < 6; ++c) stream_store<1>(s1 + (int64_t)(1 + c) * ld + gi, ep[c]);
      }
      if constexpr (CLEAN) {
        if (lane == 0) {
          if (any_plastic) { if (tile_stamp == stamp) stamps[tile] = 0u; }
          else if (tile_stamp != stamp) stamps[tile] = stamp;
        }
      }
    }

    // ---- 5. stage stress and tangent coefficients in LDS --------------------------------------
    stage2[lane * 3 + 0] = double2_t{s[0], s[1]};
    stage2[lane * 3 + 1] = double2_t{s[2], s[3]};
    stage2[lane * 3 + 2] = double2_t{s[4], s[5]};
    if constexpr (ss_has_coef<LAW> && TL == TL_PACK4) {
      double2_t* c4 = reinterpret_cast<double2_t*>(coef) + lane * 2;
      c4[0] = double2_t{c1, c2};
      c4[1] = double2_t{c3, wn};
    } else if constexpr (ss_has_coef<LAW>) {
#include "small_strain_stage_coef.hpp"
    }
    wave_lds_sync();

    // ---- 6. coalesced stress store (3 x 1 KiB) -----------------------------------------------
#include "tile_rows6_store.hpp"
    // ---- 7. coalesced tangent store: entry pair (i, j..j+1) of point q ---------------------------
    if constexpr (TL == TL_PACK4) {
      static_assert(ss_has_coef<LAW>, "the elastic tangent is a constant: nothing to write");
      if (npts == WAVE) {   // 64 x 4 doubles: two 1 KiB wave stores
        double2_t* gct = reinterpret_cast<double2_t*>(ct + base * 4);
        const double2_t* c4 = reinterpret_cast<const double2_t*>(coef);
        stream_store<0>(gct + lane, c4[lane]);
        stream_store<0>(gct + WAVE + lane, c4[WAVE + lane]);
      } else {
        double2_t* gct = reinterpret_cast<double2_t*>(ct + base * 4);
        const double2_t* c4 = reinterpret_cast<const double2_t*>(coef);
        if (lane < npts * 2) stream_store<0>(gct + lane, c4[lane]);
        if (WAVE + lane < npts * 2) stream_store<0>(gct + WAVE + lane, c4[WAVE + lane]);
      }
    } else if constexpr (TL == TL_COEF) {
      // the staged coefficients as they are: 64 x 9 doubles, contiguous (4.5 KiB per tile)
      static_assert(ss_has_coef<LAW>, "the elastic tangent is a constant: nothing to write");
      if (npts == WAVE) {
        double2_t* gct = reinterpret_cast<double2_t*>(ct + base * 9);
        const double2_t* c2 = reinterpret_cast<const double2_t*>(coef);
#pragma unroll
        for (int k = 0; k < 5; ++k) {
          const int idx = k * WAVE + lane;
          if (idx < 288) stream_store<0>(gct + idx, c2[idx]);
        }
      } else {
        double* gct = ct + base * 9;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
          const int idx = k * WAVE + lane;
          if (idx < npts * 9) stream_store<0>(gct + idx, coef[idx]);
        }
      }
    } else if constexpr (TL == TL_FULL) {
      // full 6x6, row-major (quadrature_map.py:83-105): 18 x 1 KiB per tile, 18 pairs per point.
      // The (q, i, j) of a lane's pair advance by a fixed pattern from one iteration to the next
      // (64 pairs = 3 points + 10 pairs), so they are carried instead of re-divided; for a full tile
      // (wave-uniform) the stores are unpredicated and the LDS reads of 3 iterations are issued
      // together, ahead of the arithmetic (groups of 3: larger groups spill at 128 VGPRs).
      double2_t* gct = reinterpret_cast<double2_t*>(ct + base * 36);
      auto entry = [&](int q, int i, int j) -> double2_t {
        double2_t v;
        if constexpr (LAW == LAW_ELASTIC) {
          v.x = ((i < 3 && j < 3) ? lambda : 0.0) + ((i == j) ? 2.0 * mu : 0.0);
          v.y = ((i < 3 && j + 1 < 3) ? lambda : 0.0) + ((i == j + 1) ? 2.0 * mu : 0.0);
        } else {
          v = tangent_pair(coef + q * 9, i, j);
        }
        return v;
      };
      if (npts == WAVE) {
#pragma unroll 1  // a fully unrolled loop gets its (loop-invariant) index arithmetic hoisted out of the
                  // tile loop: 18 x (q, i, j) live across tiles, which spills at 128 VGPRs
        for (int g = 0; g < 6; ++g) {
          double2_t v[3];
#pragma unroll
          for (int u = 0; u < 3; ++u) {
            const int k = (g * 3 + u) * WAVE + lane;
            const int q = k / 18;
            const int r = k - q * 18;
            const int i = r / 3;
            v[u] = entry(q, i, (r - i * 3) * 2);
          }
#pragma unroll
          for (int u = 0; u < 3; ++u) stream_store<0>(gct + (g * 3 + u) * WAVE + lane, v[u]);
        }
      } else {
        const int lim = npts * 18;
#pragma unroll 1
        for (int it = 0; it < 18; ++it) {
          const int k = it * WAVE + lane;
          const int q = k / 18;
          const int r = k - q * 18;
          const int i = r / 3;
          if (k < lim) stream_store<0>(gct + k, entry(q, i, (r - i * 3) * 2));
        }
      }
    } else {
      // symmetric-packed: the 21 entries (i <= j) of the upper triangle, row-major, per point
      // (the J2 tangent is symmetric).  10.5 x 1 KiB per tile.
      constexpr unsigned long long IP = 0x0ull | (1ull << 18) | (1ull << 21) | (1ull << 24) | (1ull << 27) | (1ull << 30) |
                                        (2ull << 33) | (2ull << 36) | (2ull << 39) | (2ull << 42) | (3ull << 45) |
                                        (3ull << 48) | (3ull << 51) | (4ull << 54) | (4ull << 57) | (5ull << 60);
      constexpr unsigned long long JP = (0ull << 0) | (1ull << 3) | (2ull << 6) | (3ull << 9) | (4ull << 12) | (5ull << 15) |
                                        (1ull << 18) | (2ull << 21) | (3ull << 24) | (4ull << 27) | (5ull << 30) |
                                        (2ull << 33) | (3ull << 36) | (4ull << 39) | (5ull << 42) | (3ull << 45) |
                                        (4ull << 48) | (5ull << 51) | (4ull << 54) | (5ull << 57) | (5ull << 60);
      double* gct = ct + base * 21;
      const int lim = npts * 21;
#pragma unroll 4
      for (int it = 0; it < 11; ++it) {
        const int e0 = (it * WAVE + lane) * 2;
        double v[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int e = e0 + u;
          const int q = e / 21;
          const int t = e - q * 21;
          const int i = (int)((IP >> (3 * t)) & 7ull), j = (int)((JP >> (3 * t)) & 7ull);
          double x;
          if constexpr (LAW == LAW_ELASTIC) {
            x = ((i < 3 && j < 3) ? lambda : 0.0) + ((i == j) ? 2.0 * mu : 0.0);
          } else {
            const double* cf = coef + (q < WAVE ? q : 0) * 9;
            x = (((i < 3 && j < 3) ? cf[0] : 0.0) + ((i == j) ? cf[1] : 0.0)) + cf[2] * (cf[3 + i] * cf[3 + j]);
          }
          v[u] = x;
        }
        if (e0 + 1 < lim) stream_store<0>(reinterpret_cast<double2_t*>(gct + e0), double2_t{v[0], v[1]});
        else if (e0 < lim) stream_store<0>(gct + e0, v[0]);
      }
    }
    wave_lds_sync();  // LDS regions are rewritten by the next tile
  }

  store_block_stats(stats, c_plastic, c_notconv, c_nan, c_maxit, red);
