// Hosford plasticity with linear isotropic hardening under the plane-strain hypothesis (gradient: strain (4), flux: stress (4), both
// [xx, yy, zz, sqrt(2) xy]; the 4x4 tangent) for gfx950.
//
// By definition the law is DXM_LAW_HOSFORD_LINEAR (hosford.hip, whose header comment states the law, the local Newton and the
// consistent tangent) on the embedded strain [xx, yy, zz, sqrt(2) xy, 0, 0], restricted to the four components such a state has; the
// out-of-plane shears of strain, plastic strain, stress and tangent are zero and stay zero.  eps_zz is read like the other components
// (a plane-strain caller passes 0), sig_zz is returned.  What the restriction saves:
//   * the deviatoric trial stress is a 2x2 block (t_xx, t_yy, t_xy) and the principal value t_zz with the eigenvector e_z: ONE
//     closed-form Jacobi rotation diagonalises it, n_0 = (c, s, 0), n_1 = (-s, c, 0),
//         tau = s / c = -2 t_xy / (d + sgn(d) sqrt(d^2 + 4 t_xy^2)),  d = t_yy - t_xx  (the smaller root; sgn(0) = +1),
//     and tau = 0 where d = t_xy = 0.  Zero shear gives (c, s) = (1, 0); t_xx == t_yy with shear gives 45 degrees; the all-zero strain
//     never gets here (the elastic shortcut), and would give (1, 0);
//   * the local Newton on the three principal deviatoric stresses and dp is law 10's, unchanged;
//   * Ct = sum_ij P_ij E_i E_j^T + th_01 M_01 M_01^T with
//         E_0 = [c^2, s^2, 0, sqrt(2) c s],  E_1 = [s^2, c^2, 0, -sqrt(2) c s],  E_2 = [0, 0, 1, 0],
//         M_01 = [-sqrt(2) c s, sqrt(2) c s, 0, c^2 - s^2]:
//     the shear moduli th_02, th_12 multiply the out-of-plane shear directions and drop out, so one divided difference (over the
//     differences x3, x2 that pair (0, 1) leaves) remains of three.
// hfp_pow_am2 / hfp_divided_difference are copies of hosford.hip's (that unit is not touched: its assembly is pinned).
//
// Resources: 166 VGPRs, 3 waves per SIMD, no scratch, with no occupancy argument (an argument of 4 spills 109 VGPRs: the register peak
// is inside the local Newton).  What keeps it at 166: the wave-uniform tile base of the state streams (no 64-bit index per lane), 32-bit
// counters, per-lane invariants re-derived per tile, and the point's record parking what the Newton does not read.
//
// Mapping and memory as plane_strain.hip: one thread per point, one wave per tile of 64 points, 256-thread workgroups, grid-stride
// over the tiles, wave-private LDS ordered by wave_lds_sync() (no workgroup barrier in the tile loop), one BlockStats record per
// workgroup.
//   strain in / stress out: a tile's rows of 4 are 2048 contiguous bytes, two passes of 64 lanes x 16 B, redistributed through LDS;
//   state: 8 B-per-lane SoA streams, five in (p, the plastic strain), nine out;
//   tangent: never held per thread.  Each point stages the 10 upper-triangle entries of its block in LDS and the wave writes the 16
//     entries per point in output order: 8 passes of 16 B per lane, non-temporal; one point is one whole 128 B line written by 8
//     lanes.  In pass k lane l writes the pair (row (l & 7) >> 1, columns 2 (l & 1) and + 1) of point 8 k + (l >> 3); (i, j) and
//     (j, i) read the same staged number, so the block is exactly symmetric;
//   a ragged last tile is bounded by lane: rows of 4 doubles are whole pairs, a pair is read or written or not, and nothing is read or
//     written past the launch's points.
#include "hosford_plane.hpp"

#include "hosford.hpp"   // the slots of LawParams law 10's build function fills (HF_AM2, HF_INVA, HF_AM1)
#include "principal_axes.hpp"

namespace dxm {

// |x|^(a-2) of a ratio 0 <= ax <= 1 with lx = log(ax)   (hosford.hip::hf_pow_am2)
__device__ __forceinline__ double hfp_pow_am2(double ax, double lx, double am2) {
  return ax > 0.0 ? exp(am2 * lx) : (am2 == 0.0 ? 1.0 : 0.0);
}

// (sgn(x) |x|^m - sgn(y) |y|^m) / (x - y), m = a - 1, from the signed ratios, their logarithms and u = |.|^(m-1)
// (hosford.hip::hf_divided_difference and its header comment)
__device__ __forceinline__ double hfp_divided_difference(double m, double xs, double ys, double lx, double ly, double ux, double uy) {
  const double ax = fabs(xs), ay = fabs(ys);
  const double px = ux * ax, py = uy * ay;
  const bool same = xs * ys > 0.0;
  const double h = 0.5 * (lx - ly), y = m * h;
  const double series = m * sqrt(ux * uy) * sinhc_series(y * y) * fast_rcp(sinhc_series(h * h));
  const double quotient = same ? (px - py) / (ax - ay) : (px + py) / (ax + ay);
  return (same && fmax(fabs(y), fabs(h)) <= 0.1) ? series : quotient;
}

__global__ void __launch_bounds__(BLOCK)
hosford_plane_kernel(const LawParams prm, const int64_t n, const double* __restrict__ eps, const double* __restrict__ s0,
                     double* __restrict__ s1, const int64_t ld, double* __restrict__ sig, double* __restrict__ ct,
                     BlockStats* __restrict__ stats) {
  __shared__ __attribute__((aligned(16))) double lds_all[WAVES_PER_BLOCK * HFP_LDS_PER_WAVE];
  __shared__ unsigned long long red[4 * WAVES_PER_BLOCK];
  static_assert(HFP_LDS_BYTES == sizeof(lds_all) + sizeof(red), "hosford_plane.hpp states the LDS of the kernel");
  static_assert(WAVE * HFP_DIM == 2 * 2 * WAVE && WAVE * HFP_CT == 8 * 2 * WAVE && (HFP_LDS_PER_WAVE * 8) % 16 == 0,
                "a tile's rows are two, its tangent eight whole passes of 16 B per lane");

  int lane = threadIdx.x & (WAVE - 1);
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform: tile bookkeeping and LDS bases in scalar registers
  double* stage = lds_all + wid * HFP_LDS_PER_WAVE;           // 64 x 4: strain in, stress out
  double2_t* stage2 = reinterpret_cast<double2_t*>(stage);
  double* tri = stage + WAVE * HFP_DIM;                       // 64 x 10 tangent entries

  const int64_t ntiles = (n + WAVE - 1) / WAVE;
  const int64_t tile_stride = (int64_t)gridDim.x * WAVES_PER_BLOCK;
  unsigned c_plastic = 0, c_notconv = 0, c_nan = 0, c_maxit = 0;   // per thread: at most the number of its tiles

  const double lambda = prm.lambda, mu = prm.mu;
  const double SQ2 = 1.4142135623730950488;

  for (int64_t tile = (int64_t)blockIdx.x * WAVES_PER_BLOCK + wid; tile < ntiles; tile += tile_stride) {
    const int64_t base = tile * WAVE;
    const int npts = (n - base) < WAVE ? (int)(n - base) : WAVE;
    // per-lane invariants are re-derived per tile from an opaque copy (small_strain.hpp: hoisted, they cost registers over the whole body)
    asm volatile("" : "+v"(lane));
    lane &= WAVE - 1;
    const bool valid = lane < npts;
    // the tile's first point of every state stream is wave-uniform; the lane is a 32-bit offset to it
    const double* s0b = s0 + base;
    double* s1b = s1 + base;

    // ---- 1. the tile's strain rows: 128 x 16 B, coalesced, into LDS (zeros beyond the last point); the old state, SoA ----------
    {
      const double2_t* g2 = reinterpret_cast<const double2_t*>(eps + base * HFP_DIM);
      const int npairs = npts * 2;
#pragma unroll
      for (int pass = 0; pass < 2; ++pass) {
        const int q = lane + pass * WAVE;
        double2_t v = {0.0, 0.0};
        if (q < npairs) v = stream_load<2>(g2 + q);
        stage2[q] = v;
      }
    }
    double e[4], ep[4] = {0.0, 0.0, 0.0, 0.0}, p_n = 0.0;
    if (valid) {
      p_n = stream_load<3>(s0b + (int64_t)HFP_SLOT_P * ld + lane);
#pragma unroll
      for (int c = 0; c < 4; ++c) ep[c] = stream_load<3>(s0b + (int64_t)(HFP_SLOT_EP + c) * ld + lane);
    }
    wave_lds_sync();
    {
      const double2_t a = stage2[lane * 2], b = stage2[lane * 2 + 1];
      e[0] = a.x; e[1] = a.y; e[2] = b.x; e[3] = b.y;
    }
    wave_lds_sync();   // the staging region is reused for the stress below

    // ---- 2. trial state ----------------------------------------------------------------------------------------------------
#pragma unroll
    for (int c = 0; c < 4; ++c) e[c] -= ep[c];   // trial elastic strain
    const double tr = e[0] + e[1] + e[2];
    int ro = lane * HFP_TRI;   // opaque: every access is base + small immediate
    asm volatile("" : "+v"(ro));
    double* rec = tri + ro;   // the point's 10 tangent entries; while the local Newton runs it parks (c, s), the trial and the plastic strain
    double cchk = 0.0;   // sum of everything the point writes, for the non-finite check
    bool plastic = false;
    // new state (SoA) and the stress into the staging region: called once per point, as soon as the three are known
    auto finish = [&](const double* sg, const double* eel, const double* epl, double p_new) {
      if (valid) {
#pragma unroll
        for (int c = 0; c < 4; ++c) stream_store<1>(s1b + (int64_t)(HFP_SLOT_EEL + c) * ld + lane, eel[c]);
        stream_store<1>(s1b + (int64_t)HFP_SLOT_P * ld + lane, p_new);
#pragma unroll
        for (int c = 0; c < 4; ++c) stream_store<1>(s1b + (int64_t)(HFP_SLOT_EP + c) * ld + lane, epl[c]);
      }
      stage2[lane * 2] = double2_t{sg[0], sg[1]};
      stage2[lane * 2 + 1] = double2_t{sg[2], sg[3]};
      double chk = p_new;
#pragma unroll
      for (int c = 0; c < 4; ++c) chk += sg[c] + eel[c];
      cchk += chk;
    };
    const double R_n = prm.sig0 + prm.h1 * p_n;
    const double third = tr * (1.0 / 3.0);
    double vm;
    {
      const double d0 = e[0] - third, d1 = e[1] - third, d2 = e[2] - third;
      vm = 2.0 * mu * sqrt(1.5 * (d0 * d0 + d1 * d1 + d2 * d2 + e[3] * e[3]));
    }
    // seq <= max|s_i - s_j| <= 2 / sqrt(3) x the von Mises stress for every a >= 1: below that bound the point is elastic and the
    // eigen-solve is skipped (a hydrostatic trial state, vm = 0, never gets past it)
    if (1.1547005383792517 * vm > R_n) {
      // ---- 3. eigenbasis of the deviatoric trial stress: one rotation in the plane, e_z is principal -----------------------------
      double t0 = 2.0 * mu * (e[0] - third), t1 = 2.0 * mu * (e[1] - third);
      const double t2 = 2.0 * mu * (e[2] - third);
      const double t01 = SQ2 * mu * e[3];   // tensor component: Mandel / sqrt(2)
      double cs, sn;
      {
        const double d = t1 - t0;
        const double den = d + copysign(sqrt(d * d + 4.0 * t01 * t01), d);
        const double tau = den != 0.0 ? -2.0 * t01 * fast_rcp(den) : 0.0;
        cs = fast_rcp(sqrt(tau * tau + 1.0));
        sn = tau * cs;
        t0 += tau * t01;
        t1 -= tau * t01;
      }
      rec[0] = cs; rec[1] = sn;
#pragma unroll
      for (int c = 0; c < 4; ++c) { rec[2 + c] = e[c]; rec[6 + c] = ep[c]; }
      asm volatile("" ::: "memory");   // read back from LDS after the loop, not kept in registers
      // ---- 4. principal-space Newton (hosford.hip, section 4) ------------------------------------------------------------------
      const double am2 = prm.c[HF_AM2], inva = prm.c[HF_INVA], am1 = prm.c[HF_AM1];
      const double H = prm.h1, mu2 = 2.0 * mu;
      double q0 = t0, q1 = t1, q2 = t2, dp = 0.0;   // principal deviatoric stresses, plastic multiplier
      double seq, f0, f1, f2;                        // equivalent stress and flow direction of the last evaluation
      double x2, x3, l2, l3, u1, u2, u3, dmax, qq, qa2;
      double i00, i01, i02, i11, i12, i22, z0, z1, z2, nz;   // A'^-1, z = A'^-1 n, n.z
      double tolp = 0.0;
      unsigned iters = 0;
      plastic = true;
      for (;;) {
        const double d1 = q0 - q1, d2 = q1 - q2, d3 = q0 - q2;
        dmax = fmax(fabs(d1), fmax(fabs(d2), fabs(d3)));
        const double idm = 1.0 / dmax;
        const double x1 = d1 * idm;
        x2 = d2 * idm; x3 = d3 * idm;
        const double a1 = fabs(x1), a2 = fabs(x2), a3 = fabs(x3);
        const double l1 = log(a1);
        l2 = log(a2); l3 = log(a3);
        u1 = hfp_pow_am2(a1, l1, am2); u2 = hfp_pow_am2(a2, l2, am2); u3 = hfp_pow_am2(a3, l3, am2);
        const double phi = 0.5 * (u1 * a1 * a1 + u2 * a2 * a2 + u3 * a3 * a3);
        qq = exp(-inva * log(phi));
        seq = dmax / qq;
        qa2 = 1.0 / (phi * qq * qq);
        const double h1 = 0.5 * u1 * qa2, h2 = 0.5 * u2 * qa2, h3 = 0.5 * u3 * qa2;
        const double g1 = h1 * (x1 * qq), g2 = h2 * (x2 * qq), g3 = h3 * (x3 * qq);
        f0 = g1 + g3; f1 = g2 - g1; f2 = -g2 - g3;
        const double r4 = seq - prm.sig0 - H * (p_n + dp);
        if (iters == 0) {
          if (!(r4 > 0.0)) { plastic = false; break; }   // the trial state is inside the yield surface
          tolp = fmax(prm.tol, prm.rtol * seq);
        }
        // A' = I + w (B^T diag(h) B - n n^T), w = 2 mu dp (a - 1) / seq
        const double w = mu2 * dp * am1 / seq;
        const double a00 = 1.0 + w * (h1 + h3 - f0 * f0), a11 = 1.0 + w * (h1 + h2 - f1 * f1), a22 = 1.0 + w * (h2 + h3 - f2 * f2);
        const double a01 = w * (-h1 - f0 * f1), a02 = w * (-h3 - f0 * f2), a12 = w * (-h2 - f1 * f2);
        {
          const double c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
          const double idet = 1.0 / (a00 * c00 + a01 * c01 + a02 * c02);
          i00 = c00 * idet; i01 = c01 * idet; i02 = c02 * idet;
          i11 = (a00 * a22 - a02 * a02) * idet; i12 = (a01 * a02 - a00 * a12) * idet; i22 = (a00 * a11 - a01 * a01) * idet;
        }
        z0 = i00 * f0 + i01 * f1 + i02 * f2; z1 = i01 * f0 + i11 * f1 + i12 * f2; z2 = i02 * f0 + i12 * f1 + i22 * f2;
        nz = f0 * z0 + f1 * z1 + f2 * z2;
        const double r0 = (q0 - t0) + mu2 * dp * f0, r1 = (q1 - t1) + mu2 * dp * f1, r2 = (q2 - t2) + mu2 * dp * f2;
        const double res = fmax(fmax(fabs(r0), fabs(r1)), fmax(fabs(r2), fabs(r4)));
        if (res <= tolp) break;
        if (iters >= (unsigned)prm.maxit) { if (valid) ++c_notconv; break; }
        const double y0 = i00 * r0 + i01 * r1 + i02 * r2, y1 = i01 * r0 + i11 * r1 + i12 * r2, y2 = i02 * r0 + i12 * r1 + i22 * r2;
        const double ddp = (r4 - (f0 * y0 + f1 * y1 + f2 * y2)) / (mu2 * nz + H);
        q0 -= y0 + mu2 * z0 * ddp; q1 -= y1 + mu2 * z1 * ddp; q2 -= y2 + mu2 * z2 * ddp;
        dp += ddp;
        ++iters;
      }
      asm volatile("" ::: "memory");
      cs = rec[0]; sn = rec[1];
#pragma unroll
      for (int c = 0; c < 4; ++c) { e[c] = rec[2 + c]; ep[c] = rec[6 + c]; }
      if (plastic) {
        // ---- 5. moduli of the returned state; back to the global axes as Mandel 4-vectors --------------------------------------
        const double gden = mu2 * mu2 / (mu2 * nz + H);
        const double P00 = lambda + mu2 * i00 - gden * z0 * z0, P11 = lambda + mu2 * i11 - gden * z1 * z1, P22 = lambda + mu2 * i22 - gden * z2 * z2;
        const double P01 = lambda + mu2 * i01 - gden * z0 * z1, P02 = lambda + mu2 * i02 - gden * z0 * z2, P12 = lambda + mu2 * i12 - gden * z1 * z2;
        const double rs = qq * qa2 / dmax;   // q^(a-1) / max|d|
        // pair (0,1): difference d1, the other two d3 and d2
        const double rho01 = rs * (u1 + 0.5 * hfp_divided_difference(am1, x3, x2, l3, l2, u3, u2));
        const double th01 = mu2 / (1.0 + mu2 * dp * rho01);

        const double cc = cs * cs, ss = sn * sn, sc = SQ2 * (cs * sn);
        const double E0[4] = {cc, ss, 0.0, sc}, E1[4] = {ss, cc, 0.0, -sc}, E2[4] = {0.0, 0.0, 1.0, 0.0};
        const double M01[4] = {-sc, sc, 0.0, cc - ss};
        {
          const double ktr = prm.kappa * (e[0] + e[1] + e[2]);   // of the trial strain read back: the bits of tr
          double sg[4];
#pragma unroll
          for (int I = 0; I < 4; ++I) {
            const double fl = dp * (f0 * E0[I] + f1 * E1[I] + f2 * E2[I]);   // dp n
            sg[I] = (I < 3 ? ktr : 0.0) + q0 * E0[I] + q1 * E1[I] + q2 * E2[I];
            e[I] -= fl;
            ep[I] += fl;
          }
          finish(sg, e, ep, p_n + dp);
        }
        double X0[4], X1[4], X2[4];
#pragma unroll
        for (int I = 0; I < 4; ++I) {
          X0[I] = P00 * E0[I] + P01 * E1[I] + P02 * E2[I];
          X1[I] = P01 * E0[I] + P11 * E1[I] + P12 * E2[I];
          X2[I] = P02 * E0[I] + P12 * E1[I] + P22 * E2[I];
        }
#pragma unroll
        for (int I = 0; I < 4; ++I)
#pragma unroll
          for (int K = I; K < 4; ++K) {
            const double v = E0[I] * X0[K] + E1[I] * X1[K] + E2[I] * X2[K] + th01 * M01[I] * M01[K];
            rec[hfp_tri10(I, K)] = v;
            cchk += v;
          }
        if (valid) {
          ++c_plastic;
          c_maxit = iters > c_maxit ? iters : c_maxit;
        }
      }
    }
    if (!plastic) {
      const double ltr = lambda * tr;
      double sg[4];
      sg[0] = ltr + 2.0 * mu * e[0]; sg[1] = ltr + 2.0 * mu * e[1]; sg[2] = ltr + 2.0 * mu * e[2];
      sg[3] = 2.0 * mu * e[3];
      finish(sg, e, ep, p_n);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int k = i; k < 4; ++k) rec[hfp_tri10(i, k)] = ((i < 3 && k < 3) ? lambda : 0.0) + ((i == k) ? 2.0 * mu : 0.0);
    }
    // stress, state and tangent
    if (valid && !(fabs(cchk) <= 1.79769313486231570e308)) ++c_nan;
    wave_lds_sync();

    // ---- 6. the stress rows, as the strain came in ------------------------------------------------------------------------------
    {
      double2_t* f2g = reinterpret_cast<double2_t*>(sig + base * HFP_DIM);
      const int npairs = npts * 2;
#pragma unroll
      for (int pass = 0; pass < 2; ++pass) {
        const int q = lane + pass * WAVE;
        if (q < npairs) stream_store<0>(f2g + q, stage2[q]);
      }
    }
    // ---- 7. the tangent in output order: 8 passes of 64 x 16 B, pair (ti, tj..tj+1) of point 8 k + tq ---------------------------
    {
      // this lane's pair: row ti, columns tj and tj + 1 of the point 8 k + tq in pass k, as slots of the staged triangle
      const int tq = lane >> 3, ti = (lane & 7) >> 1, tj = (lane & 1) * 2;
      const int slot0 = hfp_tri10(ti, tj), slot1 = hfp_tri10(ti, tj + 1);
      double2_t* c2g = reinterpret_cast<double2_t*>(ct + base * HFP_CT);
#pragma unroll
      for (int pass = 0; pass < 8; ++pass) {
        const int q = pass * 8 + tq;
        const double* r = tri + q * HFP_TRI;
        const double2_t v = {r[slot0], r[slot1]};
        if (q < npts) stream_store<0>(c2g + pass * WAVE + lane, v);
      }
    }
    wave_lds_sync();   // the LDS region is rewritten by the next tile
  }

  store_block_stats(stats, c_plastic, c_notconv, c_nan, c_maxit, red);
}

const void* hosford_plane_kernel_fn() { return (const void*)hosford_plane_kernel; }

void hosford_plane_launch(int grid, hipStream_t st, const LawParams& prm, int64_t cnt, const double* grad, const double* s0, double* s1,
                          int64_t ld, double* flux, double* ct, BlockStats* bs) {
  hipLaunchKernelGGL(hosford_plane_kernel, dim3(grid), dim3(BLOCK), 0, st, prm, cnt, grad, s0, s1, ld, flux, ct, bs);
}

}  // namespace dxm
