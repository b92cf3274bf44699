// Ogden hyperelasticity under the plane-strain hypothesis (gradient F (5) = [F00, F11, F22, F01, F10], flux PK1 (5) in the same order,
// the 5x5 tangent dP/dF, one internal state variable PK2Stress (4) = [xx, yy, zz, sqrt(2) xy]) for gfx950.
//
// By definition the law is DXM_LAW_OGDEN (hyperelastic.hip, whose header comment states the energy and the principal-value formulas)
// on F = [[F00, F01, 0], [F10, F11, 0], [0, 0, F22]], restricted to the components such an F has.  C = F^T F is then a 2x2 block plus
// c2 = F22^2 with the eigenvector e_z:
//   * one Jacobi rotation diagonalises the block exactly (principal_axes.hpp: the rotation law 7 sweeps five times over three planes);
//   * the kept rows and columns of A[(i,J),(k,L)] = sum_MP F[i][M] CC[MJ][PL] F[k][P] + delta_ik S[L][J] read CC = 2 dS/dC only in
//     the four components [00, 11, 22, 01], a symmetric 4x4 of 10 entries: the out-of-plane shear directions G02, G12 and with them
//     the divided differences th02, th12 drop out, th01 is the only one;
//   * S_i, D_ij, Q2, the divided difference with its series switch and f3 through opaque() are the formulas of hyperelastic.hip,
//     copied (that unit is not touched: its assembly is pinned).
// One thread per point evaluates all of it; there is no second role for a lane, unlike the 81-entry tangent of law 7.
//
// Mapping and I/O: one wave per tile of 64 points, 256-thread workgroups, tiles walked grid-stride; LDS is wave-private and ordered by
// wave_lds_sync(), no workgroup barrier inside the tile loop.  plane5_rows5_*.hpp move F in and PK1 out (2560 B per tile, 16 B per lane
// through LDS); in rounds of OGP_PPR = 32 points the lanes of the round write their 25 tangent entries to the wave's out-tile and
// plane5_out25_copyout.hpp copies the round's 6400 B out in output order, 16 B per lane, non-temporal, every 128 B line whole
// (ogden_plane.hpp: why rounds of 32).  The state leaves as four 8 B-per-lane SoA streams.  312 B per point.
#include "ogden_plane.hpp"

#include "hyperelastic.hpp"   // the slots of LawParams law 7's build function fills (OG_A, OG_AM2, OG_MA3, OG_M)
#include "principal_axes.hpp"

namespace dxm {

// (c_i^m - c_j^m) / (c_i - c_j) from c, ln c, c^(m-1), c^m of both (hyperelastic.hip, header comment)
__device__ __forceinline__ double ogp_divided_difference(double m, double ci, double cj, double li, double lj, double pwi, double pwj, double ui,
                                                         double uj) {
  const double h = 0.5 * (li - lj), y = m * h;
  const double series = m * sqrt(pwi * pwj) * sinhc_series(y * y) * fast_rcp(sinhc_series(h * h));
  const double quotient = (ui - uj) * fast_rcp(ci - cj);
  return fmax(fabs(y), fabs(h)) <= 0.1 ? series : quotient;
}

// slot of the pair (a, b) in the symmetric 4-vector [00, 11, 22, 01]; (a, b) both in the plane or both 2
constexpr int ogp_sym4(int a, int b) { return a == b ? a : 3; }
// slot of entry (i <= k) of a symmetric 4x4 kept as its upper triangle, row by row
constexpr int ogp_tri10(int i, int k) { return i <= k ? i * 4 - i * (i - 1) / 2 + (k - i) : k * 4 - k * (k - 1) / 2 + (i - k); }

__global__ void __launch_bounds__(BLOCK)
ogden_plane_kernel(const LawParams prm, const int64_t n, const double* __restrict__ Fin, double* __restrict__ s1, const int64_t ld,
                   double* __restrict__ Pout, double* __restrict__ ct, BlockStats* __restrict__ stats) {
  __shared__ __attribute__((aligned(16))) double lds_all[WAVES_PER_BLOCK * OGP_LDS_PER_WAVE];
  static_assert(sizeof(lds_all) == OGP_LDS_BYTES, "the LDS that ogden_plane.hpp states");

  const int lane0 = threadIdx.x & (WAVE - 1);
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform: tile bookkeeping in scalar registers
  double* outt = lds_all + wid * OGP_LDS_PER_WAVE;   // the tangent out-tile of this wave ...
  double* stage = outt;                              // ... whose start stages F in and PK1 out
  double2_t* stage2 = reinterpret_cast<double2_t*>(stage);

  const int64_t ntiles = (n + WAVE - 1) / WAVE;
  const int64_t tile_stride = (int64_t)gridDim.x * WAVES_PER_BLOCK;
  unsigned long long c_nan = 0;

  const double mu = prm.mu, kappa = prm.kappa;
  const double a = prm.c[OG_A], am2 = prm.c[OG_AM2], ma3 = prm.c[OG_MA3], m = prm.c[OG_M];
  const double SQ2 = 1.4142135623730950488;
  constexpr int RI[5] = {0, 1, 2, 0, 1};   // row index of entry t of the 5-vector
  constexpr int RJ[5] = {0, 1, 2, 1, 0};   // column index           (utils.py:168-172)
  int lane = lane0;

  for (int64_t tile = (int64_t)blockIdx.x * WAVES_PER_BLOCK + wid; tile < ntiles; tile += tile_stride) {
    const int64_t base = tile * WAVE;
    const int npts = (n - base) < WAVE ? (int)(n - base) : WAVE;
    // per-lane invariants are re-derived per tile from an opaque copy (fefp.hpp: hoisted, they cost registers over the whole body)
    asm volatile("" : "+v"(lane));
    lane &= WAVE - 1;
    const bool valid = lane < npts;
    const int64_t gi = base + lane;

    // ---- 1. F through LDS (64 x 5 doubles = 160 double2 per tile) -------------------------------------
    double F5[5];
#include "plane5_rows5_load.hpp"
    wave_lds_sync();
#include "plane5_rows5_take.hpp"
    wave_lds_sync();
    const double F00 = F5[0], F11 = F5[1], F22 = F5[2], F01 = F5[3], F10 = F5[4];

    // ---- 2. C = F^T F: a 2x2 block and c2; one rotation diagonalises the block ---------------------------
    double J = F22 * (F00 * F11 - F01 * F10);
    J = J > 0.0 ? J : __builtin_nan("");   // an inverted or flat point has no answer: NaN outputs, counted below
    double c0 = F00 * F00 + F10 * F10;
    double c1 = F11 * F11 + F01 * F01;
    double c01 = F00 * F01 + F10 * F11;
    const double c2 = F22 * F22;
    double n0[3] = {1.0, 0.0, 0.0}, n1[3] = {0.0, 1.0, 0.0};   // eigenvector columns; the third is e_z
    {
      double r0 = 0.0, r1 = 0.0;   // the entries that couple the plane to z: none
      jacobi_rotate(c0, c1, c01, r0, r1, n0, n1);
    }

    // ---- 3. principal stresses and moduli (hyperelastic.hip, section 3) ---------------------------------------
    double S4[4], CC[10];
    {
      const double l0 = log(c0), l1 = log(c1), l2 = log(c2);
      const double i0 = fast_rcp(c0), i1 = fast_rcp(c1), i2 = fast_rcp(c2);
      const double pw0 = exp(am2 * l0), pw1 = exp(am2 * l1), pw2 = exp(am2 * l2);   // c^(a-2) = c^(m-1)
      const double u0 = c0 * pw0, u1 = c1 * pw1, u2 = c2 * pw2;                       // c^m
      const double f = c0 * u0 + c1 * u1 + c2 * u2;                                   // sum c^a
      const double A0 = mu * exp(ma3 * (l0 + l1 + l2)) + 0.0 * J;                     // mu det(C)^(-a/3); NaN with J
      const double p = kappa * (J - 1.0) * J;
      // f / 3 as one rounded value: contracted into the differences below, the unrounded product 3 x 0.333... would leave
      // mu x 5.6e-17 of isochoric stress at F = I instead of an exact zero
      const double f3 = opaque(f * (1.0 / 3.0));
      const double q = p - A0 * f3;
      const double s0 = A0 * u0 + q * i0, sp1 = A0 * u1 + q * i1, s2 = A0 * u2 + q * i2;
      const double t0 = A0 * (u0 - f3 * i0), t1 = A0 * (u1 - f3 * i1), t2 = A0 * (u2 - f3 * i2);
      const double Q2 = 0.5 * kappa * (2.0 * J - 1.0) * J + a * A0 * f * (1.0 / 9.0);
      const double aA3 = a * A0 * (1.0 / 3.0);
      const double D00 = 2.0 * (Q2 * i0 * i0 - aA3 * 2.0 * u0 * i0 + A0 * m * pw0 - q * i0 * i0);
      const double D11 = 2.0 * (Q2 * i1 * i1 - aA3 * 2.0 * u1 * i1 + A0 * m * pw1 - q * i1 * i1);
      const double D22 = 2.0 * (Q2 * i2 * i2 - aA3 * 2.0 * u2 * i2 + A0 * m * pw2 - q * i2 * i2);
      const double D01 = 2.0 * (Q2 * i0 * i1 - aA3 * (u0 * i1 + u1 * i0));
      const double D02 = 2.0 * (Q2 * i0 * i2 - aA3 * (u0 * i2 + u2 * i0));
      const double D12 = 2.0 * (Q2 * i1 * i2 - aA3 * (u1 * i2 + u2 * i1));
      const double th01 = A0 * ogp_divided_difference(m, c0, c1, l0, l1, pw0, pw1, u0, u1) - q * i0 * i1;

      // back to the global axes in the components [00, 11, 22, 01]: E_i = n_i n_i, G01 = n0 n1 + n1 n0; E2 = e_z e_z = (0, 0, 1, 0)
      const double E0[4] = {n0[0] * n0[0], n0[1] * n0[1], 0.0, n0[0] * n0[1]};
      const double E1[4] = {n1[0] * n1[0], n1[1] * n1[1], 0.0, n1[0] * n1[1]};
      const double E2[4] = {0.0, 0.0, 1.0, 0.0};
      const double G01[4] = {2.0 * n0[0] * n1[0], 2.0 * n0[1] * n1[1], 0.0, n0[0] * n1[1] + n1[0] * n0[1]};
      double Si4[4];
#pragma unroll
      for (int I = 0; I < 4; ++I) {
        S4[I] = s0 * E0[I] + sp1 * E1[I] + s2 * E2[I];
        Si4[I] = t0 * E0[I] + t1 * E1[I] + t2 * E2[I];
      }
      if (valid) {
        stream_store<1>(s1 + 0 * ld + gi, Si4[0]);
        stream_store<1>(s1 + 1 * ld + gi, Si4[1]);
        stream_store<1>(s1 + 2 * ld + gi, Si4[2]);
        stream_store<1>(s1 + 3 * ld + gi, SQ2 * Si4[3]);
      }
      double X0[4], X1[4], X2[4];   // D E
#pragma unroll
      for (int I = 0; I < 4; ++I) {
        X0[I] = D00 * E0[I] + D01 * E1[I] + D02 * E2[I];
        X1[I] = D01 * E0[I] + D11 * E1[I] + D12 * E2[I];
        X2[I] = D02 * E0[I] + D12 * E1[I] + D22 * E2[I];
      }
#pragma unroll
      for (int I = 0; I < 4; ++I)
#pragma unroll
        for (int Kx = I; Kx < 4; ++Kx)
          CC[ogp_tri10(I, Kx)] = E0[I] * X0[Kx] + E1[I] * X1[Kx] + E2[I] * X2[Kx] + th01 * G01[I] * G01[Kx];
      // non-finite results (J <= 0, a non-finite F): every output of the point is a combination of these with finite weights
      const double chk = ((s0 + sp1) + (s2 + D00)) + ((D11 + D22) + (D01 + D02)) + (D12 + th01);
      if (valid && !(fabs(chk) <= 1.79769313486231570e308)) ++c_nan;
    }

    // ---- 4. PK1 = F S through LDS, coalesced store --------------------------------------------------------
    {
      double P5[5];
      P5[0] = F00 * S4[0] + F01 * S4[3];
      P5[1] = F10 * S4[3] + F11 * S4[1];
      P5[2] = F22 * S4[2];
      P5[3] = F00 * S4[3] + F01 * S4[1];
      P5[4] = F10 * S4[0] + F11 * S4[3];
#include "plane5_rows5_put.hpp"
    }
    wave_lds_sync();
#include "plane5_rows5_store.hpp"
    wave_lds_sync();   // the out-tile below aliases the staging region

    // ---- 5. tangent: column (k, L) at a time, B[MJ] = sum_P CC[MJ][PL] F[k][P], then A[(i,J),(k,L)] = sum_M F[i][M] B[MJ] + delta_ik S[L][J]
#pragma unroll 1
    for (int rd = 0; rd < WAVE / OGP_PPR; ++rd) {
      if (lane / OGP_PPR == rd) {
        int ro = (lane % OGP_PPR) * OGP_CT;   // opaque: every write below is base + small immediate (fefp.hpp)
        asm volatile("" : "+v"(ro));
        double* rec = outt + ro;
#pragma unroll
        for (int col = 0; col < 5; ++col) {
          const int k = RI[col], L = RJ[col];
          double B[4];
          if (k == 2) {
#pragma unroll
            for (int I = 0; I < 4; ++I) B[I] = CC[ogp_tri10(I, 2)] * F22;
          } else {
            const double Fk0 = k == 0 ? F00 : F10, Fk1 = k == 0 ? F01 : F11;
#pragma unroll
            for (int I = 0; I < 4; ++I) B[I] = CC[ogp_tri10(I, ogp_sym4(0, L))] * Fk0 + CC[ogp_tri10(I, ogp_sym4(1, L))] * Fk1;
          }
#pragma unroll
          for (int r = 0; r < 5; ++r) {
            const int i = RI[r], Jx = RJ[r];
            double t;
            if (i == 2) {
              t = F22 * B[2];
            } else {
              const double Fi0 = i == 0 ? F00 : F10, Fi1 = i == 0 ? F01 : F11;
              t = Fi0 * B[ogp_sym4(0, Jx)] + Fi1 * B[ogp_sym4(1, Jx)];
            }
            if (i == k) t += S4[ogp_sym4(L, Jx)];
            rec[r * 5 + col] = t;
          }
        }
      }
      wave_lds_sync();
      const int p0 = rd * OGP_PPR;
#include "plane5_out25_copyout.hpp"
      wave_lds_sync();   // the next round's records, or the next tile's F, go over the out-tile
    }
  }
  // the workgroup reduction borrows the first words of every wave's own region (the tile loop is over)
  store_block_stats(stats, 0, 0, c_nan, 0, reinterpret_cast<unsigned long long*>(lds_all), OGP_LDS_PER_WAVE);
}

const void* ogden_plane_kernel_fn() { return (const void*)ogden_plane_kernel; }

void ogden_plane_launch(int grid, hipStream_t st, const LawParams& prm, int64_t cnt, const double* F, double* s1, int64_t ld, double* P,
                        double* ct, BlockStats* bs) {
  hipLaunchKernelGGL(ogden_plane_kernel, dim3(grid), dim3(BLOCK), 0, st, prm, cnt, F, s1, ld, P, ct, bs);
}

}  // namespace dxm
