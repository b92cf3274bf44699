// Logarithmic-strain J2 plasticity with linear hardening under the plane-strain hypothesis (gradient F (5) = [F00, F11, F22, F01, F10],
// flux PK1 (5) in the same order, the 5x5 tangent dP/dF; internal state variables ElasticStrain (4) and EquivalentPlasticStrain (1),
// hidden state PlasticStrain (4), the symmetric tensors as [xx, yy, zz, sqrt(2) xy]) for gfx950.
//
// By definition the law is DXM_LAW_LOG_STRAIN_J2 (log_strain.hip, whose header comment states the construction step by step) on
// F = [[F00, F01, 0], [F10, F11, 0], [0, 0, F22]], restricted to the components such an F has.  C = F^T F is then a 2x2 block plus
// c2 = F22^2 with the eigenvector e_z, and the old plastic strain has no out-of-plane shear:
//   * one Jacobi rotation diagonalises the block exactly (principal_axes.hpp: the rotation law 19 sweeps five times over three
//     planes); c01 = 0 passes through with (cos, sin) = (1, 0);
//   * every tensor of the law has four components in the eigenbasis, B = (E_0, E_1, E_2, G_01) written as 4-vectors [xx, yy, zz, xy]
//     with E_2 = (0, 0, 1, 0): its G_02 and G_12 components are zero, so th_02, th_12, g_002, g_220, g_112, g_221 and g_012 multiply
//     zeros and drop out.  One first divided difference th_01 and two second ones g_001, g_110 remain, none of them involves c2;
//   * CC^ is a symmetric 4x4 of 10 entries and CC = B^T CC^ B a 4x4 change of basis (law 19: 21 entries, 6x6);
//   * the radial return is law 19's line by line on the four components (T is not coaxial with C once there is a history).
// lsp_theta / lsp_gamma are copies of log_strain.hip's ls_theta / ls_gamma (that unit is not touched: its assembly is pinned).
// One thread per point evaluates all of it; there is no second role for a lane, unlike the 81-entry tangent of law 19.
//
// Mapping and I/O are those of ogden_plane.hip: one wave per tile of 64 points, 256-thread workgroups, tiles walked grid-stride; LDS
// is wave-private and ordered by wave_lds_sync(), no workgroup barrier inside the tile loop.  plane5_rows5_*.hpp move F in and PK1
// out; in rounds of LSP_PPR = 32 points the lanes of the round write their 25 tangent entries to the wave's out-tile and
// plane5_out25_copyout.hpp copies the round's 6400 B out in output order, 16 B per lane, non-temporal, every 128 B line whole.  The
// state is SoA, 8 B per lane: five streams in (p, Ep), nine out.  392 B per point.
#include "log_strain_plane.hpp"

#include "principal_axes.hpp"

namespace dxm {

constexpr double LSP_GAMMA_SWITCH = 0.05;   // max |d| up to which lsp_gamma takes its Taylor form
constexpr int LSP_GAMMA_TERMS = 15;         // n = 0 .. 14: the first dropped term is below 136 x 0.05^15 / 17 = 2.4e-19

// ln[c_i, c_j] from the two values and y = (ln c_i - ln c_j) / 2   (log_strain.hip::ls_theta)
__device__ __forceinline__ double lsp_theta(double ci, double cj, double y) {
  const double ey = exp(y);
  const double far = 0.5 * (ey - fast_rcp(ey)) / y;
  const double sc = fabs(y) <= 0.1 ? sinhc_series(y * y) : far;
  return fast_rcp(sqrt(ci * cj) * sc);
}

// ln[ca, ck, cb]: the Taylor form in the relative distances to the mean where they are at most LSP_GAMMA_SWITCH, `far` beyond: the
// quotient of first differences over the largest gap, which the caller forms   (log_strain.hip::ls_gamma)
__device__ __forceinline__ double lsp_gamma(double ca, double ck, double cb, double far) {
  const double m = (ca + ck + cb) * (1.0 / 3.0);
  const double im = fast_rcp(m);
  const double d0 = (ca - m) * im, d1 = (ck - m) * im, d2 = (cb - m) * im;
  const double e1 = d0 + d1 + d2, e2 = d0 * d1 + d0 * d2 + d1 * d2, e3 = d0 * d1 * d2;
  double h3 = 0.0, h2 = 0.0, h1 = 1.0, acc = -0.5;
#pragma unroll
  for (int n = 1; n < LSP_GAMMA_TERMS; ++n) {
    const double h = e1 * h1 - e2 * h2 + e3 * h3;
    acc += ((n & 1) ? 1.0 : -1.0) / (double)(n + 2) * h;
    h3 = h2; h2 = h1; h1 = h;
  }
  const bool small = fmax(fabs(d0), fmax(fabs(d1), fabs(d2))) <= LSP_GAMMA_SWITCH;
  return small ? acc * im * im : far;
}

// slot of the pair (a, b) in the symmetric 4-vector [00, 11, 22, 01]; (a, b) both in the plane or both 2
constexpr int lsp_sym4(int a, int b) { return a == b ? a : 3; }
// slot of entry (i, k) of a symmetric 4x4 kept as its upper triangle, row by row
constexpr int lsp_tri10(int i, int k) { return i <= k ? i * 4 - i * (i - 1) / 2 + (k - i) : k * 4 - k * (k - 1) / 2 + (i - k); }

__global__ void __launch_bounds__(BLOCK)
log_strain_plane_kernel(const LawParams prm, const int64_t n, const double* __restrict__ Fin, const double* __restrict__ s0,
                        double* __restrict__ s1, const int64_t ld, double* __restrict__ Pout, double* __restrict__ ct,
                        BlockStats* __restrict__ stats) {
  __shared__ __attribute__((aligned(16))) double lds_all[WAVES_PER_BLOCK * LSP_LDS_PER_WAVE];
  static_assert(sizeof(lds_all) == LSP_LDS_BYTES, "the LDS that log_strain_plane.hpp states");
  constexpr int OGP_PPR = LSP_PPR;   // the name under which plane5_out25_copyout.hpp reads the round size

  const int lane0 = threadIdx.x & (WAVE - 1);
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform: tile bookkeeping in scalar registers
  double* outt = lds_all + wid * LSP_LDS_PER_WAVE;   // the tangent out-tile of this wave ...
  double* stage = outt;                              // ... whose start stages F in and PK1 out
  double2_t* stage2 = reinterpret_cast<double2_t*>(stage);

  const int64_t ntiles = (n + WAVE - 1) / WAVE;
  const int64_t tile_stride = (int64_t)gridDim.x * WAVES_PER_BLOCK;
  unsigned long long c_plastic = 0, c_nan = 0;

  const double lambda = prm.lambda, mu = prm.mu;
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

    // ---- 1. F through LDS (64 x 5 doubles = 160 double2 per tile); old state, SoA ---------------------------------
    double F5[5];
    double ep[4] = {0.0, 0.0, 0.0, 0.0}, p_n = 0.0;   // Mandel
#include "plane5_rows5_load.hpp"
    if (valid) {
      p_n = stream_load<3>(s0 + (int64_t)LSP_SLOT_P * ld + gi);
#pragma unroll
      for (int c = 0; c < 4; ++c) ep[c] = stream_load<3>(s0 + (int64_t)(LSP_SLOT_EP + c) * ld + gi);
    }
    wave_lds_sync();
#include "plane5_rows5_take.hpp"
    wave_lds_sync();
    const double F00 = F5[0], F11 = F5[1], F22 = F5[2], F01 = F5[3], F10 = F5[4];

    // ---- 2. C = F^T F: a 2x2 block and c2; one rotation diagonalises the block ---------------------------------
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

    // ---- 3. the update in the eigenbasis, stresses and moduli (log_strain.hip, section 3) ---------------------
    double S4[4], CC[10];
    {
      // B = (E_0, E_1, E_2, G_01) as 4-vectors of tensor components [00, 11, 22, 01]: X = sum_a X^_a B_a
      const double B[4][4] = {{n0[0] * n0[0], n0[1] * n0[1], 0.0, n0[0] * n0[1]},
                              {n1[0] * n1[0], n1[1] * n1[1], 0.0, n1[0] * n1[1]},
                              {0.0, 0.0, 1.0, 0.0},
                              {2.0 * n0[0] * n1[0], 2.0 * n0[1] * n1[1], 0.0, n0[0] * n1[1] + n1[0] * n0[1]}};
      const double nanJ = 0.0 * J;   // NaN with J, else zero
      const double l0 = log(c0), l1 = log(c1), l2 = log(c2);
      const double e0 = 0.5 * l0, e1 = 0.5 * l1, e2 = 0.5 * l2;
      // trial elastic strain in the eigenbasis: diag(e) - N^T Ep_n N; X^_ii = E_i : X, X^_01 = G_01 : X / 2 (the off-diagonal tensor
      // component counts twice; the state is Mandel: tensor component = Mandel / sqrt(2))
      double ee[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        const double t = B[a][0] * ep[0] + B[a][1] * ep[1] + B[a][2] * ep[2] + SQ2 * (B[a][3] * ep[3]);
        ee[a] = a < 3 ? -t : -0.5 * t;
      }
      ee[0] += e0; ee[1] += e1; ee[2] += e2;
      const double tr = ee[0] + ee[1] + ee[2];
      const double third = tr * (1.0 / 3.0);
      const double dv[4] = {ee[0] - third, ee[1] - third, ee[2] - third, ee[3]};
      const double seq = 2.0 * mu * sqrt(1.5 * (dv[0] * dv[0] + dv[1] * dv[1] + dv[2] * dv[2] + 2.0 * (dv[3] * dv[3])));
      const double ftr = seq - (prm.sig0 + prm.h1 * p_n);
      const bool plastic = ftr > 0.0;
      // closed-form radial return (IsotropicLinearHardeningPlasticity.mfront:49-77): n = 3/2 s / seq, dp = f / (H + 3 mu)
      const double gam = 1.0 / (prm.h1 + 3.0 * mu);
      const double dp = plastic ? ftr * gam : 0.0;
      const double iseq = plastic ? 1.0 / seq : 0.0;
      const double beta = dp * iseq;
      const double k1 = lambda + 2.0 * mu * mu * beta, k2 = 2.0 * mu - 6.0 * mu * mu * beta;
      const double k3 = plastic ? 4.0 * mu * mu * (beta - gam) : 0.0;
      double nf[4], Th[4];   // flow direction and stress, eigenbasis components
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        nf[a] = 3.0 * mu * dv[a] * iseq;
        const double el = ee[a] - dp * nf[a];
        Th[a] = (a < 3 ? lambda * tr : 0.0) + 2.0 * mu * el;
      }
      const double p_new = p_n + dp;
      // new state, global axes, Mandel: Ep = Ep_n + dp N n^ N^T, eel = E - Ep
      {
        double chk = p_new;
#pragma unroll
        for (int I = 0; I < 4; ++I) {
          const double wI = I < 3 ? 1.0 : SQ2;
          double dE = 0.0;
          const double Eg = e0 * B[0][I] + e1 * B[1][I] + e2 * B[2][I];
#pragma unroll
          for (int a = 0; a < 4; ++a) dE += nf[a] * B[a][I];
          const double epn = ep[I] + wI * dp * dE;
          const double eel = wI * Eg - epn + nanJ;
          chk += eel;
          if (valid) {
            stream_store<1>(s1 + (int64_t)(LSP_SLOT_EEL + I) * ld + gi, eel);
            stream_store<1>(s1 + (int64_t)(LSP_SLOT_EP + I) * ld + gi, epn + nanJ);
          }
        }
        if (valid) stream_store<1>(s1 + (int64_t)LSP_SLOT_P * ld + gi, p_new + nanJ);
        if (valid && !(fabs(chk) <= 1.79769313486231570e308)) ++c_nan;
        else if (valid && plastic) ++c_plastic;
      }

      // first divided differences (NaN with J: every output below is a combination of these)
      const double i0 = fast_rcp(c0), i1 = fast_rcp(c1), i2 = fast_rcp(c2);
      const double th01 = lsp_theta(c0, c1, e0 - e1);
      const double th[4] = {i0 + nanJ, i1 + nanJ, i2 + nanJ, th01 + nanJ};
#pragma unroll
      for (int I = 0; I < 4; ++I) {
        double s = 0.0;
#pragma unroll
        for (int a = 0; a < 4; ++a) s += (th[a] * Th[a]) * B[a][I];
        S4[I] = s;
      }

      // second divided differences; beyond the switch the quotient over the gap: (1 / c_i - th_ij) / (c_i - c_j)
      const double g001 = lsp_gamma(c0, c0, c1, (i0 - th01) / (c0 - c1)), g110 = lsp_gamma(c1, c1, c0, (i1 - th01) / (c1 - c0));

      // CC^ = th Ct^ th + G^ (upper triangle in the basis B)
      double Ch[10];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = a; b < 4; ++b) {
          double v = k3 * nf[a] * nf[b];
          if (a < 3 && b < 3) v += k1;
          if (a == b) v += a < 3 ? k2 : 0.5 * k2;
          Ch[lsp_tri10(a, b)] = th[a] * th[b] * v;
        }
      Ch[lsp_tri10(0, 0)] -= 2.0 * Th[0] * i0 * i0;   // 4 T^_ii g_iii, g_iii = -1 / (2 c_i^2)
      Ch[lsp_tri10(1, 1)] -= 2.0 * Th[1] * i1 * i1;
      Ch[lsp_tri10(2, 2)] -= 2.0 * Th[2] * i2 * i2;
      Ch[lsp_tri10(0, 3)] += 2.0 * Th[3] * g001;
      Ch[lsp_tri10(1, 3)] += 2.0 * Th[3] * g110;
      Ch[lsp_tri10(3, 3)] += Th[1] * g110 + Th[0] * g001;

      // back to the global axes, column by column: x = CC^ B[.][K], CC[I][K] = sum_a B[a][I] x[a]
#pragma unroll
      for (int Kx = 0; Kx < 4; ++Kx) {
        double x[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          double t = 0.0;
#pragma unroll
          for (int b = 0; b < 4; ++b) t += Ch[lsp_tri10(a, b)] * B[b][Kx];
          x[a] = t;
        }
#pragma unroll
        for (int I = 0; I <= Kx; ++I) {
          double t = 0.0;
#pragma unroll
          for (int a = 0; a < 4; ++a) t += B[a][I] * x[a];
          CC[lsp_tri10(I, Kx)] = t;
        }
      }
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

    // ---- 5. tangent (ogden_plane.hip, step 5): column (k, L) at a time, B[MJ] = sum_P CC[MJ][PL] F[k][P], then
    //         A[(i,J),(k,L)] = sum_M F[i][M] B[MJ] + delta_ik S[L][J]
#pragma unroll 1
    for (int rd = 0; rd < WAVE / LSP_PPR; ++rd) {
      if (lane / LSP_PPR == rd) {
        int ro = (lane % LSP_PPR) * LSP_CT;   // opaque: every write below is base + small immediate (fefp.hpp)
        asm volatile("" : "+v"(ro));
        double* rec = outt + ro;
#pragma unroll
        for (int col = 0; col < 5; ++col) {
          const int k = RI[col], L = RJ[col];
          double Bv[4];
          if (k == 2) {
#pragma unroll
            for (int I = 0; I < 4; ++I) Bv[I] = CC[lsp_tri10(I, 2)] * F22;
          } else {
            const double Fk0 = k == 0 ? F00 : F10, Fk1 = k == 0 ? F01 : F11;
#pragma unroll
            for (int I = 0; I < 4; ++I) Bv[I] = CC[lsp_tri10(I, lsp_sym4(0, L))] * Fk0 + CC[lsp_tri10(I, lsp_sym4(1, L))] * Fk1;
          }
#pragma unroll
          for (int r = 0; r < 5; ++r) {
            const int i = RI[r], Jx = RJ[r];
            double t;
            if (i == 2) {
              t = F22 * Bv[2];
            } else {
              const double Fi0 = i == 0 ? F00 : F10, Fi1 = i == 0 ? F01 : F11;
              t = Fi0 * Bv[lsp_sym4(0, Jx)] + Fi1 * Bv[lsp_sym4(1, Jx)];
            }
            if (i == k) t += S4[lsp_sym4(L, Jx)];
            rec[r * 5 + col] = t;
          }
        }
      }
      wave_lds_sync();
      const int p0 = rd * LSP_PPR;
#include "plane5_out25_copyout.hpp"
      wave_lds_sync();   // the next round's records, or the next tile's F, go over the out-tile
    }
  }
  // the workgroup reduction borrows the first words of every wave's own region (the tile loop is over)
  store_block_stats(stats, c_plastic, 0, c_nan, 0, reinterpret_cast<unsigned long long*>(lds_all), LSP_LDS_PER_WAVE);
}

const void* log_strain_plane_kernel_fn() { return (const void*)log_strain_plane_kernel; }

void log_strain_plane_launch(int grid, hipStream_t st, const LawParams& prm, int64_t cnt, const double* F, const double* s0, double* s1,
                             int64_t ld, double* P, double* ct, BlockStats* bs) {
  hipLaunchKernelGGL(log_strain_plane_kernel, dim3(grid), dim3(BLOCK), 0, st, prm, cnt, F, s0, s1, ld, P, ct, bs);
}

}  // namespace dxm
