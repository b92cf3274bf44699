// Ogden hyperelasticity (gradient F (9), flux PK1 (9), 9x9 tangent dP/dF, one internal state variable PK2Stress (6)) for gfx950.
//
// The law is the reference's demos/mfront/hyperelasticity/Ogden.mfront, restated from its stored energy
//   W(F) = (mu / alpha) (J^(-alpha/3) sum_i c_i^a - 3) + K/2 (J - 1)^2,     a = alpha / 2, C = F^T F = sum_i c_i n_i n_i^T, J = det F.
// W depends on C through its eigenvalues only, so S = 2 dW/dC is coaxial with C and everything is evaluated in the eigenbasis:
// with g = det(C)^(-a/3), f = sum c_i^a, m = a - 1, p = K (J - 1) J and q = p - mu g f / 3
//   S_i     = mu g c_i^m + q / c_i                       (the isochoric part alone, the ISV: mu g (c_i^m - f / (3 c_i)))
//   D_ij    = 2 dS_i/dc_j = 2 [Q2 / (c_i c_j) - (a mu g / 3) (c_i^m / c_j + c_j^m / c_i)] + 2 delta_ij [mu g m c_i^(m-1) - q / c_i^2],
//             Q2 = K (2 J - 1) J / 2 + a mu g f / 9
//   th_ij   = (S_i - S_j) / (c_i - c_j) = mu g DD_m(c_i, c_j) - q / (c_i c_j)
//   CC      = 2 dS/dC = sum_ij D_ij (n_i n_i)(n_j n_j) + sum_{i<j} th_ij (n_i n_j + n_j n_i)(n_i n_j + n_j n_i)
// The only cancelling quotient is the divided difference DD_m = (c_i^m - c_j^m) / (c_i - c_j).  With h = (ln c_i - ln c_j) / 2 it is
//   DD_m = m (c_i c_j)^((m-1)/2) sinhc(m h) / sinhc(h),     sinhc(y) = sinh(y) / y = 1 + y^2/6 + y^4/120 + ...
// which has no cancellation at all; the kernel evaluates that form (five terms of the even series: 2e-22 at |y| = 0.1) wherever
// max(|m h|, |h|) <= 0.1 and the plain quotient beyond, where it loses at most a factor 5 of the powers' own rounding: both are
// accurate on either side of the switch, exactly repeated eigenvalues (uniaxial loading, F = I) take the series at h = 0.
//
// Mapping and I/O are those of fefp.hpp, as shared text: tile_rows9_*.hpp (F in, PK1 out), tile_out81_roles.hpp and
// tile_out81_copyout.hpp (the tangent in rounds of 16 points through an out-tile transposed in LDS).  The epilogue between them
// differs: the owner lane stages F (9), S (6) and CC as a full 6x6 (36, so that the column lanes address it as row * 6 + lane
// constant); lane (point slot, column (k, L)) forms B[MJ] = sum_P CC[MJ][PL] F[k][P] (symmetric in MJ: 6 values) and the nine rows
// A[(i,J),(k,L)] = sum_M F[i][M] B[MJ] + delta_ik S[L][J].
#include "hyperelastic.hpp"

#include "fefp.hpp"   // the shared skeleton's constants (F2_PPR, F2_OUT, F2_NIT, F2_COEF, F2_LDS_PER_WAVE), DXM_SYM
#include "principal_axes.hpp"

namespace dxm {

constexpr int OG_REC = 51;   // F 0..8 | S 9..14 | CC 15..50; 102 dwords = 38 mod 64: the 16 owner lanes' 8 B writes fall on distinct bank pairs (19 l mod 32)
static_assert(F2_PPR * OG_REC <= F2_COEF, "the records fit the coefficient region of the FeFp layout: same LDS, two workgroups per CU");
static_assert(WAVE % F2_PPR == 0, "every round of a full tile is a full round");
constexpr int OG_SWEEPS = 5;   // cyclic Jacobi sweeps of the 3x3 eigenproblem (off-diagonal below 1e-16 |C| after 4 on every test family)

// (c_i^m - c_j^m) / (c_i - c_j) from c, ln c, c^(m-1), c^m of both (header comment)
__device__ __forceinline__ double divided_difference(double m, double ci, double cj, double li, double lj, double pwi, double pwj, double ui, double uj) {
  const double h = 0.5 * (li - lj), y = m * h;
  const double series = m * sqrt(pwi * pwj) * sinhc_series(y * y) * fast_rcp(sinhc_series(h * h));
  const double quotient = (ui - uj) * fast_rcp(ci - cj);
  return fmax(fabs(y), fabs(h)) <= 0.1 ? series : quotient;
}

__global__ void __launch_bounds__(BLOCK, DXM_FEFP_WGS)
ogden_kernel(const LawParams prm, const int64_t n, const double* __restrict__ Fin, double* __restrict__ s1, const int64_t ld,
             double* __restrict__ Pout, double* __restrict__ ct, BlockStats* __restrict__ stats) {
  __shared__ __attribute__((aligned(16))) double lds_all[WAVES_PER_BLOCK * F2_LDS_PER_WAVE];

  const int lane0 = threadIdx.x & (WAVE - 1);
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform: tile bookkeeping in scalar registers
  double* stage = lds_all + wid * F2_LDS_PER_WAVE;   // F in / PK1 out staging, reused as the tangent out-tile
  double* outt = stage;
  double2_t* stage2 = reinterpret_cast<double2_t*>(stage);

  const int64_t ntiles = (n + WAVE - 1) / WAVE;
  const int64_t tile_stride = (int64_t)gridDim.x * WAVES_PER_BLOCK;
  unsigned long long c_nan = 0;

  const double mu = prm.mu, kappa = prm.kappa;
  const double a = prm.c[OG_A], am2 = prm.c[OG_AM2], ma3 = prm.c[OG_MA3], m = prm.c[OG_M];
  const double SQ2 = 1.4142135623730950488;
  constexpr int TI[9] = {0, 1, 2, 0, 1, 0, 2, 1, 2};  // row index of entry t of the 9-vector
  constexpr int TJ[9] = {0, 1, 2, 1, 0, 2, 0, 2, 1};  // column index           (utils.py:168-190)
  constexpr bool OUT81_WHOLE_KIB = false;             // tile_out81_copyout.hpp: per-lane bounds only in the ragged branch
  int lane = lane0;

  for (int64_t tile = (int64_t)blockIdx.x * WAVES_PER_BLOCK + wid; tile < ntiles; tile += tile_stride) {
    const int64_t base = tile * WAVE;
    const int npts = (n - base) < WAVE ? (int)(n - base) : WAVE;
    // per-lane invariants are re-derived per tile from an opaque copy (fefp.hpp: hoisted, they cost registers over the whole body)
    asm volatile("" : "+v"(lane));
    lane &= WAVE - 1;
    const bool valid = lane < npts;
    const int64_t gi = base + lane;
#include "tile_out81_roles.hpp"
    // slot of the symmetric pair (P, LL) for P = 0, 1, 2
    const int vL0 = LL == 0 ? 0 : LL + 2, vL1 = LL == 1 ? 1 : LL + 3, vL2 = LL == 2 ? 2 : LL + 4;

    // ---- 1. F through LDS (64 x 9 doubles = 288 double2 per tile) -------------------------------------
    double F[9];
#include "tile_rows9_load.hpp"
    wave_lds_sync();
#include "tile_rows9_take.hpp"
    wave_lds_sync();

    // ---- 2. C = F^T F and its eigen-decomposition (cyclic Jacobi, fixed sweeps, registers only) ------------
    double J = det3(F);
    J = J > 0.0 ? J : __builtin_nan("");   // an inverted or flat point has no answer: NaN outputs, counted below
    double c0 = F[0] * F[0] + F[3] * F[3] + F[6] * F[6];
    double c1 = F[1] * F[1] + F[4] * F[4] + F[7] * F[7];
    double c2 = F[2] * F[2] + F[5] * F[5] + F[8] * F[8];
    double c01 = F[0] * F[1] + F[3] * F[4] + F[6] * F[7];
    double c02 = F[0] * F[2] + F[3] * F[5] + F[6] * F[8];
    double c12 = F[1] * F[2] + F[4] * F[5] + F[7] * F[8];
    double n0[3] = {1.0, 0.0, 0.0}, n1[3] = {0.0, 1.0, 0.0}, n2[3] = {0.0, 0.0, 1.0};   // eigenvector columns
#pragma unroll 1
    for (int sw = 0; sw < OG_SWEEPS; ++sw) {
      jacobi_rotate(c0, c1, c01, c02, c12, n0, n1);
      jacobi_rotate(c0, c2, c02, c01, c12, n0, n2);
      jacobi_rotate(c1, c2, c12, c01, c02, n1, n2);
    }

    // ---- 3. principal stresses and moduli ---------------------------------------------------------------
    double S6[6], CC[21];
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
      const double th01 = A0 * divided_difference(m, c0, c1, l0, l1, pw0, pw1, u0, u1) - q * i0 * i1;
      const double th02 = A0 * divided_difference(m, c0, c2, l0, l2, pw0, pw2, u0, u2) - q * i0 * i2;
      const double th12 = A0 * divided_difference(m, c1, c2, l1, l2, pw1, pw2, u1, u2) - q * i1 * i2;

      // back to the global axes: E_i = n_i n_i, G_ij = n_i n_j + n_j n_i as symmetric 6-vectors
      double E0[6], E1[6], E2[6], G01[6], G02[6], G12[6];
#pragma unroll
      for (int I = 0; I < 6; ++I) {
        const int M = SI[I], Jx = SJ[I];
        E0[I] = n0[M] * n0[Jx]; E1[I] = n1[M] * n1[Jx]; E2[I] = n2[M] * n2[Jx];
        G01[I] = n0[M] * n1[Jx] + n1[M] * n0[Jx];
        G02[I] = n0[M] * n2[Jx] + n2[M] * n0[Jx];
        G12[I] = n1[M] * n2[Jx] + n2[M] * n1[Jx];
      }
      double Si6[6];
#pragma unroll
      for (int I = 0; I < 6; ++I) {
        S6[I] = s0 * E0[I] + sp1 * E1[I] + s2 * E2[I];
        Si6[I] = t0 * E0[I] + t1 * E1[I] + t2 * E2[I];
      }
      if (valid) {
        stream_store<1>(s1 + 0 * ld + gi, Si6[0]);
        stream_store<1>(s1 + 1 * ld + gi, Si6[1]);
        stream_store<1>(s1 + 2 * ld + gi, Si6[2]);
        stream_store<1>(s1 + 3 * ld + gi, SQ2 * Si6[3]);
        stream_store<1>(s1 + 4 * ld + gi, SQ2 * Si6[4]);
        stream_store<1>(s1 + 5 * ld + gi, SQ2 * Si6[5]);
      }
      double X0[6], X1[6], X2[6];   // D E, then the th-weighted G in place
#pragma unroll
      for (int I = 0; I < 6; ++I) {
        X0[I] = D00 * E0[I] + D01 * E1[I] + D02 * E2[I];
        X1[I] = D01 * E0[I] + D11 * E1[I] + D12 * E2[I];
        X2[I] = D02 * E0[I] + D12 * E1[I] + D22 * E2[I];
      }
#pragma unroll
      for (int I = 0; I < 6; ++I)
#pragma unroll
        for (int Kx = I; Kx < 6; ++Kx)
          CC[TRI21_AT(I, Kx)] = E0[I] * X0[Kx] + E1[I] * X1[Kx] + E2[I] * X2[Kx] + th01 * G01[I] * G01[Kx] + th02 * G02[I] * G02[Kx] +
                    th12 * G12[I] * G12[Kx];
      // non-finite results (det F <= 0, a non-finite F): every output of the point is a combination of these with finite weights
      const double chk = ((s0 + sp1) + (s2 + D00)) + ((D11 + D22) + (D01 + D02)) + ((D12 + th01) + (th02 + th12));
      if (valid && !(fabs(chk) <= 1.79769313486231570e308)) ++c_nan;
    }

    // ---- 4. PK1 = F S through LDS, coalesced store --------------------------------------------------------
    {
      double P[9];
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int Jx = 0; Jx < 3; ++Jx)
          P[i * 3 + Jx] = F[i * 3] * S6[DXM_SYM(0, Jx)] + F[i * 3 + 1] * S6[DXM_SYM(1, Jx)] + F[i * 3 + 2] * S6[DXM_SYM(2, Jx)];
#include "tile_rows9_put.hpp"
    }
    wave_lds_sync();
#include "tile_rows9_store.hpp"
    wave_lds_sync();   // the out-tile below aliases the staging region

    // ---- 5. tangent, F2_PPR points per round ---------------------------------------------------------------
#pragma unroll 1
    for (int rd = 0; rd < (WAVE + F2_PPR - 1) / F2_PPR; ++rd) {
      const int p0 = rd * F2_PPR;                                   // first point of the round
      const int cnt = (WAVE - p0) < F2_PPR ? (WAVE - p0) : F2_PPR;  // points staged this round
      if (lane >= p0 && lane < p0 + cnt) {
        int ro = F2_OUT + (lane - p0) * OG_REC;   // opaque: every access below is base + small immediate (fefp.hpp)
        asm volatile("" : "+v"(ro));
        double* rec = stage + ro;
#pragma unroll
        for (int t = 0; t < 9; ++t) rec[t] = F[t];
#pragma unroll
        for (int I = 0; I < 6; ++I) rec[9 + I] = S6[I];
#pragma unroll
        for (int I = 0; I < 6; ++I)
#pragma unroll
          for (int Kx = 0; Kx < 6; ++Kx) rec[15 + I * 6 + Kx] = CC[I <= Kx ? TRI21_AT(I, Kx) : TRI21_AT(Kx, I)];
      }
      wave_lds_sync();
#pragma unroll 1
      for (int st = 0; st < F2_STEPS; ++st) {
        const int ql = st * 7 + ps;                                // point inside the round
        if (lane < 63 && ql < cnt) {
          int ro = F2_OUT + ql * OG_REC;
          asm volatile("" : "+v"(ro));
          const double* rec = stage + ro;
          // all LDS reads first (the out-tile writes below may alias them for the compiler)
          double fi[9];
#pragma unroll
          for (int t = 0; t < 9; ++t) fi[t] = rec[t];
          const double* cL0 = rec + 15 + vL0;
          const double* cL1 = rec + 15 + vL1;
          const double* cL2 = rec + 15 + vL2;
          const double sL0 = rec[9 + vL0], sL1 = rec[9 + vL1], sL2 = rec[9 + vL2];   // S[L][J], J = 0, 1, 2
          const double Fk0 = kk == 0 ? fi[0] : (kk == 1 ? fi[3] : fi[6]);             // F[k][P]
          const double Fk1 = kk == 0 ? fi[1] : (kk == 1 ? fi[4] : fi[7]);
          const double Fk2 = kk == 0 ? fi[2] : (kk == 1 ? fi[5] : fi[8]);
          double B[6];
#pragma unroll
          for (int I = 0; I < 6; ++I) B[I] = cL0[I * 6] * Fk0 + cL1[I * 6] * Fk1 + cL2[I * 6] * Fk2;
          double x[9];
#pragma unroll
          for (int r = 0; r < 9; ++r) {
            const int i = TI[r], Jx = TJ[r];
            const double sJ = Jx == 0 ? sL0 : (Jx == 1 ? sL1 : sL2);
            const double mi = i == 0 ? mk0 : (i == 1 ? mk1 : mk2);
            double t = mi * sJ;
            t += fi[i * 3] * B[DXM_SYM(0, Jx)];
            t += fi[i * 3 + 1] * B[DXM_SYM(1, Jx)];
            t += fi[i * 3 + 2] * B[DXM_SYM(2, Jx)];
            x[r] = t;
          }
          double* o = outt + ql * 81 + cc;
#pragma unroll
          for (int r = 0; r < 9; ++r) o[r * 9] = x[r];
        }
      }
      wave_lds_sync();
#include "tile_out81_copyout.hpp"
      wave_lds_sync();
    }
  }
  // the workgroup reduction borrows the first words of every wave's own region (the tile loop is over)
  store_block_stats(stats, 0, 0, c_nan, 0, reinterpret_cast<unsigned long long*>(lds_all), F2_LDS_PER_WAVE);
}

const void* ogden_kernel_fn() { return (const void*)ogden_kernel; }

void ogden_launch(int grid, hipStream_t st, const LawParams& prm, int64_t cnt, const double* F, double* s1, int64_t ld, double* P,
                  double* ct, BlockStats* bs) {
  hipLaunchKernelGGL(ogden_kernel, dim3(grid), dim3(BLOCK), 0, st, prm, cnt, F, s1, ld, P, ct, bs);
}

}  // namespace dxm
