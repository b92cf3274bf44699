// Logarithmic-strain J2 plasticity with linear hardening (gradient F (9), flux PK1 (9), 9x9 tangent dP/dF; internal state variables
// ElasticStrain (6) and EquivalentPlasticStrain (1), hidden state PlasticStrain (6)) for gfx950.
//
// The law is the reference's demos/mfront/finite_strain_elastoplasticity/LogarithmicStrainPlasticity.mfront, restated from its
// equations: the Miehe-Apel-Lambrecht construction around the small-strain radial return (Hooke, Mises, R(p) = s0 + H0 p, theta = 1).
// With C = F^T F = sum_i c_i n_i n_i^T, e_i = ln(c_i) / 2 and hats for components in the eigenbasis of C:
//   1. Hencky strain   E = sum e_i n_i n_i^T
//   2. radial return on the trial elastic strain E - Ep_n (Ep_n: the old logarithmic plastic strain), evaluated in the eigenbasis
//      (the law is isotropic): T^, dp, the flow direction n^ and the algorithmic moduli Ct = c1 1x1 + c2 I_sym + c3 n^ x n^
//   3. th_ij = ln[c_i, c_j] = 1 / (sqrt(c_i c_j) sinhc(e_i - e_j)), th_ii = 1 / c_i: no cancellation for any pair
//      S^_ij = th_ij T^_ij,   S = N S^ N^T,   PK1 = F S
//   4. g_akb = ln[c_a, c_k, c_b], the second divided difference, symmetric in its arguments (ls_gamma below)
//   5. CC^_ijkl = th_ij Ct^_ijkl th_kl + G^_ijkl, G^ the minor-symmetrised tensor of
//      G(H, K) = 2 sum_akb T^_ab g_akb (H_ak K_kb + K_ak H_kb):  G^_ijkl = d_jk M_ijl + d_ik M_jil + d_jl M_ijk + d_il M_jik,
//      M_abc = T^_ac g_abc.  In the basis B = (E_0, E_1, E_2, G_01, G_02, G_12), E_i = n_i n_i, G_ij = n_i n_j + n_j n_i, that is
//        [ii][ii] 4 T^_ii g_iii    [ii][ij] 2 T^_ij g_iij    [ij][ij] T^_jj g_ijj + T^_ii g_iij    [ij][ik] T^_jk g_012
//      and zero elsewhere; CC = sum_ab CC^[a][b] B_a B_b^T (21 entries).
//   6. from here on the kernel is Ogden's: A[(i,J),(k,L)] = delta_ik S_LJ + F_iM CC_MJPL F_kP.
// T is not coaxial with C once there is a plastic history, so all six components of T^ and n^ are carried.
//
// Mapping and I/O are those of hyperelastic.hip: one point per lane, tile_rows9_*.hpp (F in, PK1 out), tile_out81_roles.hpp and
// tile_out81_copyout.hpp (the tangent in rounds of 16 points through an out-tile transposed in LDS), the same records (F 9, S 6,
// CC as a full 6x6).  State: SoA, 8 B per lane, the slots of the Hosford law.
#include "log_strain.hpp"

#include "fefp.hpp"   // the shared skeleton's constants (F2_PPR, F2_OUT, F2_NIT, F2_COEF, F2_LDS_PER_WAVE), DXM_SYM
#include "principal_axes.hpp"

namespace dxm {

constexpr int LS_REC = 51;   // F 0..8 | S 9..14 | CC 15..50 (hyperelastic.hip: OG_REC, the same bank arithmetic)
static_assert(F2_PPR * LS_REC <= F2_COEF, "the records fit the coefficient region of the FeFp layout: same LDS");
static_assert(WAVE % F2_PPR == 0, "every round of a full tile is a full round");
constexpr int LS_SWEEPS = 5;   // cyclic Jacobi sweeps of the 3x3 eigenproblem (hyperelastic.hip)
constexpr double LS_GAMMA_SWITCH = 0.05;   // max |d| up to which ls_gamma takes its Taylor form
constexpr int LS_GAMMA_TERMS = 15;         // n = 0 .. 14: the first dropped term is below 136 x 0.05^15 / 17 = 2.4e-19

// ln[c_i, c_j] from the two values and y = (ln c_i - ln c_j) / 2 (header comment, step 3)
__device__ __forceinline__ double ls_theta(double ci, double cj, double y) {
  const double ey = exp(y);
  const double far = 0.5 * (ey - fast_rcp(ey)) / y;
  const double sc = fabs(y) <= 0.1 ? sinhc_series(y * y) : far;
  return fast_rcp(sqrt(ci * cj) * sc);
}

// ln[ca, ck, cb]: with m the mean and d = (c - m) / m, m^-2 sum_n (-1)^(n+1) / (n + 2) h_n(d) where max |d| <= LS_GAMMA_SWITCH
// (h_n: the complete homogeneous symmetric polynomial, h_n = e1 h_(n-1) - e2 h_(n-2) + e3 h_(n-3)); `far` beyond: the quotient of
// first differences over the largest gap, which the caller forms
__device__ __forceinline__ double ls_gamma(double ca, double ck, double cb, double far) {
  const double m = (ca + ck + cb) * (1.0 / 3.0);
  const double im = fast_rcp(m);
  const double d0 = (ca - m) * im, d1 = (ck - m) * im, d2 = (cb - m) * im;
  const double e1 = d0 + d1 + d2, e2 = d0 * d1 + d0 * d2 + d1 * d2, e3 = d0 * d1 * d2;
  double h3 = 0.0, h2 = 0.0, h1 = 1.0, acc = -0.5;
#pragma unroll
  for (int n = 1; n < LS_GAMMA_TERMS; ++n) {
    const double h = e1 * h1 - e2 * h2 + e3 * h3;
    acc += ((n & 1) ? 1.0 : -1.0) / (double)(n + 2) * h;
    h3 = h2; h2 = h1; h1 = h;
  }
  const bool small = fmax(fabs(d0), fmax(fabs(d1), fabs(d2))) <= LS_GAMMA_SWITCH;
  return small ? acc * im * im : far;
}

__global__ void __launch_bounds__(BLOCK, DXM_FEFP_WGS)
log_strain_kernel(const LawParams prm, const int64_t n, const double* __restrict__ Fin, const double* __restrict__ s0,
                  double* __restrict__ s1, const int64_t ld, double* __restrict__ Pout, double* __restrict__ ct,
                  BlockStats* __restrict__ stats) {
  __shared__ __attribute__((aligned(16))) double lds_all[WAVES_PER_BLOCK * F2_LDS_PER_WAVE];

  const int lane0 = threadIdx.x & (WAVE - 1);
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform: tile bookkeeping in scalar registers
  double* stage = lds_all + wid * F2_LDS_PER_WAVE;   // F in / PK1 out staging, reused as the tangent out-tile
  double* outt = stage;
  double2_t* stage2 = reinterpret_cast<double2_t*>(stage);

  const int64_t ntiles = (n + WAVE - 1) / WAVE;
  const int64_t tile_stride = (int64_t)gridDim.x * WAVES_PER_BLOCK;
  unsigned long long c_plastic = 0, c_nan = 0;

  const double lambda = prm.lambda, mu = prm.mu;
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

    // ---- 1. F through LDS (64 x 9 doubles = 288 double2 per tile); old state, SoA ------------------------------
    double F[9];
    double ep[6] = {0, 0, 0, 0, 0, 0}, p_n = 0.0;   // Mandel
#include "tile_rows9_load.hpp"
    if (valid) {
      p_n = stream_load<3>(s0 + (int64_t)LS_SLOT_P * ld + gi);
#pragma unroll
      for (int c = 0; c < 6; ++c) ep[c] = stream_load<3>(s0 + (int64_t)(LS_SLOT_EP + c) * ld + gi);
    }
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
    // F stays in the lane's own nine staging slots, which nobody writes before tile_rows9_put.hpp: it is read again for step 4
    // instead of being held in registers across step 3
    asm volatile("" ::: "memory");
    double n0[3] = {1.0, 0.0, 0.0}, n1[3] = {0.0, 1.0, 0.0}, n2[3] = {0.0, 0.0, 1.0};   // eigenvector columns
#pragma unroll 1
    for (int sw = 0; sw < LS_SWEEPS; ++sw) {
      jacobi_rotate(c0, c1, c01, c02, c12, n0, n1);
      jacobi_rotate(c0, c2, c02, c01, c12, n0, n2);
      jacobi_rotate(c1, c2, c12, c01, c02, n1, n2);
    }

    // ---- 3. the update in the eigenbasis, stresses and moduli ----------------------------------------------
    double S6[6], CC[21];
    {
      // B = (E_0, E_1, E_2, G_01, G_02, G_12) as symmetric 6-vectors of tensor components: X = sum_a X^_a B_a
      // (built twice, before the update and again for the rotation of the moduli: held across the divided differences and the
      // assembly of CC^ between the two, its 36 values do not fit 256 registers next to them)
      double B[6][6];
      auto build_basis = [&]() {
#pragma unroll
        for (int I = 0; I < 6; ++I) {
          const int M = SI[I], Jx = SJ[I];
          B[0][I] = n0[M] * n0[Jx]; B[1][I] = n1[M] * n1[Jx]; B[2][I] = n2[M] * n2[Jx];
          B[3][I] = n0[M] * n1[Jx] + n1[M] * n0[Jx];
          B[4][I] = n0[M] * n2[Jx] + n2[M] * n0[Jx];
          B[5][I] = n1[M] * n2[Jx] + n2[M] * n1[Jx];
        }
      };
      build_basis();
      const double nanJ = 0.0 * J;   // NaN with J, else zero
      const double l0 = log(c0), l1 = log(c1), l2 = log(c2);
      const double e0 = 0.5 * l0, e1 = 0.5 * l1, e2 = 0.5 * l2;
      // trial elastic strain in the eigenbasis: diag(e) - N^T Ep_n N; X^_ii = E_i : X, X^_ij = G_ij : X / 2 (off-diagonal tensor
      // components count twice; the state is Mandel: tensor component = Mandel / sqrt(2))
      double ee[6];
#pragma unroll
      for (int a = 0; a < 6; ++a) {
        double t = B[a][0] * ep[0] + B[a][1] * ep[1] + B[a][2] * ep[2] + SQ2 * (B[a][3] * ep[3] + B[a][4] * ep[4] + B[a][5] * ep[5]);
        ee[a] = a < 3 ? -t : -0.5 * t;
      }
      ee[0] += e0; ee[1] += e1; ee[2] += e2;
      const double tr = ee[0] + ee[1] + ee[2];
      const double third = tr * (1.0 / 3.0);
      double dv[6] = {ee[0] - third, ee[1] - third, ee[2] - third, ee[3], ee[4], ee[5]};
      const double seq = 2.0 * mu * sqrt(1.5 * (dv[0] * dv[0] + dv[1] * dv[1] + dv[2] * dv[2] + 2.0 * (dv[3] * dv[3] + dv[4] * dv[4] + dv[5] * dv[5])));
      const double ftr = seq - (prm.sig0 + prm.h1 * p_n);
      const bool plastic = ftr > 0.0;
      // closed-form radial return (IsotropicLinearHardeningPlasticity.mfront:49-77): n = 3/2 s / seq, dp = f / (H + 3 mu)
      const double gam = 1.0 / (prm.h1 + 3.0 * mu);
      const double dp = plastic ? ftr * gam : 0.0;
      const double iseq = plastic ? 1.0 / seq : 0.0;
      const double beta = dp * iseq;
      const double k1 = lambda + 2.0 * mu * mu * beta, k2 = 2.0 * mu - 6.0 * mu * mu * beta;
      const double k3 = plastic ? 4.0 * mu * mu * (beta - gam) : 0.0;
      double nf[6], Th[6];   // flow direction and stress, eigenbasis components
#pragma unroll
      for (int a = 0; a < 6; ++a) {
        nf[a] = 3.0 * mu * dv[a] * iseq;
        const double el = ee[a] - dp * nf[a];
        Th[a] = (a < 3 ? lambda * tr : 0.0) + 2.0 * mu * el;
      }
      const double p_new = p_n + dp;
      // new state, global axes, Mandel: Ep = Ep_n + dp N n^ N^T, eel = E - Ep
      {
        double chk = p_new;
#pragma unroll
        for (int I = 0; I < 6; ++I) {
          const double wI = I < 3 ? 1.0 : SQ2;
          double dE = 0.0, Eg = e0 * B[0][I] + e1 * B[1][I] + e2 * B[2][I];
#pragma unroll
          for (int a = 0; a < 6; ++a) dE += nf[a] * B[a][I];
          const double epn = ep[I] + wI * dp * dE;
          const double eel = wI * Eg - epn + nanJ;
          chk += eel;
          if (valid) {
            stream_store<1>(s1 + (int64_t)(LS_SLOT_EEL + I) * ld + gi, eel);
            stream_store<1>(s1 + (int64_t)(LS_SLOT_EP + I) * ld + gi, epn + nanJ);
          }
        }
        if (valid) stream_store<1>(s1 + (int64_t)LS_SLOT_P * ld + gi, p_new + nanJ);
        if (valid && !(fabs(chk) <= 1.79769313486231570e308)) ++c_nan;
        else if (valid && plastic) ++c_plastic;
      }

      // first divided differences (NaN with J: every output below is a combination of these)
      const double i0 = fast_rcp(c0), i1 = fast_rcp(c1), i2 = fast_rcp(c2);
      const double th01 = ls_theta(c0, c1, e0 - e1), th02 = ls_theta(c0, c2, e0 - e2), th12 = ls_theta(c1, c2, e1 - e2);
      const double th[6] = {i0 + nanJ, i1 + nanJ, i2 + nanJ, th01 + nanJ, th02 + nanJ, th12 + nanJ};
#pragma unroll
      for (int I = 0; I < 6; ++I) {
        double s = 0.0;
#pragma unroll
        for (int a = 0; a < 6; ++a) s += (th[a] * Th[a]) * B[a][I];
        S6[I] = s;
      }

      // second divided differences; beyond the switch the quotient over the largest gap of the sorted triple: for (i, i, j) that
      // is (1 / c_i - th_ij) / (c_i - c_j) whichever is larger
      const double g001 = ls_gamma(c0, c0, c1, (i0 - th01) / (c0 - c1)), g110 = ls_gamma(c1, c1, c0, (i1 - th01) / (c1 - c0));
      const double g002 = ls_gamma(c0, c0, c2, (i0 - th02) / (c0 - c2)), g220 = ls_gamma(c2, c2, c0, (i2 - th02) / (c2 - c0));
      const double g112 = ls_gamma(c1, c1, c2, (i1 - th12) / (c1 - c2)), g221 = ls_gamma(c2, c2, c1, (i2 - th12) / (c2 - c1));
      double g012;
      {
        const double a01 = fabs(c0 - c1), a02 = fabs(c0 - c2), a12 = fabs(c1 - c2);
        // the middle argument is the one that is not in the largest gap
        const double f1 = (th01 - th12) / (c0 - c2), f0 = (th01 - th02) / (c1 - c2), f2 = (th02 - th12) / (c0 - c1);
        const double far = (a02 >= a01 && a02 >= a12) ? f1 : (a12 >= a01 ? f0 : f2);
        g012 = ls_gamma(c0, c1, c2, far);
      }

      // CC^ = th Ct^ th + G^ (upper triangle in the basis B)
      double Ch[21];
#pragma unroll
      for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = a; b < 6; ++b) {
          double v = k3 * nf[a] * nf[b];
          if (a < 3 && b < 3) v += k1;
          if (a == b) v += a < 3 ? k2 : 0.5 * k2;
          Ch[TRI21_AT(a, b)] = th[a] * th[b] * v;
        }
      Ch[TRI21_AT(0, 0)] -= 2.0 * Th[0] * i0 * i0;   // 4 T^_ii g_iii, g_iii = -1 / (2 c_i^2)
      Ch[TRI21_AT(1, 1)] -= 2.0 * Th[1] * i1 * i1;
      Ch[TRI21_AT(2, 2)] -= 2.0 * Th[2] * i2 * i2;
      Ch[TRI21_AT(0, 3)] += 2.0 * Th[3] * g001; Ch[TRI21_AT(1, 3)] += 2.0 * Th[3] * g110;
      Ch[TRI21_AT(0, 4)] += 2.0 * Th[4] * g002; Ch[TRI21_AT(2, 4)] += 2.0 * Th[4] * g220;
      Ch[TRI21_AT(1, 5)] += 2.0 * Th[5] * g112; Ch[TRI21_AT(2, 5)] += 2.0 * Th[5] * g221;
      Ch[TRI21_AT(3, 3)] += Th[1] * g110 + Th[0] * g001;
      Ch[TRI21_AT(4, 4)] += Th[2] * g220 + Th[0] * g002;
      Ch[TRI21_AT(5, 5)] += Th[2] * g221 + Th[1] * g112;
      Ch[TRI21_AT(3, 4)] += Th[5] * g012; Ch[TRI21_AT(3, 5)] += Th[4] * g012; Ch[TRI21_AT(4, 5)] += Th[3] * g012;

      // back to the global axes, column by column: x = CC^ B[.][K], CC[I][K] = sum_a B[a][I] x[a]; the basis again, from
      // opaque copies of the eigenvectors (the compiler would otherwise keep the first one)
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        asm volatile("" : "+v"(n0[k]));
        asm volatile("" : "+v"(n1[k]));
        asm volatile("" : "+v"(n2[k]));
      }
      build_basis();
#pragma unroll
      for (int Kx = 0; Kx < 6; ++Kx) {
        double x[6];
#pragma unroll
        for (int a = 0; a < 6; ++a) {
          double t = 0.0;
#pragma unroll
          for (int b = 0; b < 6; ++b) t += Ch[a <= b ? TRI21_AT(a, b) : TRI21_AT(b, a)] * B[b][Kx];
          x[a] = t;
        }
#pragma unroll
        for (int I = 0; I <= Kx; ++I) {
          double t = 0.0;
#pragma unroll
          for (int a = 0; a < 6; ++a) t += B[a][I] * x[a];
          CC[TRI21_AT(I, Kx)] = t;
        }
      }
    }

    // ---- 4. PK1 = F S through LDS, coalesced store --------------------------------------------------------
    asm volatile("" ::: "memory");
#include "tile_rows9_take.hpp"
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

    // ---- 5. tangent, F2_PPR points per round (hyperelastic.hip, step 5) -------------------------------------
#pragma unroll 1
    for (int rd = 0; rd < (WAVE + F2_PPR - 1) / F2_PPR; ++rd) {
      const int p0 = rd * F2_PPR;                                   // first point of the round
      const int cnt = (WAVE - p0) < F2_PPR ? (WAVE - p0) : F2_PPR;  // points staged this round
      if (lane >= p0 && lane < p0 + cnt) {
        int ro = F2_OUT + (lane - p0) * LS_REC;   // opaque: every access below is base + small immediate (fefp.hpp)
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
          int ro = F2_OUT + ql * LS_REC;
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
          double Bv[6];
#pragma unroll
          for (int I = 0; I < 6; ++I) Bv[I] = cL0[I * 6] * Fk0 + cL1[I * 6] * Fk1 + cL2[I * 6] * Fk2;
          double x[9];
#pragma unroll
          for (int r = 0; r < 9; ++r) {
            const int i = TI[r], Jx = TJ[r];
            const double sJ = Jx == 0 ? sL0 : (Jx == 1 ? sL1 : sL2);
            const double mi = i == 0 ? mk0 : (i == 1 ? mk1 : mk2);
            double t = mi * sJ;
            t += fi[i * 3] * Bv[DXM_SYM(0, Jx)];
            t += fi[i * 3 + 1] * Bv[DXM_SYM(1, Jx)];
            t += fi[i * 3 + 2] * Bv[DXM_SYM(2, Jx)];
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
  store_block_stats(stats, c_plastic, 0, c_nan, 0, reinterpret_cast<unsigned long long*>(lds_all), F2_LDS_PER_WAVE);
}

const void* log_strain_kernel_fn() { return (const void*)log_strain_kernel; }

void log_strain_launch(int grid, hipStream_t st, const LawParams& prm, int64_t cnt, const double* F, const double* s0, double* s1,
                       int64_t ld, double* P, double* ct, BlockStats* bs) {
  hipLaunchKernelGGL(log_strain_kernel, dim3(grid), dim3(BLOCK), 0, st, prm, cnt, F, s0, s1, ld, P, ct, bs);
}

}  // namespace dxm
