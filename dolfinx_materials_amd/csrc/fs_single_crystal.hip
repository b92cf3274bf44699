// Finite-strain FCC single-crystal viscoplasticity (the reference's FCCMericCailletaudFiniteStrainSingleCrystalViscoPlasticity
// behaviour, restated from its equations) with a material frame per handle or per Gauss point, for gfx950.  Gradient: F (9), flux:
// PK1 (9), 9-vectors in the order [11, 22, 33, 12, 21, 13, 31, 23, 32] (TI / TJ); the tangent dP/dF is 81 independent numbers.
//
// The law, in the material frame (rows of R = material axes; F_m = R F R^T, P = R^T P_m R, the tangent rotated accordingly): cubic
// stiffness D, twelve {111}<01-1> systems numbered as in single_crystal.hpp with mu_i = m_i x n_i (unit direction, unit normal, NOT
// symmetrised), unknowns the twelve slip increments dg of an implicit step (theta = 1) of length dt:
//   Fe_tr = F Fp_n^-1,  A = I - sum dg_i mu_i,  dFp^-1 = A / det(A)^(1/3),  Fe = Fe_tr dFp^-1,  G = Fp_n^-1 dFp^-1,
//   Eel = (Fe^T Fe - I) / 2,  S = D : Eel,  M = (I + 2 Eel) S,  tau_i = M : mu_i,
//   r_i = tau0 + Q sum_j h_ij (1 - exp(-b (p_j + |dg_j|))),   da_i = (dg_i - d a_i |dg_i|) / (1 + d |dg_i|),   x_i = C (a_i + da_i),
//   f_i = max(|tau_i - x_i| - r_i, 0),  s_i = sgn(tau_i - x_i),   residual  fg_i = dg_i - dt (f_i / K)^n s_i,
//   J_ij = delta_ij + w_i (-d tau_i / d dg_j + C dda_i delta_ij + s_i Q b h_ij exp(-b (p_j + |dg_j|)) sgn(dg_j)),  w_i = dt n (f_i / K)^n / f_i,
//   d dFp^-1 / d dg_j = det(A)^(-1/3) (-mu_j + tr(A^-1 mu_j) A / 3);  for a variation dFe of Fe and dG of G:
//   dEel = sym(Fe^T dFe),  dS = D : dEel,  dM = 2 dEel S + (I + 2 Eel) dS,  dP = det(Fp_n) ((dFe S + Fe dS) G^T + Fe S dG^T),
//   P_m = det(Fp_n) Fe S G^T,   dP/dF = dP/dF|dg - sum_j (dP / d dg_j) X_j,   X = J^-1 (d fg / d F),  d fg_i / d F = -w_i d tau_i / d F;
//   state: g += dg, p += |dg|, a += da, Fp = dFp Fp_n.
// Newton from dg = 0; a step is halved while the new max |fg| is not finite or larger than the old one (a halving counts as an
// iteration); stop at max |fg_i| <= rtol, then apply the correction of the factorisation the tangent needs anyway: the tangent is
// formed at the iterate the convergence test saw, stress and state after the correction.  A point at the cap writes its elastic
// trial response (St-Venant-Kirchhoff about Fp_n) and keeps the state bits it read.
//
// Mapping.  Around the Newton: one thread per point, one wave per tile of 64, F in and PK1 out by tile_rows9_*.hpp, the tangent in
// four rounds of 16 points through an out-tile in LDS that leaves by tile_out81_copyout.hpp.  The Newton itself, inside a tangent
// round: ONE LANE PER SLIP SYSTEM, 16 lanes per point (12 working), four yielded points per Newton round.  A lane holds its row
// of [J | fg | 9 tangent right-hand sides] (22 doubles); the variations of M it needs are formed once per row (lane j that of dg_j,
// lane u < 9 that of component u of F) and exchanged through LDS; Gauss-Jordan with partial pivoting as in single_crystal.hip.
// Wave-private LDS only, no s_barrier inside the tile loop.
#include "fs_single_crystal.hpp"

#include "fefp.hpp"   // F2_PPR, F2_NIT of tile_out81_copyout.hpp, det3

namespace dxm {

static_assert(F2_PPR == FX_PPR && F2_NIT * 2 * WAVE == FX_OUT, "the out-tile is the one tile_out81_copyout.hpp reads");

__device__ __forceinline__ double fx_push(double v, int dst_lane) {   // lane dst_lane receives v (a permutation within the wave)
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_ds_permute(dst_lane << 2, lo);
  hi = __builtin_amdgcn_ds_permute(dst_lane << 2, hi);
  return __hiloint2double(hi, lo);
}

// 3x3 tensors are row-major double[9]; symmetric ones the 6-vector [11, 22, 33, 12, 13, 23] addressed by DXM_SYM
__device__ __forceinline__ void fx_mul(const double* a, const double* b, double* c) {   // c = a b
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) c[i * 3 + j] = a[i * 3] * b[j] + a[i * 3 + 1] * b[3 + j] + a[i * 3 + 2] * b[6 + j];
}
__device__ __forceinline__ void fx_mul_nt(const double* a, const double* b, double* c) {   // c = a b^T
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) c[i * 3 + j] = a[i * 3] * b[j * 3] + a[i * 3 + 1] * b[j * 3 + 1] + a[i * 3 + 2] * b[j * 3 + 2];
}
__device__ __forceinline__ void fx_mul_ns(const double* a, const double* s6, double* c) {   // c = a s, s symmetric
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      c[i * 3 + j] = a[i * 3] * s6[DXM_SYM(0, j)] + a[i * 3 + 1] * s6[DXM_SYM(1, j)] + a[i * 3 + 2] * s6[DXM_SYM(2, j)];
}
__device__ __forceinline__ void fx_adj(const double* a, double* adj) {   // a adj = det(a) I
  adj[0] = a[4] * a[8] - a[5] * a[7]; adj[1] = a[2] * a[7] - a[1] * a[8]; adj[2] = a[1] * a[5] - a[2] * a[4];
  adj[3] = a[5] * a[6] - a[3] * a[8]; adj[4] = a[0] * a[8] - a[2] * a[6]; adj[5] = a[2] * a[3] - a[0] * a[5];
  adj[6] = a[3] * a[7] - a[4] * a[6]; adj[7] = a[1] * a[6] - a[0] * a[7]; adj[8] = a[0] * a[4] - a[1] * a[3];
}

// the kinematics of one iterate
struct FxKin {
  double A[9], a3;   // I - sum dg mu, det(A)^(-1/3)
  double Fe[9], G[9];
  double CE[6], S[6];   // Fe^T Fe = I + 2 Eel, D : Eel
};

__device__ __forceinline__ void fx_stiff(const FxParams& sp, const double* e6, double* s6) {
  const double tr = e6[0] + e6[1] + e6[2];
#pragma unroll
  for (int i = 0; i < 3; ++i) s6[i] = (sp.c11 - sp.c12) * e6[i] + sp.c12 * tr;
#pragma unroll
  for (int i = 3; i < 6; ++i) s6[i] = sp.g2 * e6[i];
}

// from k.A: everything else of the iterate
__device__ __forceinline__ void fx_kinematics(const FxParams& sp, const double* fetr, const double* fpi, FxKin& k) {
  k.a3 = 1.0 / cbrt(det3(k.A));
  double dp[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) dp[t] = k.a3 * k.A[t];
  fx_mul(fetr, dp, k.Fe);
  fx_mul(fpi, dp, k.G);
  double e6[6];
#pragma unroll
  for (int I = 0; I < 6; ++I) {
    const int i = SI[I], j = SJ[I];
    k.CE[I] = k.Fe[i] * k.Fe[j] + k.Fe[3 + i] * k.Fe[3 + j] + k.Fe[6 + i] * k.Fe[6 + j];
    e6[I] = 0.5 * (k.CE[I] - (I < 3 ? 1.0 : 0.0));
  }
  fx_stiff(sp, e6, k.S);
}

// dEel = sym(Fe^T dFe) and dS = D : dEel of a variation dFe
__device__ __forceinline__ void fx_dstrain(const FxParams& sp, const FxKin& k, const double* dFe, double* dE, double* dS) {
#pragma unroll
  for (int I = 0; I < 6; ++I) {
    const int i = SI[I], j = SJ[I];
    const double x = k.Fe[i] * dFe[j] + k.Fe[3 + i] * dFe[3 + j] + k.Fe[6 + i] * dFe[6 + j];
    const double y = k.Fe[j] * dFe[i] + k.Fe[3 + j] * dFe[3 + i] + k.Fe[6 + j] * dFe[6 + i];
    dE[I] = 0.5 * (x + y);
  }
  fx_stiff(sp, dE, dS);
}

// dM = 2 dEel S + (I + 2 Eel) dS
__device__ __forceinline__ void fx_dM(const FxParams& sp, const FxKin& k, const double* dFe, double* dM) {
  double dE[6], dS[6];
  fx_dstrain(sp, k, dFe, dE, dS);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double t = 0.0;
#pragma unroll
      for (int m = 0; m < 3; ++m) t += 2.0 * dE[DXM_SYM(i, m)] * k.S[DXM_SYM(m, j)] + k.CE[DXM_SYM(i, m)] * dS[DXM_SYM(m, j)];
      dM[i * 3 + j] = t;
    }
}

// dP = c ((dFe S + Fe dS) G^T + Fe S dG^T); dG null: the variation leaves G alone
__device__ __forceinline__ void fx_dP(const FxParams& sp, const FxKin& k, double c, const double* dFe, const double* dG, double* dP) {
  double dE[6], dS[6], x[9], y[9];
  fx_dstrain(sp, k, dFe, dE, dS);
  fx_mul_ns(dFe, k.S, x);
  fx_mul_ns(k.Fe, dS, y);
#pragma unroll
  for (int t = 0; t < 9; ++t) x[t] += y[t];
  fx_mul_nt(x, k.G, dP);
  if (dG) {
    fx_mul_ns(k.Fe, k.S, x);
    fx_mul_nt(x, dG, y);
#pragma unroll
    for (int t = 0; t < 9; ++t) dP[t] += y[t];
  }
#pragma unroll
  for (int t = 0; t < 9; ++t) dP[t] *= c;
}

template <int FRAME>
__global__ void __launch_bounds__(FX_BLOCK) __attribute__((amdgpu_waves_per_eu(1, 1)))
fs_single_crystal_kernel(const LawParams prm, const FxParams sp, const int64_t n, const double* __restrict__ Fin, const Frame9 uniform,
                         const double* __restrict__ frames, const int64_t ldf, const double* __restrict__ s0, double* __restrict__ s1,
                         const int64_t ld, double* __restrict__ Pout, double* __restrict__ ct, BlockStats* __restrict__ stats) {
  __shared__ __attribute__((aligned(16))) double lds_all[FX_WAVES * FX_LDS_PER_WAVE];
  __shared__ double sys_tab[16 * FX_SYS];   // per slip system: mu_i (9, row-major), row i of Q h (12); rows 12..15 are zero
  __shared__ unsigned long long red[4 * FX_WAVES];
  static_assert(FX_LDS_BYTES == sizeof(lds_all) + sizeof(sys_tab) + sizeof(red), "fs_single_crystal.hpp states the LDS of the kernel");

  int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  double* outt = lds_all + wid * FX_LDS_PER_WAVE;   // the out-tile of a tangent round: FX_PPR x 81 in output order
  double* stage = outt + FX_OUT;                    // F in / PK1 out
  double* park = stage + FX_STAGE;                  // per point: Fe_tr (9), Fp_n^-1 (9), det Fp_n
  double* xch = park + WAVE * FX_PARK;              // per Newton row: 21 exchanged 3x3 tensors
  double* hand = xch + 4 * FX_XCH;                  // per point of a tangent round: the twelve slip increments, status, iterations
  double2_t* stage2 = reinterpret_cast<double2_t*>(stage);

  const int64_t ntiles = (n + WAVE - 1) / WAVE;
  const int64_t tile_stride = (int64_t)gridDim.x * FX_WAVES;
  unsigned long long c_plastic = 0, c_notconv = 0, c_nan = 0, c_maxit = 0;

  constexpr double INV_SQRT6 = 0.40824829046386301637;
  constexpr int RM[9] = {0, 4, 8, 1, 3, 2, 6, 5, 7};    // row-major index of entry t of a 9-vector
  constexpr int VEC[9] = {0, 3, 5, 4, 1, 7, 6, 8, 2};   // entry of the 9-vector of row-major index r
  constexpr bool OUT81_WHOLE_KIB = false;               // tile_out81_copyout.hpp: per-lane bounds only in the ragged branch

  const int li = threadIdx.x & 15;
  const int grp = (threadIdx.x >> 4) & 3;
  if (threadIdx.x < 16) {
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      double v = 0.0;
#pragma unroll
      for (int i = 0; i < SC_NSYS; ++i) v = (li == i) ? INV_SQRT6 * (SC.s[i][t / 3] * SC.n[i][t % 3]) : v;
      sys_tab[li * FX_SYS + t] = v;
    }
#pragma unroll
    for (int j = 0; j < SC_NSYS; ++j) {
      double q = 0.0;
#pragma unroll
      for (int i = 0; i < SC_NSYS; ++i) q = (li == i) ? sp.qh[SC.cls[i][j]] : q;
      sys_tab[li * FX_SYS + 9 + j] = q;
    }
  }
  __syncthreads();   // once, ahead of the tile loop
  // read through an opaque copy of this address wherever they are used: hoisted out of the Newton loop the 21 doubles cost 42 VGPRs
  const double* const sys_row = sys_tab + li * FX_SYS;
#define FX_SYS_ROW(name)        \
  const double* name = sys_row; \
  asm volatile("" : "+v"(name))

  // A = I - sum_j dg_j mu_j from the increment of every lane of the 16-lane row
  auto gather_A = [&](double dgv, double* A) {
#pragma unroll
    for (int t = 0; t < 9; ++t) A[t] = (t % 4 == 0) ? 1.0 : 0.0;
#pragma unroll
    for (int j = 0; j < SC_NSYS; ++j) {
      const double dgj = __shfl(dgv, j, 16);
#pragma unroll
      for (int t = 0; t < 9; ++t)
        if (SC.s[j][t / 3] * SC.n[j][t % 3] != 0) A[t] -= (INV_SQRT6 * (SC.s[j][t / 3] * SC.n[j][t % 3])) * dgj;
    }
  };

  for (int64_t tile = (int64_t)blockIdx.x * FX_WAVES + wid; tile < ntiles; tile += tile_stride) {
    const int64_t base = tile * WAVE;
    const int npts = (n - base) < WAVE ? (int)(n - base) : WAVE;
    asm volatile("" : "+v"(lane));
    lane &= WAVE - 1;
    const bool valid = lane < npts;

    // ---- 1. F through LDS; the frame of the point --------------------------------------------------------------------
    int sl = lane;   // the lane, as an opaque copy per phase: addresses and loaded values of one phase are not kept for the next
    double R[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    auto load_frame = [&]() {
      if constexpr (FRAME == OR_FRAME_FIELD) {
#pragma unroll
        for (int k = 0; k < 9; ++k)   // both branches assign: nothing of an earlier phase stays live
          R[k / 3][k % 3] = valid ? stream_load<3>(frames + ((int64_t)k * ldf + base) + (unsigned)sl) : (k % 4 == 0 ? 1.0 : 0.0);
      } else if constexpr (FRAME == OR_FRAME_UNIFORM) {
#pragma unroll
        for (int k = 0; k < 9; ++k) {
          double r = uniform.r[k];
          asm volatile("" : "+v"(r));
          R[k / 3][k % 3] = r;
        }
      }
    };
#include "tile_rows9_load.hpp"
    load_frame();
    wave_lds_sync();

    auto load0 = [&](int slot) { return stream_load<3>(s0 + ((int64_t)slot * ld + base) + (unsigned)sl); };
    auto store1 = [&](int slot, double v) { stream_store<1>(s1 + ((int64_t)slot * ld + base) + (unsigned)sl, v); };

    int po = lane * FX_PARK;   // opaque: every access is base + small immediate
    asm volatile("" : "+v"(po));
    double* mypark = park + po;

    // ---- 2. trial state: Fe_tr = R F R^T Fp_n^-1, resolved shear stresses against the hardened thresholds at dg = 0 -----
    bool plastic = false;
    {
      double F[9];
#include "tile_rows9_take.hpp"
      if constexpr (FRAME != OR_FRAME_NONE) {
        double t[9];
        fx_mul(&R[0][0], F, t);
        fx_mul_nt(t, &R[0][0], F);
      }
      double fpn[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
      if (valid) {
#pragma unroll
        for (int t = 0; t < 9; ++t) fpn[RM[t]] = load0(FX_SLOT_FP + t);
      }
      FxKin k;
      double fpi[9], fetr[9];
      fx_adj(fpn, fpi);
      const double c = fpn[0] * fpi[0] + fpn[1] * fpi[3] + fpn[2] * fpi[6];
      const double ic = 1.0 / c;
#pragma unroll
      for (int t = 0; t < 9; ++t) fpi[t] *= ic;
      fx_mul(F, fpi, fetr);
#pragma unroll
      for (int t = 0; t < 9; ++t) { mypark[t] = fetr[t]; mypark[9 + t] = fpi[t]; }
      mypark[18] = c;
#pragma unroll
      for (int t = 0; t < 9; ++t) k.A[t] = (t % 4 == 0) ? 1.0 : 0.0;
      fx_kinematics(sp, fetr, fpi, k);
      double M[9];
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
          M[i * 3 + j] = k.CE[DXM_SYM(i, 0)] * k.S[DXM_SYM(0, j)] + k.CE[DXM_SYM(i, 1)] * k.S[DXM_SYM(1, j)] + k.CE[DXM_SYM(i, 2)] * k.S[DXM_SYM(2, j)];
      __builtin_amdgcn_sched_barrier(0);
      double om[SC_NSYS];   // 1 - exp(-b p_j)
#pragma unroll
      for (int j = 0; j < SC_NSYS; ++j) {
        const double p = valid ? load0(FX_SLOT_P + j) : 0.0;
        om[j] = 1.0 - exp(-sp.b * p);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll 1
      for (int i = 0; i < SC_NSYS; ++i) {
        const double* sr = sys_tab + i * FX_SYS;
        double tau = sr[0] * M[0];
#pragma unroll
        for (int t = 1; t < 9; ++t) tau += sr[t] * M[t];
        double r = sp.tau0;
#pragma unroll
        for (int j = 0; j < SC_NSYS; ++j) r += sr[9 + j] * om[j];
        const double a = valid ? load0(FX_SLOT_A + i) : 0.0;
        plastic = plastic || (fabs(tau - sp.C * a) - r > 0.0);
      }
      plastic = plastic && valid;
    }
    wave_lds_sync();

    const unsigned long long pm = __ballot(plastic);

    // ---- 3. four tangent rounds of 16 points: Newton rounds of its yielded points, then every point of the round -----------
#pragma unroll 1
    for (int q = 0; q < WAVE / FX_PPR; ++q) {
      const int p0 = q * FX_PPR;
      if (p0 >= npts) break;   // a ragged tile: nothing of this round exists
      const int cnt = FX_PPR;
      const bool mine = (lane >> 4) == q;
      const unsigned pmq = (unsigned)(pm >> p0) & 0xffffu;
      const int nyield = __popc(pmq);
      const int rank = __popc(pmq & ((1u << (lane & 15)) - 1u));

      for (int r0 = 0; r0 < nyield; r0 += 4) {
        int owner = -1;   // the tile-local point of this 16-lane row
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const unsigned long long mk = __ballot(plastic && mine && rank == r0 + k);
          const int o = mk ? __ffsll((long long)mk) - 1 : -1;
          owner = (grp == k) ? o : owner;
        }
        const bool work = owner >= 0 && li < SC_NSYS;
        const int ow = owner < 0 ? 0 : owner;
        const double p_i = work ? s0[(int64_t)(FX_SLOT_P + li) * ld + base + ow] : 0.0;
        const double a_i = work ? s0[(int64_t)(FX_SLOT_A + li) * ld + base + ow] : 0.0;
        int pko = ow * FX_PARK;
        asm volatile("" : "+v"(pko));
        const double* pk = park + pko;   // Fe_tr, Fp_n^-1, det Fp_n of the row's point
        int xo = grp * FX_XCH;
        asm volatile("" : "+v"(xo));
        double* xr = xch + xo;

        // everything of an iterate that does not depend on the lane's own system
        auto iterate = [&](double dgv, FxKin& k) {
          gather_A(dgv, k.A);
          double fetr[9], fpi[9];
#pragma unroll
          for (int t = 0; t < 9; ++t) { fetr[t] = pk[t]; fpi[t] = pk[9 + t]; }
          fx_kinematics(sp, fetr, fpi, k);
        };
        // the variation of dFp^-1 with the lane's own slip increment, and those of Fe and G that follow
        auto slip_variation = [&](const FxKin& k, const double* mu, double* dFe, double* dG) {
          double adj[9];
          fx_adj(k.A, adj);
          double tr = 0.0;   // tr(adj(A) mu)
#pragma unroll
          for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) tr += adj[a * 3 + b] * mu[b * 3 + a];
          // tr(A^-1 mu) / 3 = tr(adj mu) a3^3 / 3 (det(A) = a3^-3)
          const double h = tr * (k.a3 * k.a3 * k.a3) * (1.0 / 3.0);
          double ddp[9], fetr[9], fpi[9];
#pragma unroll
          for (int t = 0; t < 9; ++t) { ddp[t] = k.a3 * (h * k.A[t] - mu[t]); fetr[t] = pk[t]; fpi[t] = pk[9 + t]; }
          fx_mul(fetr, ddp, dFe);
          fx_mul(fpi, ddp, dG);
        };
        // the variation of Fe with component li (< 9) of the material-frame F: row TI of dFe is row TJ of G
        auto f_variation = [&](const FxKin& k, double* dFe) {
          const int kk = (0x26124 >> (2 * (li < 9 ? li : 0))) & 3;
          const int LL = (0x18864 >> (2 * (li < 9 ? li : 0))) & 3;
          // by 0 / 1 factors: a select between the rows becomes an indexed access to a copy of G in scratch memory
          const double l0 = LL == 0 ? 1.0 : 0.0, l1 = LL == 1 ? 1.0 : 0.0, l2 = LL == 2 ? 1.0 : 0.0;
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const double g = l0 * k.G[c] + l1 * k.G[3 + c] + l2 * k.G[6 + c];
#pragma unroll
            for (int r = 0; r < 3; ++r) dFe[r * 3 + c] = (kk == r && li < 9) ? g : 0.0;
          }
        };

        double dgi = 0.0, step = 0.0, dg_acc = 0.0, old = __builtin_inf();
        double X9[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // row i of J^-1 (d fg / dF) at the accepted iterate
        unsigned it = 0;
        int st_g = 0;
        bool done = owner < 0;
        const int sh = lane & 48;
        for (;;) {
          const double adg = fabs(dgi);
          const double Ei = exp(-sp.b * (p_i + adg));
          double row[22];   // my row of [J | fg | d fg / dF]; first the hardening part of J_ij without its factor s_i b
          double tau, r = sp.tau0;
          {
            FxKin k;
            iterate(dgi, k);
            double mu[9];
            {
              FX_SYS_ROW(sys0);
#pragma unroll
              for (int t = 0; t < 9; ++t) mu[t] = sys0[t];
            }
            // tau_i = mu_i : (CE S)
            tau = 0.0;
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
              for (int b = 0; b < 3; ++b)
                tau += mu[a * 3 + b] * (k.CE[DXM_SYM(a, 0)] * k.S[DXM_SYM(0, b)] + k.CE[DXM_SYM(a, 1)] * k.S[DXM_SYM(1, b)] +
                                        k.CE[DXM_SYM(a, 2)] * k.S[DXM_SYM(2, b)]);
            // the variations of M: mine with dg_li, and with component li of F
            double dFe[9], dG[9], dM[9];
            slip_variation(k, mu, dFe, dG);
            fx_dM(sp, k, dFe, dM);
#pragma unroll
            for (int t = 0; t < 9; ++t) xr[li * 9 + t] = dM[t];
            f_variation(k, dFe);
            fx_dM(sp, k, dFe, dM);
            if (li < 9) {
#pragma unroll
              for (int t = 0; t < 9; ++t) xr[(12 + li) * 9 + t] = dM[t];
            }
          }
          wave_lds_sync();
          double mu[9];
          {
            FX_SYS_ROW(sys1);
#pragma unroll
            for (int t = 0; t < 9; ++t) mu[t] = sys1[t];
#pragma unroll
            for (int j = 0; j < SC_NSYS; ++j) {
              const double dgj = __shfl(dgi, j, 16), Ej = __shfl(Ei, j, 16);
              const double qh = sys1[9 + j];
              r += qh * (1.0 - Ej);
              row[j] = qh * Ej * (dgj > 0.0 ? 1.0 : -1.0);
            }
          }
          const double sgi = dgi > 0.0 ? 1.0 : -1.0;
          const double den = 1.0 / (1.0 + sp.d * adg);
          const double da = (dgi - sp.d * a_i * adg) * den;
          const double y = tau - sp.C * (a_i + da);
          const double s = y > 0.0 ? 1.0 : -1.0;
          const double f = work ? fmax(fabs(y) - r, 0.0) : 0.0;
          const double fk = f > 0.0 ? exp(sp.n * log(f / sp.K)) : 0.0;   // (f / K)^n
          const double fg = work ? dgi - sp.dt * fk * s : 0.0;
          const bool bad = ((__ballot(!(fabs(fg) <= old)) >> sh) & 0xffffull) != 0;
          const bool conv = ((__ballot(!(fabs(fg) <= prm.rtol)) >> sh) & 0xffffull) == 0;
          double fmx = fabs(fg);
#pragma unroll
          for (int m = 8; m > 0; m >>= 1) fmx = fmax(fmx, __shfl_xor(fmx, m, 16));

          const double w = f > 0.0 ? sp.dt * (sp.n * fk / f) : 0.0;
          const double dda = (1.0 - sp.d * a_i * sgi) * den * den;
#pragma unroll
          for (int j = 0; j < SC_NSYS; ++j) {
            double dtau = 0.0;   // d tau_i / d dg_j = mu_i : dM_j
#pragma unroll
            for (int t = 0; t < 9; ++t) dtau += mu[t] * xr[j * 9 + t];
            double t = s * sp.b * row[j] - dtau;
            if (li == j) t += sp.C * dda;
            row[j] = (li == j ? 1.0 : 0.0) + w * t;
            __builtin_amdgcn_sched_barrier(0);   // column after column: issued together the 189 LDS reads cost the registers
          }
          row[12] = fg;
#pragma unroll
          for (int u = 0; u < 9; ++u) {
            double dtau = 0.0;
#pragma unroll
            for (int t = 0; t < 9; ++t) dtau += mu[t] * xr[(12 + u) * 9 + t];
            row[13 + u] = -w * dtau;
            __builtin_amdgcn_sched_barrier(0);
          }
          if (!work) {   // an idle row: the unit row of its own column, nothing on the right
#pragma unroll
            for (int k = 0; k < 22; ++k) row[k] = (k < SC_NSYS && k == li) ? 1.0 : 0.0;
          }
          wave_lds_sync();   // the exchanged tensors are rewritten by the next iterate

          // Gauss-Jordan over the 16-lane row (single_crystal.hip): the pivot of column c is the unused lane with the largest
          // entry; the row is shifted left by one entry per column, so that the pivot column is entry 0 in every pass of a
          // loop that stays rolled; after the twelve passes fg is entry 0 and the right-hand sides 1..9
          bool used = li >= SC_NSYS;
          int mycol = li;
          double mypiv = 1.0;
#pragma unroll 1
          for (int c = 0; c < SC_NSYS; ++c) {
            double v = used ? -1.0 : fabs(row[0]);
            int who = li;
#pragma unroll
            for (int m = 8; m > 0; m >>= 1) {
              const double ov = __shfl_xor(v, m, 16);
              const int ow2 = __shfl_xor(who, m, 16);
              if (ov > v || (ov == v && ow2 < who)) { v = ov; who = ow2; }
            }
            const bool me = li == who;
            if (me) { used = true; mycol = c; mypiv = row[0]; }
            const double piv = __shfl(row[0], who, 16);
            const double fac = me ? 0.0 : row[0] / piv;
#pragma unroll
            for (int k = 1; k < 22; ++k) {
              const double pk2 = __shfl(row[k], who, 16);
              row[k - 1] = __builtin_fma(-fac, pk2, row[k]);
            }
            row[21] = 0.0;
          }
          const int dst = (lane & 48) | (mycol & 15);
          const double ipiv = 1.0 / mypiv;
          const double delta = fx_push(row[0] * ipiv, dst);
#pragma unroll
          for (int k = 0; k < 9; ++k) {
            const double x = fx_push(row[1 + k] * ipiv, dst);
            X9[k] = (!done && !bad) ? x : X9[k];   // the accepted iterate is the last one that gets here
          }

          if (!done) {
            if (bad) {
              if (it == 0) { st_g = 1; done = true; }   // no step to halve: the integration fails here
              else {
                step *= 0.5;
                dgi -= step;
                ++it;
                if (it >= (unsigned)prm.maxit) { st_g = 1; done = true; }
              }
            } else {
              old = fmx;
              dg_acc = dgi;
              step = -delta;
              dgi += step;
              if (conv || it >= (unsigned)prm.maxit) {
                if (!conv) st_g = 1;
                done = true;
              } else {
                ++it;
              }
            }
          }
          if (__ballot(!done) == 0) break;
        }
        if (!work) { dgi = 0.0; dg_acc = 0.0; }

        // the tangent of the row's point in the material frame, at the iterate the convergence test saw: lane j forms
        // dP / d dg_j, lane u < 9 column u of dP/dF at fixed dg; entry (t, u) = column_u[t] - sum_j dP_j[t] X_j[u]
        {
          FxKin k;
          iterate(dg_acc, k);
          const double c = pk[18];
          double mu[9];
          {
            FX_SYS_ROW(sys3);
#pragma unroll
            for (int t = 0; t < 9; ++t) mu[t] = sys3[t];
          }
          double dFe[9], dG[9], dP[9];
          slip_variation(k, mu, dFe, dG);
          fx_dP(sp, k, c, dFe, dG, dP);
#pragma unroll
          for (int r = 0; r < 9; ++r) xr[li * 9 + VEC[r]] = work ? dP[r] : 0.0;
          f_variation(k, dFe);
          fx_dP(sp, k, c, dFe, nullptr, dP);
          if (li < 9) {
#pragma unroll
            for (int r = 0; r < 9; ++r) xr[(12 + li) * 9 + VEC[r]] = dP[r];
          }
        }
        wave_lds_sync();
        {
          int ro = (ow - p0) * 81;
          asm volatile("" : "+v"(ro));
          double* rec = outt + ro;
#pragma unroll 1
          for (int t = 0; t < 9; ++t) {
            const double dpt = xr[li * 9 + t];
#pragma unroll
            for (int u = 0; u < 9; ++u) {
              double v = dpt * X9[u];
#pragma unroll
              for (int m = 8; m > 0; m >>= 1) v += __shfl_xor(v, m, 16);
              if (owner >= 0 && li == u) rec[t * 9 + u] = xr[(12 + u) * 9 + t] - v;
            }
          }
        }
        // handed to the point's own thread in its own slot of the round: read in step 4
        if (work) hand[(ow - p0) * FX_HAND + li] = dgi;
        if (owner >= 0 && li == 12) hand[(ow - p0) * FX_HAND + 12] = (double)st_g;
        if (owner >= 0 && li == 13) hand[(ow - p0) * FX_HAND + 13] = (double)it;
        wave_lds_sync();
      }

      // ---- 4. new state, stress and the tangent in the global axes, one thread per point of the round --------------------
      if (mine) {
        asm volatile("" : "+v"(sl));
        double dg[SC_NSYS];
        int status = 0;
        unsigned iters = 0;
        if (plastic) {
          int ho = (lane - p0) * FX_HAND;
          asm volatile("" : "+v"(ho));
          const double* h = hand + ho;
          status = (int)h[12];
          iters = (unsigned)h[13];
#pragma unroll
          for (int i = 0; i < SC_NSYS; ++i) dg[i] = h[i];
        }
        const bool moved = plastic && status == 0;
        if (!moved) {
#pragma unroll
          for (int i = 0; i < SC_NSYS; ++i) dg[i] = 0.0;
        }
        load_frame();
        double cchk = 0.0;   // sum of everything the point writes
        FxKin k;
#pragma unroll
        for (int t = 0; t < 9; ++t) k.A[t] = (t % 4 == 0) ? 1.0 : 0.0;
#pragma unroll
        for (int j = 0; j < SC_NSYS; ++j)
#pragma unroll
          for (int t = 0; t < 9; ++t)
            if (SC.s[j][t / 3] * SC.n[j][t % 3] != 0) k.A[t] -= (INV_SQRT6 * (SC.s[j][t / 3] * SC.n[j][t % 3])) * dg[j];
        double c;
        {
          double fetr[9], fpi[9];
#pragma unroll
          for (int t = 0; t < 9; ++t) { fetr[t] = mypark[t]; fpi[t] = mypark[9 + t]; }
          c = mypark[18];
          fx_kinematics(sp, fetr, fpi, k);
        }
        if (valid) {
          // Fp = dFp Fp_n = A^-1 Fp_n / a3
          double adj[9], fpn[9], fp[9];
          fx_adj(k.A, adj);
          const double sc = k.a3 * k.a3;   // adj / det / a3 = adj a3^3 / a3
#pragma unroll
          for (int t = 0; t < 9; ++t) { adj[t] *= sc; fpn[RM[t]] = load0(FX_SLOT_FP + t); }
          fx_mul(adj, fpn, fp);
#pragma unroll
          for (int t = 0; t < 9; ++t) {
            const double v = moved ? fp[RM[t]] : fpn[RM[t]];
            store1(FX_SLOT_FP + t, v);
            cchk += v;
          }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int i = 0; i < SC_NSYS; ++i) {
            const double g = load0(FX_SLOT_G + i);
            const double p = load0(FX_SLOT_P + i);
            const double a = load0(FX_SLOT_A + i);
            const double adg = fabs(dg[i]);
            const double da = (dg[i] - sp.d * a * adg) / (1.0 + sp.d * adg);
            const double gn = moved ? g + dg[i] : g, pn = moved ? p + adg : p, an = moved ? a + da : a;
            store1(FX_SLOT_G + i, gn);
            store1(FX_SLOT_P + i, pn);
            store1(FX_SLOT_A + i, an);
            cchk += gn + pn + an;
            __builtin_amdgcn_sched_barrier(0);   // system after system: issued together the 36 loads cost 72 VGPRs
          }
        }
        int ro = (lane - p0) * 81;
        asm volatile("" : "+v"(ro));
        double* rec = outt + ro;
        if (!moved) {   // the St-Venant-Kirchhoff tangent about Fp_n, column by column
#pragma unroll
          for (int u = 0; u < 9; ++u) {
            double dFe[9], dP[9];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
              for (int cc = 0; cc < 3; ++cc) dFe[r * 3 + cc] = (r == RM[u] / 3) ? k.G[(RM[u] % 3) * 3 + cc] : 0.0;
            fx_dP(sp, k, c, dFe, nullptr, dP);
#pragma unroll
            for (int r = 0; r < 9; ++r) rec[VEC[r] * 9 + u] = dP[r];
            __builtin_amdgcn_sched_barrier(0);   // column after column
          }
        }
        double P[9];
        {
          double x[9];
          fx_mul_ns(k.Fe, k.S, x);
          fx_mul_nt(x, k.G, P);
#pragma unroll
          for (int t = 0; t < 9; ++t) P[t] *= c;
        }
        if constexpr (FRAME != OR_FRAME_NONE) {
          // P = R^T P_m R
          double x[9];
#pragma unroll
          for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) x[i * 3 + j] = R[0][i] * P[j] + R[1][i] * P[3 + j] + R[2][i] * P[6 + j];
          fx_mul(x, &R[0][0], P);
          // T[(iJ),(kL)] = R_ai R_bJ T_m[(ab),(cd)] R_ck R_dL in place, one index per pass: new[.. x ..] = sum_y R[y][x] old[.. y ..]
#pragma unroll
          for (int pass = 0; pass < 4; ++pass) {
#pragma unroll
            for (int o = 0; o < 27; ++o) {
              const int oo[3] = {o / 9, (o / 3) % 3, o % 3};   // the three indices the pass leaves alone, in order
              int idx[3];
#pragma unroll
              for (int y = 0; y < 3; ++y) {
                int q4[4], nx = 0;
#pragma unroll
                for (int pos = 0; pos < 4; ++pos) q4[pos] = pos == pass ? y : oo[nx++];
                idx[y] = VEC[q4[0] * 3 + q4[1]] * 9 + VEC[q4[2] * 3 + q4[3]];
              }
              const double v0 = rec[idx[0]], v1 = rec[idx[1]], v2 = rec[idx[2]];
#pragma unroll
              for (int x2 = 0; x2 < 3; ++x2) rec[idx[x2]] = R[0][x2] * v0 + R[1][x2] * v1 + R[2][x2] * v2;
              if (o % 9 == 8) __builtin_amdgcn_sched_barrier(0);
            }
            __builtin_amdgcn_sched_barrier(0);
          }
        }
#pragma unroll
        for (int t = 0; t < 81; ++t) {
          cchk += rec[t];
          if (t % 9 == 8) __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int t = 0; t < 9; ++t) cchk += P[t];
#include "tile_rows9_put.hpp"
        if (valid && plastic) {
          ++c_plastic;
          if (status != 0) ++c_notconv;
          c_maxit = iters > c_maxit ? iters : c_maxit;
        }
        if (valid && !(fabs(cchk) <= 1.79769313486231570e308)) ++c_nan;
      }
      wave_lds_sync();

      // ---- 5. the round's tangent leaves in output order ------------------------------------------------------------------
#include "tile_out81_copyout.hpp"
      wave_lds_sync();
    }

    // ---- 6. PK1 -----------------------------------------------------------------------------------------------------------
#include "tile_rows9_store.hpp"
    wave_lds_sync();   // the LDS regions are rewritten by the next tile
  }

  // store_block_stats (dxm_common.hpp) for a workgroup of FX_WAVES waves
  c_plastic = wave_sum(c_plastic);
  c_notconv = wave_sum(c_notconv);
  c_nan = wave_sum(c_nan);
  c_maxit = wave_max(c_maxit);
  if ((threadIdx.x & (WAVE - 1)) == 0) {
    red[wid * 4 + 0] = c_plastic; red[wid * 4 + 1] = c_notconv; red[wid * 4 + 2] = c_nan; red[wid * 4 + 3] = c_maxit;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    BlockStats bs = {0, 0, 0, 0};
    for (int w = 0; w < FX_WAVES; ++w) {
      bs.n_plastic += red[w * 4 + 0];
      bs.n_not_converged += red[w * 4 + 1];
      bs.n_nan += red[w * 4 + 2];
      bs.max_iters = red[w * 4 + 3] > bs.max_iters ? red[w * 4 + 3] : bs.max_iters;
    }
    stats[blockIdx.x] = bs;
  }
}
#undef FX_SYS_ROW

const void* fs_single_crystal_kernel_fn() { return (const void*)fs_single_crystal_kernel<OR_FRAME_NONE>; }

void fs_single_crystal_launch(int frame, int grid, hipStream_t st, const LawParams& prm, const FxParams& sp, int64_t cnt, const double* F,
                              const Frame9& uniform, const double* frames, int64_t ldf, const double* s0, double* s1, int64_t ld, double* P,
                              double* ct, BlockStats* bs) {
#define DXM_LAUNCH_FX(FR) \
  hipLaunchKernelGGL((fs_single_crystal_kernel<FR>), dim3(grid), dim3(FX_BLOCK), 0, st, prm, sp, cnt, F, uniform, frames, ldf, s0, s1, ld, P, ct, bs)
  if (frame == OR_FRAME_FIELD) DXM_LAUNCH_FX(OR_FRAME_FIELD);
  else if (frame == OR_FRAME_UNIFORM) DXM_LAUNCH_FX(OR_FRAME_UNIFORM);
  else DXM_LAUNCH_FX(OR_FRAME_NONE);
#undef DXM_LAUNCH_FX
}

}  // namespace dxm
