// Plane-stress J2 plasticity with isotropic hardening for gfx950: the backward-Euler update of laws 1 and 2 (Hooke, von Mises,
// associated flow, R(p) linear or Voce) under sig_zz = sig_xz = sig_yz = 0, what the reference's
// demos/jax/elastoplasticity/_plane_stress_elastoplasticity.py obtains by carrying eps_zz as an extra unknown of the global problem.
// Strain, stress and plastic strain are 3-vectors [xx, yy, sqrt(2) xy] (the convention of plane_stress.hip); the state is p and the
// in-plane plastic strain, eps_p,zz = -(eps_p,xx + eps_p,yy) is implied.
//
// The in-plane form.  In the basis a = (s0 + s1)/sqrt 2, b = (s0 - s1)/sqrt 2, c = s2 both the plane-stress stiffness
// C = diag(CA, CB, CB), CA = E/(1-nu), CB = E/(1+nu), and the deviatoric projector P = diag(1/3, 1, 1) are diagonal, and
// seq^2 = 3/2 s^T P s = 1/2 sa^2 + 3/2 sb^2 + 3/2 sc^2.  With the multiplier dg of  eps_p - eps_p,n = dg P s  (dg = 3/2 dp / seq):
//   t = C (eps - eps_p,n),   s_i = t_i / (1 + dg k_i),  k = (CA/3, CB, CB),   p = p_n + 2/3 dg seq(dg)
//   g(dg) = seq(dg) - R(p_n + 2/3 dg seq(dg)) = 0
// For hardening parameters (H >= 0; Voce with sigu >= sig0) g is decreasing and convex: one root.  Softening parameters (H < 0,
// sigu < sig0), which the build functions accept, lose both: only g(0) > 0 >= g(hi) below holds for them, and the bracket finds a
// root between.  Even linear hardening has no closed form, so both laws iterate:
//   start: the larger of two lower bounds of the root.  With kmax = max k_i, seq(dg) >= seq_tr / (1 + dg kmax) and seq(dg) <= seq_tr;
//     R concave gives R(p) <= R_n + R'_n (p - p_n), so g >= seq_tr / (1 + dg kmax) - R_n - c dg with c = 2/3 max(R'_n, 0) seq_tr, whose
//     root is 2 f / (B + sqrt(B^2 + 4 c kmax f)), B = c + R_n kmax, f = seq_tr - R_n (H = 0: the start of plane_stress.hip); Voce also
//     has R <= max(sigu, R_n) = cap: dg >= (seq_tr / cap - 1) / kmax.
//   safeguard: a root is bracketed in [lo, hi], lo = 0 (g(0) = f > 0), hi = (seq_tr / floor - 1) / kmin with floor a positive lower
//     bound of R over the step: seq(hi) <= seq_tr / (1 + hi kmin) = floor <= R, so g(hi) <= 0.  Hardening: floor = R_n.  Voce:
//     floor = min(R_n, sigu) (R runs monotonically from R_n towards sigu).  Linear, H < 0: p - p_n = 2/3 dg seq(dg) and
//     dg s_i = t_i dg / (1 + dg k_i) < t_i / k_i, so p - p_n < 2/3 sqrt(1/2 (ta/ka)^2 + 3/2 ((tb/CB)^2 + (tc/CB)^2)) = dp_max and
//     floor = R_n + H dp_max.  A floor that is not positive gives no bracket: the point is counted in n_not_converged at its first
//     residual and writes the start (the 6-wide body does the same for rho <= 0).  Every iterate moves the end of its sign; a
//     Newton step that leaves (lo, hi) is replaced by the midpoint.  From a lower bound of a convex decreasing g Newton is
//     monotone and the safeguard idle; under softening it works.
//   end: |g| <= max(tol, rtol seq_tr), the tolerance of the 6-wide laws (dxm_set_newton); the step computed from that last residual
//     is still taken, unsafeguarded.  A point at the cap is counted and writes its last iterate.
// eps_p = eps - C^-1 s at a yielded point.  Tangent, with A = diag(C_i / (1 + dg k_i)), n = 3/2 P s, theta = 1 - 2/3 R' dg:
//   D = A - (A n)(A n)^T / (n^T A n + R' seq^2 / theta),   R' = 0: the TANGENT block of plane_stress.hip with q = 3/2
// rotated back from the basis; the plane-stress C at an elastic point.  Six distinct numbers: the block is exactly symmetric.
// A non-finite strain takes the elastic path (no comparison with NaN holds), keeps its state bits and counts once in n_nan.
//
// Every operation is individually rounded (no contraction), in the order written in the body, so that a restatement follows it;
// hardening_R / hardening_dR are small_strain.hpp's, called, not copied (the linear R = sig0 + H p is one contracted FMA there).
//
// Mapping and memory as plane_stress.hip: one thread per point, one wave per tile of 64 points, 256-thread workgroups, grid-stride
// over the tiles, wave-private LDS ordered by wave_lds_sync() (no workgroup barrier in the tile loop), one BlockStats record per
// workgroup.  A tile's strain and stress rows of 3 move through LDS by tile_rows3_load.hpp / tile_rows3_store.hpp; the state is four
// 8 B-per-lane SoA streams in and out (an elastic point writes back the bits it read).  The 9-wide tangent is never held per thread:
// each point stages its six distinct numbers in LDS and tile_entries_store.hpp writes the tile's 4608 B in output order (a tile
// starts on a multiple of 512 B: every 128 B line is written whole).  A ragged last tile is bounded by lane in those three texts.
// 184 B/point: strain 24 + state 32 in, stress 24 + tangent 72 + state 32 out.
#include "plane_stress_j2.hpp"

#define DXM_UPDATE_KERNELS_ONLY
#include "small_strain.hpp"   // hardening_R / hardening_dR (no kernel of that header is instantiated here)

namespace dxm {

static_assert(PSJ_LINEAR == LAW_J2_LINEAR && PSJ_VOCE == LAW_J2_VOCE, "the hardening laws are looked up by these ids");

template <int HARD>
__global__ void __launch_bounds__(BLOCK)
plane_stress_j2_kernel(const PsJ2Params prm, const int64_t n, const double* __restrict__ grad, const double* __restrict__ s0,
                       double* __restrict__ s1, const int64_t ld, double* __restrict__ flux, double* __restrict__ ct,
                       BlockStats* __restrict__ stats) {
#pragma clang fp contract(off)
  constexpr int W = 9;   // tangent entries per point: the row-major 3 x 3
  __shared__ __attribute__((aligned(16))) double lds_all[WAVES_PER_BLOCK * PSJ_LDS_PER_WAVE];
  __shared__ unsigned long long red[4 * WAVES_PER_BLOCK];
  static_assert(PSJ_LDS_BYTES == sizeof(lds_all) + sizeof(red), "plane_stress_j2.hpp states the LDS of the kernel");
  static_assert((WAVE * 3) % 2 == 0 && (WAVE * W) % 2 == 0 && (PSJ_LDS_PER_WAVE * 8) % 16 == 0, "16 B accesses of whole tiles");

  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  double* stage = lds_all + wid * PSJ_LDS_PER_WAVE;           // 64 x 3: strain in, stress out
  double2_t* stage2 = reinterpret_cast<double2_t*>(stage);
  double* rec = stage + WAVE * 3;                             // 64 x (D00, D01, D02, D11, D12, D22)

  const int64_t ntiles = (n + WAVE - 1) / WAVE;
  const int64_t tile_stride = (int64_t)gridDim.x * WAVES_PER_BLOCK;
  unsigned long long c_plastic = 0, c_notconv = 0, c_nan = 0, c_iters = 0;
  const double CA = prm.CA, CB = prm.CB, ka = prm.ka;
  constexpr double R2 = 0.70710678118654752440;   // 1 / sqrt 2
  constexpr double TWO3 = 2.0 / 3.0;

  for (int64_t tile = (int64_t)blockIdx.x * WAVES_PER_BLOCK + wid; tile < ntiles; tile += tile_stride) {
    const int64_t base = tile * WAVE;
    const int npts = (n - base) < WAVE ? (int)(n - base) : WAVE;
    const bool valid = lane < npts;
    const int64_t gi = base + lane;

    // ---- 1. the tile's strain rows into LDS; the old state -------------------------------------------------------------------------
#include "tile_rows3_load.hpp"
    double p_n = 0.0, epn[3] = {0.0, 0.0, 0.0};
    if (valid) {
      p_n = stream_load<3>(s0 + gi);
#pragma unroll
      for (int a = 0; a < 3; ++a) epn[a] = stream_load<3>(s0 + (int64_t)(1 + a) * ld + gi);
    }
    wave_lds_sync();
    const double eps[3] = {stage[lane * 3 + 0], stage[lane * 3 + 1], stage[lane * 3 + 2]};
    wave_lds_sync();   // the staging region is reused for the stress below

    // ---- 2. the law --------------------------------------------------------------------------------------------------------
    const double ee[3] = {eps[0] - epn[0], eps[1] - epn[1], eps[2] - epn[2]};
    double epo[3] = {epn[0], epn[1], epn[2]}, p_new = p_n;
    double D[PSJ_REC] = {prm.c11, prm.c12, 0.0, prm.c11, 0.0, prm.c33};
    const double ta = CA * ((ee[0] + ee[1]) * R2), tb = CB * ((ee[0] - ee[1]) * R2), tc = CB * ee[2];
    const double seqt = __builtin_sqrt((0.5 * (ta * ta) + 1.5 * (tb * tb)) + 1.5 * (tc * tc));
    const double Rn = hardening_R<HARD>(prm.law, p_n);
    const bool plastic = valid && seqt > Rn && seqt <= 1.7976931348623157e308;
    double sa = ta, sb = tb, sc = tc;
    if (plastic) {
      const double tolp = __builtin_fmax(prm.law.tol, prm.law.rtol * seqt);
      const double f = seqt - Rn;
      double dg;
      {
        const double cc = (TWO3 * __builtin_fmax(hardening_dR<HARD>(prm.law, p_n), 0.0)) * seqt;
        const double B = cc + Rn * prm.kmax;
        dg = (2.0 * f) / (B + __builtin_sqrt(B * B + (4.0 * (cc * prm.kmax)) * f));
        if constexpr (HARD == PSJ_VOCE) {
          const double cap = __builtin_fmax(prm.law.h1, Rn);
          dg = __builtin_fmax(dg, (seqt / cap - 1.0) / prm.kmax);
        }
        if (!(dg >= 0.0 && dg <= 1.7976931348623157e308)) dg = 0.0;
      }
      // the lower bound of R over the step (header): R_n itself unless the parameters soften
      // and without a positive bound there is no bracket: that point is counted at its first residual and writes the start
      double floor_R = Rn;
      int cap = prm.law.maxit;
      if constexpr (HARD == PSJ_VOCE) {
        floor_R = __builtin_fmin(Rn, prm.law.h1);
        if (!(floor_R > 0.0)) cap = 0;
      } else if (prm.law.h1 < 0.0) {   // one scalar compare on the kernel's parameters: an H >= 0 launch executes none of this
        const double ua = ta / ka, ub = tb / CB, uc = tc / CB;
        floor_R = Rn + prm.law.h1 * (TWO3 * __builtin_sqrt(0.5 * (ua * ua) + 1.5 * (ub * ub + uc * uc)));
        if (!(floor_R > 0.0)) cap = 0;
      }
      double lo = 0.0, hi = (seqt / floor_R - 1.0) / prm.kmin;
      double da, db, S, seq, pp;
      int it = 0;
      for (;;) {
        da = 1.0 / (1.0 + dg * ka); db = 1.0 / (1.0 + dg * CB);
        sa = ta * da; sb = tb * db; sc = tc * db;
        const double qa = 0.5 * (sa * sa), qb = 1.5 * (sb * sb), qc = 1.5 * (sc * sc);
        S = (qa + qb) + qc;
        seq = __builtin_sqrt(S);
        pp = p_n + (TWO3 * dg) * seq;
        const double g = seq - hardening_R<HARD>(prm.law, pp);
        const bool conv = __builtin_fabs(g) <= tolp;
        if (!conv && it >= cap) { ++c_notconv; break; }
        // seq' = -(sum q_i k_i d_i) / seq,  p' = 2/3 (seq + dg seq'),  g' = seq' - R' p'
        const double dseq = -((qa * (ka * da) + (qb + qc) * (CB * db)) / seq);
        const double gp = dseq - (TWO3 * hardening_dR<HARD>(prm.law, pp)) * (seq + dg * dseq);
        double dgn = dg - g / gp;
        if (conv) {   // the step of the last residual is taken: stress and p are formed at the new multiplier
          dg = dgn;
          da = 1.0 / (1.0 + dg * ka); db = 1.0 / (1.0 + dg * CB);
          sa = ta * da; sb = tb * db; sc = tc * db;
          S = (0.5 * (sa * sa) + 1.5 * (sb * sb)) + 1.5 * (sc * sc);
          seq = __builtin_sqrt(S);
          pp = p_n + (TWO3 * dg) * seq;
          break;
        }
        if (g > 0.0) lo = dg; else hi = dg;
        if (!(dgn > lo && dgn < hi)) dgn = 0.5 * (lo + hi);
        dg = dgn;
        ++it;
      }
      c_iters = (unsigned long long)it > c_iters ? (unsigned long long)it : c_iters;
      p_new = pp;
      // C^-1 s in the basis, rotated back
      const double xa = sa / CA, xb = sb / CB, xc = sc / CB;
      epo[0] = eps[0] - (xa + xb) * R2;
      epo[1] = eps[1] - (xa - xb) * R2;
      epo[2] = eps[2] - xc;
      {
        // A - (A n)(A n)^T / (n^T A n + R' seq^2 / theta), A = diag(C_i / (1 + dg k_i)), n = 3/2 P s, in the basis; then rotated back
        const double dR = hardening_dR<HARD>(prm.law, pp);
        const double theta = 1.0 - (TWO3 * dR) * dg;
        const double Aa = CA * da, Ab = CB * db;
        const double na = 0.5 * sa, nb = 1.5 * sb, nc = 1.5 * sc;
        const double va = Aa * na, vb = Ab * nb, vc = Ab * nc;
        const double den = ((na * va + nb * vb) + nc * vc) + (dR * S) / theta;
        const double Taa = Aa - (va * va) / den, Tbb = Ab - (vb * vb) / den, Tcc = Ab - (vc * vc) / den;
        const double Tab = -((va * vb) / den), Tac = -((va * vc) / den), Tbc = -((vb * vc) / den);
        const double h = 0.5 * (Taa + Tbb);
        D[0] = h + Tab;
        D[1] = 0.5 * (Taa - Tbb);
        D[2] = (Tac + Tbc) * R2;
        D[3] = h - Tab;
        D[4] = (Tac - Tbc) * R2;
        D[5] = Tcc;
      }
      ++c_plastic;
    }
    const double sig[3] = {(sa + sb) * R2, (sa - sb) * R2, sc};
    // a non-finite stress, state or tangent entry: v * 0 is NaN exactly for those
    double z = __builtin_fma(p_new, 0.0, 0.0);
#pragma unroll
    for (int a = 0; a < 3; ++a) z = __builtin_fma(sig[a], 0.0, __builtin_fma(epo[a], 0.0, z));
#pragma unroll
    for (int a = 0; a < PSJ_REC; ++a) z = __builtin_fma(D[a], 0.0, z);
    if (valid && !(z == 0.0)) ++c_nan;

    stage[lane * 3 + 0] = sig[0];
    stage[lane * 3 + 1] = sig[1];
    stage[lane * 3 + 2] = sig[2];
#pragma unroll
    for (int a = 0; a < PSJ_REC; ++a) rec[lane * PSJ_REC + a] = D[a];
    if (valid) {   // an elastic point writes back the bits it read
      stream_store<1>(s1 + gi, p_new);
#pragma unroll
      for (int a = 0; a < 3; ++a) stream_store<1>(s1 + (int64_t)(1 + a) * ld + gi, epo[a]);
    }
    wave_lds_sync();

    // ---- 3. the stress rows, as the strain came in ---------------------------------------------------------------------------
#include "tile_rows3_store.hpp"
    // ---- 4. the tangent in output order: entry e of the tile belongs to point e / 9, column e % 9 of the row-major 3 x 3 ----
    auto entry = [&](int e) -> double {
      const int p = e / W, col = e - p * W;
      return rec[p * PSJ_REC + sym3_slot(col)];
    };
#include "tile_entries_store.hpp"
    wave_lds_sync();   // the LDS region is rewritten by the next tile
  }

  store_block_stats(stats, c_plastic, c_notconv, c_nan, c_iters, red);
}

const void* plane_stress_j2_linear_kernel_fn() { return (const void*)plane_stress_j2_kernel<PSJ_LINEAR>; }
const void* plane_stress_j2_voce_kernel_fn() { return (const void*)plane_stress_j2_kernel<PSJ_VOCE>; }

void plane_stress_j2_launch(int hard, int grid, hipStream_t st, const PsJ2Params& prm, int64_t cnt, const double* grad,
                            const double* s0, double* s1, int64_t ld, double* flux, double* ct, BlockStats* bs) {
#define DXM_LAUNCH_PSJ(H) \
  hipLaunchKernelGGL((plane_stress_j2_kernel<H>), dim3(grid), dim3(BLOCK), 0, st, prm, cnt, grad, s0, s1, ld, flux, ct, bs)
  if (hard == PSJ_VOCE) DXM_LAUNCH_PSJ(PSJ_VOCE);
  else DXM_LAUNCH_PSJ(PSJ_LINEAR);
#undef DXM_LAUNCH_PSJ
}

}  // namespace dxm
