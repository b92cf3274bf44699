// The plane-strain hypothesis for gfx950: isotropic elasticity and J2 plasticity with linear or Voce isotropic hardening in the four
// components [xx, yy, zz, sqrt(2) xy] that strain, stress and plastic strain have in a plane-strain state (the reference's
// MFrontMaterial(..., hypothesis="plane_strain"), dolfinx_materials/mfront.py:33-37; utils.py:146-150 for the 4-vector of a 2x2
// tensor).  The update is the radial return of tests/mfront/IsotropicLinearHardeningPlasticity.mfront:49-77 in the (eps_p, p) form
// that small_strain_body.hpp states for six components, with every sum over four: the out-of-plane shears of such a state are
// zero and stay zero, so nothing is lost.  The Mandel shear sqrt(2) eps_xy enters the norms once.  eps_zz is read like the other
// components (a plane-strain caller passes 0); sig_zz is returned.
//   e = eps - epsp_n,  s_e = 2 mu dev(e),  seq = sqrt(3/2 s_e : s_e),  f = seq - R(p_n)
//   f > 0:  dp = f / (H + 3 mu)  (linear)  or the root of  seq - 3 mu dp - R(p_n + dp)  by Newton from dp = 0, ended on
//           |r| <= max(rtol max(|sig0|, 2e-8 mu), rtol seq) or at the cap of dxm_set_newton (Voce: small_strain.hpp::hardening_R / _dR)
//           n = 3/2 s_e / seq,  epsp = epsp_n + dp n,  p = p_n + dp,  e -= dp n
//   sig = lambda tr(e) 1 + 2 mu e
//   Ct = c1 1x1 + c2 I + c3 n x n,  1 = [1, 1, 1, 0],  (c1, c2, c3) = (lambda + 2 mu^2 b, 2 mu - 6 mu^2 b, 4 mu^2 (b - g)),
//        b = dp / seq,  g = 1 / (R'(p) + 3 mu);  an elastic point: (lambda, 2 mu, 0).  The tangent is built with n = dev(sig) w,
//        w = 3/2 / (seq (1 - 3 mu b)), as the 6-wide kernels do.
//
// Contraction: OFF in the kernel body (#pragma clang fp contract(off)): every operation is individually rounded, in the order
// written, so that a restatement follows it; the translation unit's -ffp-contract=fast does not apply to it.  The 6-wide kernels
// are contracted, so the two agree to rounding, not to the bit.
//
// Mapping and memory as plane_stress.hip and small_strain.hpp: one thread per point, one wave per tile of 64 points, 256-thread
// workgroups, grid-stride over the tiles, wave-private LDS ordered by wave_lds_sync() (no workgroup barrier in the tile loop), one
// BlockStats record per workgroup.
//   strain in / stress out: a tile's rows of 4 are 2048 contiguous bytes, exactly two passes of 64 lanes x 16 B, redistributed
//     through LDS (a lane reads its row as two 16 B LDS loads);
//   state: five 8 B-per-lane SoA streams in and out; an elastic point writes back the bits it read;
//   tangent: never held per thread.  Each point stages (c1, c2, c3, n0..n3) in LDS and the wave writes the 16 entries per point
//     in output order: a tile's tangent is 8192 B, 8 full passes of 16 B per lane, non-temporal.  One point's entries are one
//     128 B line and 8 lanes write it: every line is written whole.  In pass k lane l writes the pair (row (l & 7) >> 1, columns
//     2 (l & 1) and + 1) of point 8 k + (l >> 3): row and column are fixed per lane, only the point advances.  Entries are
//     k3 * (ni * nj): the block is exactly symmetric (small_strain.hpp::tangent_pair).  The elastic law: an entry depends on its
//     column only, nothing is staged;
//   a ragged last tile is bounded by lane: rows of 4 doubles are whole pairs, so a pair is read or written or not, and nothing
//     is read or written past the launch's points.
#include "plane_strain.hpp"

#define DXM_UPDATE_KERNELS_ONLY
#include "small_strain.hpp"   // hardening_R / hardening_dR, SS_THIRD (no kernel of that header is instantiated here)

namespace dxm {

static_assert(PE_ELASTIC == LAW_ELASTIC && PE_J2_LINEAR == LAW_J2_LINEAR && PE_J2_VOCE == LAW_J2_VOCE, "the hardening laws are looked up by these ids");

template <int LAW>
__global__ void __launch_bounds__(BLOCK)
plane_strain_kernel(const LawParams prm, const int64_t n, const double* __restrict__ grad, const double* __restrict__ s0,
                    double* __restrict__ s1, const int64_t ld, double* __restrict__ flux, double* __restrict__ ct,
                    BlockStats* __restrict__ stats) {
#pragma clang fp contract(off)
  constexpr bool STATE = LAW != PE_ELASTIC;
  __shared__ __attribute__((aligned(16))) double lds_all[WAVES_PER_BLOCK * PE_LDS_PER_WAVE];
  __shared__ unsigned long long red[4 * WAVES_PER_BLOCK];
  static_assert(PE_LDS_BYTES == sizeof(lds_all) + sizeof(red), "plane_strain.hpp states the LDS of the kernel");
  static_assert(WAVE * PE_DIM == 2 * 2 * WAVE && WAVE * PE_CT == 8 * 2 * WAVE && (PE_LDS_PER_WAVE * 8) % 16 == 0,
                "a tile's rows are two, its tangent eight whole passes of 16 B per lane");

  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  double* stage = lds_all + wid * PE_LDS_PER_WAVE;            // 64 x 4: strain in, stress out
  double2_t* stage2 = reinterpret_cast<double2_t*>(stage);
  [[maybe_unused]] double* rec = stage + WAVE * PE_DIM;       // 64 x (c1, c2, c3, n0..n3)

  const int64_t ntiles = (n + WAVE - 1) / WAVE;
  const int64_t tile_stride = (int64_t)gridDim.x * WAVES_PER_BLOCK;
  unsigned long long c_plastic = 0, c_notconv = 0, c_nan = 0, c_iters = 0;
  const double lambda = prm.lambda, mu = prm.mu;
  const double mu2 = 2.0 * mu;

  // this lane's pair of the tangent: row ti, columns tj and tj + 1 of the point 8 k + tq in pass k
  const int tq = lane >> 3, ti = (lane & 7) >> 1, tj = (lane & 1) * 2;
  const double t0 = ((ti < 3 && tj < 3) ? 1.0 : 0.0), t1 = ((ti < 3 && tj + 1 < 3) ? 1.0 : 0.0);   // 1x1
  const double d0 = (ti == tj) ? 1.0 : 0.0, d1 = (ti == tj + 1) ? 1.0 : 0.0;                         // I

  for (int64_t tile = (int64_t)blockIdx.x * WAVES_PER_BLOCK + wid; tile < ntiles; tile += tile_stride) {
    const int64_t base = tile * WAVE;
    const int npts = (n - base) < WAVE ? (int)(n - base) : WAVE;
    const bool valid = lane < npts;
    const int64_t gi = base + lane;

    // ---- 1. the tile's strain rows: 128 x 16 B, coalesced, into LDS (zeros beyond the last point); the old state ---------------
    {
      const double2_t* g2 = reinterpret_cast<const double2_t*>(grad + base * PE_DIM);
      const int npairs = npts * 2;
#pragma unroll
      for (int pass = 0; pass < 2; ++pass) {
        const int q = lane + pass * WAVE;
        double2_t v = {0.0, 0.0};
        if (q < npairs) v = stream_load<2>(g2 + q);
        stage2[q] = v;
      }
    }
    double p_n = 0.0, ep[4] = {0.0, 0.0, 0.0, 0.0};
    if constexpr (STATE) {
      if (valid) {
        p_n = stream_load<3>(s0 + gi);
#pragma unroll
        for (int c = 0; c < 4; ++c) ep[c] = stream_load<3>(s0 + (int64_t)(1 + c) * ld + gi);
      }
    }
    wave_lds_sync();
    double e[4];
    {
      const double2_t a = stage2[lane * 2], b = stage2[lane * 2 + 1];
      e[0] = a.x; e[1] = a.y; e[2] = b.x; e[3] = b.y;
    }
    wave_lds_sync();   // the staging region is reused for the stress below

    // ---- 2. the law ------------------------------------------------------------------------------------------------------------
    double c1 = lambda, c2 = mu2, c3 = 0.0, wn = 0.0;
    double p_new = p_n;
    if constexpr (STATE) {
#pragma unroll
      for (int c = 0; c < 4; ++c) e[c] -= ep[c];               // trial elastic strain
      const double third = ((e[0] + e[1]) + e[2]) / 3.0;
      const double se[4] = {mu2 * (e[0] - third), mu2 * (e[1] - third), mu2 * (e[2] - third), mu2 * e[3]};
      const double nrm2 = ((se[0] * se[0] + se[1] * se[1]) + se[2] * se[2]) + se[3] * se[3];
      const double seq = sqrt(1.5 * nrm2);
      const double f = seq - hardening_R<LAW>(prm, p_n);
      if (f > 0.0) {
        double dp;
        unsigned iters = 0;
        if constexpr (LAW == PE_J2_LINEAR) {
          dp = f / (prm.h1 + 3.0 * mu);
        } else {
          dp = 0.0;
          const double tolp = fmax(prm.tol, prm.rtol * seq);
          for (int it = 0;; ++it) {
            const double r = (seq - (3.0 * mu) * dp) - hardening_R<LAW>(prm, p_n + dp);
            if (fabs(r) <= tolp) break;
            if (it >= prm.maxit) { if (valid) ++c_notconv; break; }
            const double dr = -(3.0 * mu) - hardening_dR<LAW>(prm, p_n + dp);
            dp -= r / dr;
            ++iters;
          }
        }
        const double iseq = 1.0 / seq;
        const double beta = dp * iseq;
        {
          // rho = R(p) / seq of the returned state; <= 0: the direction is undefined (small_strain_body.hpp), reported, never silent
          const double rho = 1.0 - (3.0 * mu) * beta;
          wn = rho > 0.0 ? (1.5 * iseq) / rho : 0.0;
          if (LAW != PE_J2_LINEAR || prm.h1 < 0.0) { if (valid && !(rho > 0.0)) ++c_notconv; }
        }
        const double gamma = 1.0 / (hardening_dR<LAW>(prm, p_n + dp) + 3.0 * mu);
        const double mm = mu * mu;
        c1 = lambda + (2.0 * mm) * beta;
        c2 = mu2 - (6.0 * mm) * beta;
        c3 = (4.0 * mm) * (beta - gamma);
        p_new = p_n + dp;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const double dn = dp * ((1.5 * se[c]) * iseq);
          ep[c] += dn;
          e[c] -= dn;
        }
        if (valid) {
          ++c_plastic;
          c_iters = iters > c_iters ? iters : c_iters;
        }
      }
    }
    const double ltr = lambda * ((e[0] + e[1]) + e[2]);
    const double s[4] = {ltr + mu2 * e[0], ltr + mu2 * e[1], ltr + mu2 * e[2], mu2 * e[3]};
    double nn[4] = {0.0, 0.0, 0.0, 0.0};
    if constexpr (STATE) {
      const double third = ((s[0] + s[1]) + s[2]) * SS_THIRD;
      nn[0] = (s[0] - third) * wn; nn[1] = (s[1] - third) * wn; nn[2] = (s[2] - third) * wn; nn[3] = s[3] * wn;
    }
    {
      // a non-finite stress, state or tangent entry: v * 0 is NaN exactly for those (the entries are sums of products of these)
      double z = 0.0;
#pragma unroll
      for (int c = 0; c < 4; ++c) z = __builtin_fma(s[c], 0.0, z);
      if constexpr (STATE) {
#pragma unroll
        for (int c = 0; c < 4; ++c) z = __builtin_fma(ep[c], 0.0, __builtin_fma(nn[c], 0.0, z));
        z = __builtin_fma(p_new, 0.0, __builtin_fma(c1, 0.0, __builtin_fma(c2, 0.0, __builtin_fma(c3, 0.0, z))));
      }
      if (valid && !(z == 0.0)) ++c_nan;
    }

    // ---- 3. new state, SoA (an elastic point writes back the bits it read); stress and tangent record into LDS -------------------
    if constexpr (STATE) {
      if (valid) {
        stream_store<1>(s1 + gi, p_new);
#pragma unroll
        for (int c = 0; c < 4; ++c) stream_store<1>(s1 + (int64_t)(1 + c) * ld + gi, ep[c]);
      }
      double* cf = rec + lane * PE_REC;
      cf[0] = c1; cf[1] = c2; cf[2] = c3;
      cf[3] = nn[0]; cf[4] = nn[1]; cf[5] = nn[2]; cf[6] = nn[3];
    }
    stage2[lane * 2] = double2_t{s[0], s[1]};
    stage2[lane * 2 + 1] = double2_t{s[2], s[3]};
    wave_lds_sync();

    // ---- 4. the stress rows, as the strain came in --------------------------------------------------------------------------------
    {
      double2_t* f2 = reinterpret_cast<double2_t*>(flux + base * PE_DIM);
      const int npairs = npts * 2;
#pragma unroll
      for (int pass = 0; pass < 2; ++pass) {
        const int q = lane + pass * WAVE;
        if (q < npairs) stream_store<0>(f2 + q, stage2[q]);
      }
    }
    // ---- 5. the tangent in output order: 8 passes of 64 x 16 B, pair (ti, tj..tj+1) of point 8 k + tq -----------------------------
    {
      double2_t* c2g = reinterpret_cast<double2_t*>(ct + base * PE_CT);
#pragma unroll 2   // fully unrolled, the LDS reads of all eight passes are issued together: 160 VGPRs and 3 waves per SIMD for Voce
      for (int pass = 0; pass < 8; ++pass) {
        const int q = pass * 8 + tq;
        double2_t v;
        if constexpr (STATE) {
          const double* cf = rec + q * PE_REC;
          const double k1 = cf[0], k2 = cf[1], k3 = cf[2];
          const double ni = cf[3 + ti], nj0 = cf[3 + tj], nj1 = cf[4 + tj];
          v.x = (t0 * k1 + d0 * k2) + k3 * (ni * nj0);
          v.y = (t1 * k1 + d1 * k2) + k3 * (ni * nj1);
        } else {
          v.x = t0 * lambda + d0 * mu2;
          v.y = t1 * lambda + d1 * mu2;
        }
        if (q < npts) stream_store<0>(c2g + pass * WAVE + lane, v);
      }
    }
    wave_lds_sync();   // the LDS region is rewritten by the next tile
  }

  store_block_stats(stats, c_plastic, c_notconv, c_nan, c_iters, red);
}

const void* plane_strain_elastic_kernel_fn() { return (const void*)plane_strain_kernel<PE_ELASTIC>; }
const void* plane_strain_j2_linear_kernel_fn() { return (const void*)plane_strain_kernel<PE_J2_LINEAR>; }
const void* plane_strain_j2_voce_kernel_fn() { return (const void*)plane_strain_kernel<PE_J2_VOCE>; }

void plane_strain_launch(int law, int grid, hipStream_t st, const LawParams& prm, int64_t cnt, const double* grad, const double* s0,
                         double* s1, int64_t ld, double* flux, double* ct, BlockStats* bs) {
#define DXM_LAUNCH_PE(L) \
  hipLaunchKernelGGL((plane_strain_kernel<L>), dim3(grid), dim3(BLOCK), 0, st, prm, cnt, grad, s0, s1, ld, flux, ct, bs)
  if (law == PE_J2_VOCE) DXM_LAUNCH_PE(PE_J2_VOCE);
  else if (law == PE_J2_LINEAR) DXM_LAUNCH_PE(PE_J2_LINEAR);
  else DXM_LAUNCH_PE(PE_ELASTIC);
#undef DXM_LAUNCH_PE
}

}  // namespace dxm
