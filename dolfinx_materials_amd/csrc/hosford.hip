// Small-strain Hosford plasticity with linear isotropic hardening (gradient: strain (6), flux: stress (6), Mandel) for gfx950.
//
// The law (the reference's IsotropicPlasticHosfordFlowLinear behaviour, restated from its equations): Hooke's law, associated flow
// on the Hosford equivalent stress of the principal stresses s1, s2, s3
//   seq = (1/2 (|s1 - s2|^a + |s1 - s3|^a + |s2 - s3|^a))^(1/a),     R(p) = R0 + H p,
// implicit update (theta = 1) from the trial elastic strain e = eps - eps_p,n, sigma_tr = D e:
//   elastic if seq(sigma_tr) <= R(p_n); else   eps_el - e + dp n(sigma) = 0,  seq(sigma) - R0 - H (p_n + dp) = 0,  n = d seq / d sigma.
// The update is isotropic: sigma is coaxial with sigma_tr and n is deviatoric, so the unknowns are the three principal deviatoric
// stresses s_i and dp, in the eigenbasis (t_i, n_i) of dev(sigma_tr) (register-only cyclic Jacobi):
//   r_i = (s_i - t_i) + 2 mu dp n_i = 0,    r_4 = seq - R0 - H (p_n + dp) = 0,
// plain Newton from (t, 0).  With d = B s the three differences, x_k = d_k / max|d|, phi = 1/2 sum |x_k|^a, q = phi^(-1/a):
//   seq = max|d| / q,   g_k = d seq / d d_k = h_k x_k q,   h_k = 1/2 (|x_k| q)^(a-2),   n = B^T g,
//   d n / d s = (a - 1) / seq (B^T diag(h) B - n n^T).
// Every power is taken of a ratio in [0, 1] (no overflow at any stress level) as exp((a - 2) log x) (pow inlined costs registers:
// small_strain.hpp); x = 0 gives 0, or 1 for a = 2.
// Consistent tangent, with A' = I + 2 mu dp dn/ds, z = A'^-1 n (the Newton matrix of the converged state):
//   principal block  P = lambda 1x1 + 2 mu A'^-1 - 4 mu^2 z z^T / (2 mu n.z + H)      (H = 0 needs no special case: n.z > 0)
//   shear moduli     th_ij = (sigma_i - sigma_j) / (e_i - e_j) = 2 mu / (1 + 2 mu dp rho_ij),   rho_ij = (n_i - n_j) / (s_i - s_j)
//   Ct = sum_ij P_ij E_i E_j^T + sum_{i<j} th_ij M_ij M_ij^T,   E_i = n_i n_i^T, M_ij = (n_i n_j^T + n_j n_i^T) / sqrt(2) as Mandel vectors.
// rho_ij has a form without cancellation: (n_i - n_j) / d_k = (q^(a-1) / max|d|) (u_k + 1/2 DD), u_k = |x_k|^(a-2), DD the divided
// difference of sgn(x) |x|^(a-1) over the two OTHER differences (which differ by d_k).  Of opposite signs they add; of equal sign the
// quotient cancels where they are close -- repeated trial eigenvalues, i.e. uniaxial loading -- and the sinh-series form of the
// Ogden kernel takes over (hyperelastic.hip: m (xy)^((m-1)/2) sinhc(m h) / sinhc(h), h = (ln x - ln y) / 2; exact at x = y).
//
// Mapping: one thread per point, one wave per tile of 64; the tile I/O is the shared text of tile_rows6_*.hpp (strain in, stress
// out) and tile_tri21_store.hpp (the tangent, from the 21 upper-triangle entries each point stages in LDS: 10.5 KiB per wave next to
// the 3 KiB of the strain / stress staging).  While the local Newton runs, the point's record parks its eigenvectors and strains.
// State: SoA, 8 B-per-lane.
#include "hosford.hpp"

#include "principal_axes.hpp"

namespace dxm {

constexpr int HF_SWEEPS = 5;                     // cyclic Jacobi sweeps (hyperelastic.hip: off-diagonal below 1e-16 after 4)

// |x|^(a-2) of a ratio 0 <= ax <= 1 with lx = log(ax)
__device__ __forceinline__ double hf_pow_am2(double ax, double lx, double am2) {
  return ax > 0.0 ? exp(am2 * lx) : (am2 == 0.0 ? 1.0 : 0.0);
}

// (sgn(x) |x|^m - sgn(y) |y|^m) / (x - y), m = a - 1, from the signed ratios, their logarithms and u = |.|^(m-1) (header comment)
__device__ __forceinline__ double hf_divided_difference(double m, double xs, double ys, double lx, double ly, double ux, double uy) {
  const double ax = fabs(xs), ay = fabs(ys);
  const double px = ux * ax, py = uy * ay;
  const bool same = xs * ys > 0.0;
  const double h = 0.5 * (lx - ly), y = m * h;
  const double series = m * sqrt(ux * uy) * sinhc_series(y * y) * fast_rcp(sinhc_series(h * h));
  const double quotient = same ? (px - py) / (ax - ay) : (px + py) / (ax + ay);
  return (same && fmax(fabs(y), fabs(h)) <= 0.1) ? series : quotient;
}

template <int SYM>
__global__ void __launch_bounds__(BLOCK, 2)
hosford_kernel(const LawParams prm, const int64_t n, const double* __restrict__ eps, const double* __restrict__ s0,
               double* __restrict__ s1, const int64_t ld, double* __restrict__ sig, double* __restrict__ ct,
               BlockStats* __restrict__ stats) {
  __shared__ __attribute__((aligned(16))) double lds_all[WAVES_PER_BLOCK * TRI21_LDS_PER_WAVE];
  __shared__ unsigned long long red[4 * WAVES_PER_BLOCK];

  int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  double* tri = lds_all + wid * TRI21_LDS_PER_WAVE;                       // 64 x 21 tangent entries
  double2_t* stage2 = reinterpret_cast<double2_t*>(tri + WAVE * TRI21);   // strain in / stress out staging

  const int64_t ntiles = (n + WAVE - 1) / WAVE;
  const int64_t tile_stride = (int64_t)gridDim.x * WAVES_PER_BLOCK;
  unsigned long long c_plastic = 0, c_notconv = 0, c_nan = 0, c_maxit = 0;

  const double lambda = prm.lambda, mu = prm.mu;
  const double SQ2 = 1.4142135623730950488;

  for (int64_t tile = (int64_t)blockIdx.x * WAVES_PER_BLOCK + wid; tile < ntiles; tile += tile_stride) {
    const int64_t base = tile * WAVE;
    const int npts = (n - base) < WAVE ? (int)(n - base) : WAVE;
    // per-lane invariants are re-derived per tile from an opaque copy (small_strain.hpp: hoisted, they cost registers over the whole body)
    asm volatile("" : "+v"(lane));
    lane &= WAVE - 1;
    const bool valid = lane < npts;
    const int64_t gi = base + lane;

    // ---- 1. coalesced strain load (3 x 1 KiB per wave) into LDS; old state, SoA ----------------------------
    double e[6], ep[6] = {0, 0, 0, 0, 0, 0}, p_n = 0.0;
#include "tile_rows6_load.hpp"
    if (valid) {
      p_n = stream_load<3>(s0 + (int64_t)HF_SLOT_P * ld + gi);
#pragma unroll
      for (int c = 0; c < 6; ++c) ep[c] = stream_load<3>(s0 + (int64_t)(HF_SLOT_EP + c) * ld + gi);
    }
    wave_lds_sync();
#include "tile_rows6_take.hpp"
    wave_lds_sync();   // the staging region is reused for the stress below

    // ---- 2. trial state ------------------------------------------------------------------------------------
#pragma unroll
    for (int c = 0; c < 6; ++c) e[c] -= ep[c];   // trial elastic strain
    const double tr = e[0] + e[1] + e[2];
    // the 21 tangent entries of the point go straight into its LDS record (held in registers next to the eigenvectors they
    // spill at 256 VGPRs); cchk: their sum, for the non-finite check.  While the local Newton runs, the record parks the
    // eigenvectors, the trial strain and the old plastic strain (21 doubles; small_strain.hpp does the same for Ramberg-Osgood)
    int ro = lane * TRI21;   // opaque: every access is base + small immediate
    asm volatile("" : "+v"(ro));
    double* rec = tri + ro;
    double cchk = 0.0;   // sum of everything the point writes
    bool plastic = false;
    // new state (SoA) and the stress into the staging region: called once per point, as soon as the three are known
    auto finish = [&](const double* sg, const double* eel, const double* epl, double p_new) {
      if (valid) {
#pragma unroll
        for (int c = 0; c < 6; ++c) stream_store<1>(s1 + (int64_t)(HF_SLOT_EEL + c) * ld + gi, eel[c]);
        stream_store<1>(s1 + (int64_t)HF_SLOT_P * ld + gi, p_new);
#pragma unroll
        for (int c = 0; c < 6; ++c) stream_store<1>(s1 + (int64_t)(HF_SLOT_EP + c) * ld + gi, epl[c]);
      }
      stage2[lane * 3 + 0] = double2_t{sg[0], sg[1]};
      stage2[lane * 3 + 1] = double2_t{sg[2], sg[3]};
      stage2[lane * 3 + 2] = double2_t{sg[4], sg[5]};
      double chk = p_new;
#pragma unroll
      for (int c = 0; c < 6; ++c) chk += sg[c] + eel[c];
      cchk += chk;
    };
    const double R_n = prm.sig0 + prm.h1 * p_n;
    double vm;
    {
      const double third = tr * (1.0 / 3.0);
      const double d0 = e[0] - third, d1 = e[1] - third, d2 = e[2] - third;
      vm = 2.0 * mu * sqrt(1.5 * (d0 * d0 + d1 * d1 + d2 * d2 + e[3] * e[3] + e[4] * e[4] + e[5] * e[5]));
    }
    // seq <= max|s_i - s_j| <= 2 / sqrt(3) x the von Mises stress for every a >= 1: below that bound the point is elastic and the
    // eigen-solve is skipped (a hydrostatic trial state, vm = 0, never gets past it)
    if (1.1547005383792517 * vm > R_n) {
      // ---- 3. eigenbasis of the deviatoric trial stress ------------------------------------------------------
      const double third = tr * (1.0 / 3.0);
      double t0 = 2.0 * mu * (e[0] - third), t1 = 2.0 * mu * (e[1] - third), t2 = 2.0 * mu * (e[2] - third);
      double t01 = SQ2 * mu * e[3], t02 = SQ2 * mu * e[4], t12 = SQ2 * mu * e[5];   // tensor components: Mandel / sqrt(2)
      double n0[3] = {1.0, 0.0, 0.0}, n1[3] = {0.0, 1.0, 0.0}, n2[3] = {0.0, 0.0, 1.0};
#pragma unroll 1
      for (int sw = 0; sw < HF_SWEEPS; ++sw) {
        jacobi_rotate(t0, t1, t01, t02, t12, n0, n1);
        jacobi_rotate(t0, t2, t02, t01, t12, n0, n2);
        jacobi_rotate(t1, t2, t12, t01, t02, n1, n2);
      }
#pragma unroll
      for (int k = 0; k < 3; ++k) { rec[k] = n0[k]; rec[3 + k] = n1[k]; rec[6 + k] = n2[k]; }
#pragma unroll
      for (int c = 0; c < 6; ++c) { rec[9 + c] = e[c]; rec[15 + c] = ep[c]; }
      asm volatile("" ::: "memory");   // read back from LDS after the loop, not kept in registers
      // ---- 4. principal-space Newton ---------------------------------------------------------------------------
      const double am2 = prm.c[HF_AM2], inva = prm.c[HF_INVA], am1 = prm.c[HF_AM1];
      const double H = prm.h1, mu2 = 2.0 * mu;
      double q0 = t0, q1 = t1, q2 = t2, dp = 0.0;   // principal deviatoric stresses, plastic multiplier
      double seq, f0, f1, f2;                        // equivalent stress and flow direction of the last evaluation
      double x1, x2, x3, l1, l2, l3, u1, u2, u3, dmax, qq, qa2;
      double i00, i01, i02, i11, i12, i22, z0, z1, z2, nz;   // A'^-1, z = A'^-1 n, n.z
      double tolp = 0.0;
      unsigned iters = 0;
      plastic = true;
      for (;;) {
        const double d1 = q0 - q1, d2 = q1 - q2, d3 = q0 - q2;
        dmax = fmax(fabs(d1), fmax(fabs(d2), fabs(d3)));
        const double idm = 1.0 / dmax;
        x1 = d1 * idm; x2 = d2 * idm; x3 = d3 * idm;
        const double a1 = fabs(x1), a2 = fabs(x2), a3 = fabs(x3);
        l1 = log(a1); l2 = log(a2); l3 = log(a3);
        u1 = hf_pow_am2(a1, l1, am2); u2 = hf_pow_am2(a2, l2, am2); u3 = hf_pow_am2(a3, l3, am2);
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
#pragma unroll
      for (int k = 0; k < 3; ++k) { n0[k] = rec[k]; n1[k] = rec[3 + k]; n2[k] = rec[6 + k]; }
#pragma unroll
      for (int c = 0; c < 6; ++c) { e[c] = rec[9 + c]; ep[c] = rec[15 + c]; }
      if (plastic) {
        // ---- 5. moduli of the returned state -----------------------------------------------------------------
        const double gden = mu2 * mu2 / (mu2 * nz + H);
        const double P00 = lambda + mu2 * i00 - gden * z0 * z0, P11 = lambda + mu2 * i11 - gden * z1 * z1, P22 = lambda + mu2 * i22 - gden * z2 * z2;
        const double P01 = lambda + mu2 * i01 - gden * z0 * z1, P02 = lambda + mu2 * i02 - gden * z0 * z2, P12 = lambda + mu2 * i12 - gden * z1 * z2;
        const double rs = qq * qa2 / dmax;   // q^(a-1) / max|d|
        // pair (0,1): difference d1, the other two d3 and d2; (1,2): d2, others d3 and d1; (0,2): d3, others d1 and -d2
        const double rho01 = rs * (u1 + 0.5 * hf_divided_difference(am1, x3, x2, l3, l2, u3, u2));
        const double rho12 = rs * (u2 + 0.5 * hf_divided_difference(am1, x3, x1, l3, l1, u3, u1));
        const double rho02 = rs * (u3 + 0.5 * hf_divided_difference(am1, x1, -x2, l1, l2, u1, u2));
        const double th01 = mu2 / (1.0 + mu2 * dp * rho01), th02 = mu2 / (1.0 + mu2 * dp * rho02), th12 = mu2 / (1.0 + mu2 * dp * rho12);

        // back to the global axes, Mandel vectors: E_i = n_i n_i, G_ij = (n_i n_j + n_j n_i) / sqrt(2)
        double E0[6], E1[6], E2[6];
#pragma unroll
        for (int I = 0; I < 6; ++I) {
          const double wE = I < 3 ? 1.0 : SQ2;
          E0[I] = wE * n0[SI[I]] * n0[SJ[I]]; E1[I] = wE * n1[SI[I]] * n1[SJ[I]]; E2[I] = wE * n2[SI[I]] * n2[SJ[I]];
        }
        {
          const double ktr = prm.kappa * tr;
          double sg[6];
#pragma unroll
          for (int I = 0; I < 6; ++I) {
            const double fl = dp * (f0 * E0[I] + f1 * E1[I] + f2 * E2[I]);   // dp n
            sg[I] = (I < 3 ? ktr : 0.0) + q0 * E0[I] + q1 * E1[I] + q2 * E2[I];
            e[I] -= fl;
            ep[I] += fl;
          }
          finish(sg, e, ep, p_n + dp);
        }
        double G01[6], G02[6], G12[6];
#pragma unroll
        for (int I = 0; I < 6; ++I) {
          const int M = SI[I], J = SJ[I];
          G01[I] = I < 3 ? SQ2 * n0[M] * n1[M] : n0[M] * n1[J] + n1[M] * n0[J];
          G02[I] = I < 3 ? SQ2 * n0[M] * n2[M] : n0[M] * n2[J] + n2[M] * n0[J];
          G12[I] = I < 3 ? SQ2 * n1[M] * n2[M] : n1[M] * n2[J] + n2[M] * n1[J];
        }
        double X0[6], X1[6], X2[6];
#pragma unroll
        for (int I = 0; I < 6; ++I) {
          X0[I] = P00 * E0[I] + P01 * E1[I] + P02 * E2[I];
          X1[I] = P01 * E0[I] + P11 * E1[I] + P12 * E2[I];
          X2[I] = P02 * E0[I] + P12 * E1[I] + P22 * E2[I];
        }
#pragma unroll
        for (int I = 0; I < 6; ++I)
#pragma unroll
          for (int K = I; K < 6; ++K) {
            const double v = E0[I] * X0[K] + E1[I] * X1[K] + E2[I] * X2[K] + th01 * G01[I] * G01[K] + th02 * G02[I] * G02[K] +
                             th12 * G12[I] * G12[K];
            rec[TRI21_AT(I, K)] = v;
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
      double sg[6];
      sg[0] = ltr + 2.0 * mu * e[0]; sg[1] = ltr + 2.0 * mu * e[1]; sg[2] = ltr + 2.0 * mu * e[2];
      sg[3] = 2.0 * mu * e[3]; sg[4] = 2.0 * mu * e[4]; sg[5] = 2.0 * mu * e[5];
      finish(sg, e, ep, p_n);
#pragma unroll
      for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int k = i; k < 6; ++k) rec[TRI21_AT(i, k)] = ((i < 3 && k < 3) ? lambda : 0.0) + ((i == k) ? 2.0 * mu : 0.0);
    }
    // stress, state and tangent (quadrature_map.py:322-324 asserts on all three)
    if (valid && !(fabs(cchk) <= 1.79769313486231570e308)) ++c_nan;
    wave_lds_sync();

    // ---- 7. coalesced stress store; 8. tangent, in output order from the staged records ------------------------
#include "tile_rows6_store.hpp"
#include "tile_tri21_store.hpp"
    wave_lds_sync();   // the LDS region is rewritten by the next tile
  }

  store_block_stats(stats, c_plastic, c_notconv, c_nan, c_maxit, red);
}

const void* hosford_kernel_fn() { return (const void*)hosford_kernel<0>; }

void hosford_launch(int tl, int grid, hipStream_t st, const LawParams& prm, int64_t cnt, const double* grad, const double* s0,
                    double* s1, int64_t ld, double* flux, double* ct, BlockStats* bs) {
  if (tl == 1) hipLaunchKernelGGL(hosford_kernel<1>, dim3(grid), dim3(BLOCK), 0, st, prm, cnt, grad, s0, s1, ld, flux, ct, bs);
  else hipLaunchKernelGGL(hosford_kernel<0>, dim3(grid), dim3(BLOCK), 0, st, prm, cnt, grad, s0, s1, ld, flux, ct, bs);
}

}  // namespace dxm
