// Plane-stress Hosford plasticity for gfx950: the fourth return mapping of the reference's demos/cvxpy/cvxpy_materials.py (:96-110)
// without a conic program.  Strain and stress are 3-vectors [xx, yy, sqrt(2) xy]; the update is
//   s_tr = C (eps - epsp_n),   s = argmin 1/2 (t - s_tr)^T C^-1 (t - s_tr) over phi(t) <= sig0,   epsp = eps - C^-1 s  (yielded points)
//   phi(t) = ((|t_I|^a + |t_II|^a + |t_I - t_II|^a) / 2)^(1/a),   t_I, t_II the principal values,   2 <= a <= 100
// with C the plane-stress stiffness (cvxpy_materials.py:16-18) and the plastic strain the law's one, hidden, state field.
//
// phi and C are isotropic: trial and answer are coaxial, and mean, dlt, tau, r, cs, sn, p1 >= p2 are formed as the polygon branch of
// plane_stress.hip forms them.  In A = (p1 + p2)/sqrt 2, B = (p1 - p2)/sqrt 2 the stiffness is diag(E/(1-nu), E/(1+nu)) and phi is even
// in both, so with x = A / sqrt(CA), y = B / sqrt(CB) the task is the Euclidean projection of T = (|x|, y) onto a convex set that is
// symmetric in both axes.  Its boundary in the first quadrant is P(th) = rho(th) (cos th, sin th), rho = sig0 / phi(direction), and
// the answer is the root of
//   g(th) = L (T.u - rho) - T.u_perp,   u = (cos th, sin th),  u_perp = (-sin th, cos th),  L = d ln phi / d th
// (this is (P - T).P' / (-rho): g(0) = -T_y <= 0 <= T_x = g(pi/2), L vanishes at both ends).  The root is unique (every stationary
// point of the distance on the arc is visible from an exterior T).  Iteration: Newton on th from the radial angle
// atan2(T_y, T_x), inside the bracket [0, pi/2], which every evaluation shrinks; a step that leaves the bracket, or that does not
// halve the step before the last, is replaced by the bracket's midpoint.  It ends when the step just taken is at most
// tol = max(rtol, 2^-49) radians, or g == 0; the iterate is evaluated after that step, so what is handed back is rho(th)(cos th, sin th)
// of the last angle: on the surface by construction, also at the cap (counted in n_not_converged).  max_iters is the number of steps.
//
// Powers are taken of the ratios r_k = |d_k| / max_k |d_k| in [0, 1]: one pow(r_k, a - 2) per term, then two multiplications give
// r^(a-1) and r^a.  No exponent overflows.  Whether a point yields is decided by phi of the trial, formed the same way; where the
// bounds m (1/2)^(1/a) <= phi <= m (3/2)^(1/a), m the largest of |t_I|, |t_II|, |t_I - t_II|, already decide, no power is formed.
//
// tangent = 1, yielded points: in the principal frame, with Cp = [[c11, c12], [c12, c11]], v = (s_I, s_II, s_I - s_II), f = phi(s),
//   n = J^T w, w_k = sign(v_k) (|v_k|/f)^(a-1) / 2;   H = J^T diag(h) J - (a-1)/f n n^T, h_k = (a-1) (|v_k|/f)^(a-2) / (2 f)
//   lambda = (t - s).n / (n.Cp n);   A = (Cp^-1 + lambda H)^-1;   D2 = A - (A n)(A n)^T / (n.A n);   G = E/(1+nu) (s_I - s_II)/(t_I - t_II)
// and D = Q (D2 (+) G) Q^T with Q the Mandel rotation of (cs, sn).  G takes its limit (D2_11 + D2_22 - 2 D2_12)/2 where r == 0
// exactly; t_I - t_II is taken as 2 r and s_I - s_II as rho d_3 with d_3 = sqrt 2 B_d, neither a difference of rounded principal values;
// towards t_I = t_II the quotient is formed from the stationarity condition instead (in the body).  The powers are those of the
// last evaluation: |v_k|/f = r_k / (S0/2)^(1/a).
//
// Every operation is individually rounded (no contraction), in the order written in the body, so that a restatement follows it
// (up to the pow, sin, cos and atan2 implementations).
//
// Mapping and memory as plane_stress.hip: one thread per point, one wave per tile of 64 points, 256-thread workgroups, grid-stride
// over the tiles, wave-private LDS ordered by wave_lds_sync(), one BlockStats record per workgroup.  A tile's strain and stress
// rows of 3 move through LDS by tile_rows3_load.hpp / tile_rows3_store.hpp; the plastic strain is three 8 B-per-lane SoA streams.
// The 9-wide tangent is never held per thread: tile_entries_store.hpp writes it in output order; with tangent = 0 an entry depends
// on its column only, with tangent = 1 each point stages its six distinct numbers in LDS.  A ragged last tile is bounded by lane in
// those three texts.
#include "plane_stress_hosford.hpp"

namespace dxm {

template <int TANGENT>
__global__ void __launch_bounds__(BLOCK)
plane_stress_hosford_kernel(const PshParams prm, const int64_t n, const double* __restrict__ grad, const double* __restrict__ s0,
                            double* __restrict__ s1, const int64_t ld, double* __restrict__ flux, double* __restrict__ ct,
                            BlockStats* __restrict__ stats) {
#pragma clang fp contract(off)
  constexpr int W = 9;   // tangent entries per point: the row-major 3 x 3
  __shared__ __attribute__((aligned(16))) double lds_all[WAVES_PER_BLOCK * PSH_LDS_PER_WAVE];
  __shared__ unsigned long long red[4 * WAVES_PER_BLOCK];
  static_assert(PSH_LDS_BYTES == sizeof(lds_all) + sizeof(red), "plane_stress_hosford.hpp states the LDS of the kernel");
  static_assert((WAVE * 3) % 2 == 0 && (WAVE * W) % 2 == 0 && (PSH_LDS_PER_WAVE * 8) % 16 == 0, "16 B accesses of whole tiles");

  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  double* stage = lds_all + wid * PSH_LDS_PER_WAVE;           // 64 x 3: strain in, stress out
  double2_t* stage2 = reinterpret_cast<double2_t*>(stage);
  double* rec = stage + WAVE * 3;                             // 64 x (D00, D01, D02, D11, D12, D22)

  const int64_t ntiles = (n + WAVE - 1) / WAVE;
  const int64_t tile_stride = (int64_t)gridDim.x * WAVES_PER_BLOCK;
  unsigned long long c_plastic = 0, c_notconv = 0, c_nan = 0, c_iters = 0;
  const double c11 = prm.p[PSH_C11], c12 = prm.p[PSH_C12], c33 = prm.p[PSH_C33];
  constexpr double R2 = 0.70710678118654752440;        // 1 / sqrt 2
  constexpr double HALF_PI = 1.57079632679489661923;

  for (int64_t tile = (int64_t)blockIdx.x * WAVES_PER_BLOCK + wid; tile < ntiles; tile += tile_stride) {
    const int64_t base = tile * WAVE;
    const int npts = (n - base) < WAVE ? (int)(n - base) : WAVE;
    const bool valid = lane < npts;
    const int64_t gi = base + lane;

    // ---- 1. the tile's strain rows into LDS; the plastic strain ------------------------------------------------------------------
#include "tile_rows3_load.hpp"
    double epn[3] = {0.0, 0.0, 0.0};
    if (valid) {
#pragma unroll
      for (int k = 0; k < 3; ++k) epn[k] = stream_load<3>(s0 + k * ld + gi);
    }
    wave_lds_sync();
    const double eps[3] = {stage[lane * 3 + 0], stage[lane * 3 + 1], stage[lane * 3 + 2]};
    wave_lds_sync();   // the staging region is reused for the stress below

    // ---- 2. the law --------------------------------------------------------------------------------------------------------
    const double ee[3] = {eps[0] - epn[0], eps[1] - epn[1], eps[2] - epn[2]};
    double sig[3], epo[3] = {epn[0], epn[1], epn[2]};
    double D[PSH_REC] = {c11, c12, 0.0, c11, 0.0, c33};
    const double E = prm.p[PSH_E], nu = prm.p[PSH_NU], sig0 = prm.p[PSH_SIG0];
    const double am2 = prm.p[PSH_AM2], inva = prm.p[PSH_INVA];
    const double t0 = c11 * ee[0] + c12 * ee[1], t1 = c12 * ee[0] + c11 * ee[1], t2 = c33 * ee[2];
    sig[0] = t0; sig[1] = t1; sig[2] = t2;
    const double mean = 0.5 * (t0 + t1), dlt = 0.5 * (t0 - t1), tau = t2 * R2;
    const double r = __builtin_sqrt(dlt * dlt + tau * tau);
    const double cs = r > 0.0 ? dlt / r : 1.0, sn = r > 0.0 ? tau / r : 0.0;
    const double p1 = mean + r, p2 = mean - r;
    // phi of the trial, as ratios to the largest of |p1|, |p2|, |p1 - p2| (all zero: 0 / 0, not yielded).  p1 - p2 is 2 r, formed
    // without rounding: (mean + r) - (mean - r) has lost it where r is small against mean
    // The sum of the three powers lies in [1, 3]: phi lies between m (1/2)^(1/a) and m (3/2)^(1/a), and the powers are formed only
    // where these bounds (widened by 4 eps: they never decide otherwise than phi itself would) leave the point open
    bool plastic = false;
    {
      const double a1 = __builtin_fabs(p1), a2 = __builtin_fabs(p2), a3 = 2.0 * r;
      const double m = __builtin_fmax(__builtin_fmax(a1, a2), a3);
      if (m * prm.p[PSH_KLO] > sig0 && m <= 1.7976931348623157e308) {
        plastic = true;
      } else if (!(m * prm.p[PSH_KHI] <= sig0)) {
        const double r1 = a1 / m, r2 = a2 / m, r3 = a3 / m;
        const double w1 = (pow(r1, am2) * r1) * r1, w2 = (pow(r2, am2) * r2) * r2, w3 = (pow(r3, am2) * r3) * r3;
        const double phi_tr = m * pow(0.5 * ((w1 + w2) + w3), inva);
        plastic = phi_tr > sig0 && phi_tr <= 1.7976931348623157e308;
      }
    }
    if (plastic) {
      const double sqA = prm.p[PSH_SQA], sqB = prm.p[PSH_SQB], a = prm.p[PSH_A], am1 = prm.p[PSH_AM1], tol = prm.p[PSH_TOL];
      const double x = ((p1 + p2) * R2) / sqA, Ty = ((2.0 * r) * R2) / sqB;   // y >= 0: p1 >= p2
      const double Tx = __builtin_fabs(x), sx = __builtin_copysign(1.0, x);
      double lo = 0.0, hi = HALF_PI, th = atan2(Ty, Tx), dx = HALF_PI, dxold = HALF_PI;
      double c, s, d1, d2, d3, m, u1, u2, u3, v1, v2, S0, kap, rho;
      int it = 0;
      for (;;) {
        c = cos(th); s = sin(th);
        // the direction's principal values and their derivatives in th
        const double Ad = sx * (c * sqA), Bd = s * sqB;
        d1 = (Ad + Bd) * R2; d2 = (Ad - Bd) * R2; d3 = (2.0 * Bd) * R2;   // d1 - d2, without its cancellation
        const double Ap = -(sx * (s * sqA)), Bp = c * sqB;
        const double e1 = (Ap + Bp) * R2, e2 = (Ap - Bp) * R2, e3 = (2.0 * Bp) * R2;
        const double a1 = __builtin_fabs(d1), a2 = __builtin_fabs(d2), a3 = __builtin_fabs(d3);
        m = __builtin_fmax(__builtin_fmax(a1, a2), a3);
        const double r1 = a1 / m, r2 = a2 / m, r3 = a3 / m;
        u1 = pow(r1, am2); u2 = pow(r2, am2); u3 = pow(r3, am2);      // r^(a-2)
        v1 = u1 * r1; v2 = u2 * r2;                                   // r^(a-1)
        const double v3 = u3 * r3;
        S0 = (v1 * r1 + v2 * r2) + v3 * r3;                           // sum r^a
        const double N = (__builtin_copysign(v1, d1) * e1 + __builtin_copysign(v2, d2) * e2) + __builtin_copysign(v3, d3) * e3;
        const double L = N / (m * S0);
        const double K2 = ((u1 * (e1 * e1) + u2 * (e2 * e2)) + u3 * (e3 * e3)) / ((m * m) * S0);
        const double Lp = (am1 * K2 - 1.0) - a * (L * L);
        kap = pow(0.5 * S0, inva);
        rho = sig0 / (m * kap);
        const double Tu = Tx * c + Ty * s, Tp = Ty * c - Tx * s;
        const double gap = Tu - rho;
        const double g = L * gap - Tp;
        if ((it > 0 && __builtin_fabs(dx) <= tol) || g == 0.0) break;
        if (it >= prm.maxit) { ++c_notconv; break; }
        const double dg = (Lp * gap + L * (Tp + rho * L)) + Tu;
        if (g < 0.0) lo = th; else hi = th;
        const double newton = th - g / dg;
        const bool use = (newton >= lo && newton <= hi) && (__builtin_fabs(2.0 * g) <= __builtin_fabs(dxold * dg));
        const double thn = use ? newton : 0.5 * (lo + hi);
        dxold = dx;
        dx = thn - th;
        th = thn;
        ++it;
      }
      c_iters = (unsigned long long)it > c_iters ? (unsigned long long)it : c_iters;
      // the principal stresses of the last angle, put back as the polygon branch of plane_stress.hip does
      const double b1 = rho * d1, b2 = rho * d2, b3 = rho * d3;   // s_I, s_II, s_I - s_II
      const double sm = 0.5 * (b1 + b2), sr = 0.5 * b3;
      sig[0] = sm + sr * cs;
      sig[1] = sm - sr * cs;
      sig[2] = (sr * sn) / R2;
      // C^-1 s = (1/E) [[1, -nu, 0], [-nu, 1, 0], [0, 0, 1 + nu]] s
      epo[0] = eps[0] - (sig[0] - nu * sig[1]) / E;
      epo[1] = eps[1] - (sig[1] - nu * sig[0]) / E;
      epo[2] = eps[2] - ((1.0 + nu) * sig[2]) / E;
      if constexpr (TANGENT) {
        // (|v_k|/f)^(a-1) = r_k^(a-1) kap / (S0/2), (|v_k|/f)^(a-2) = r_k^(a-2) kap^2 / (S0/2); f = sig0 (the point is on the surface)
        const double hs = 0.5 * S0;
        const double k1 = kap / hs, k2 = (kap * kap) / hs;
        const double r3 = __builtin_fabs(d3) / m;
        const double w1 = 0.5 * (__builtin_copysign(v1, d1) * k1), w2 = 0.5 * (__builtin_copysign(v2, d2) * k1);
        const double w3 = 0.5 * (__builtin_copysign(u3 * r3, d3) * k1);
        const double hf = am1 / (2.0 * sig0);
        const double h1 = hf * (u1 * k2), h2 = hf * (u2 * k2), h3 = hf * (u3 * k2);
        const double n1 = w1 + w3, n2 = w2 - w3;
        const double af = am1 / sig0;
        const double H11 = (h1 + h3) - af * (n1 * n1), H22 = (h2 + h3) - af * (n2 * n2), H12 = -h3 - af * (n1 * n2);
        const double q1 = c11 * n1 + c12 * n2, q2 = c12 * n1 + c11 * n2;   // Cp n
        const double lam = ((p1 - b1) * n1 + (p2 - b2) * n2) / (n1 * q1 + n2 * q2);
        const double M11 = 1.0 / E + lam * H11, M22 = 1.0 / E + lam * H22, M12 = lam * H12 - nu / E;
        const double det = M11 * M22 - M12 * M12;
        const double A11 = M22 / det, A22 = M11 / det, A12 = -(M12 / det);
        const double z1 = A11 * n1 + A12 * n2, z2 = A12 * n1 + A22 * n2;   // A n
        const double den = n1 * z1 + n2 * z2;
        const double D11 = A11 - (z1 * z1) / den, D22 = A22 - (z2 * z2) / den, D12 = A12 - (z1 * z2) / den;
        const double gam = 0.25 * ((D11 + D22) - 2.0 * D12);
        const double alp = 0.25 * ((D11 + D22) + 2.0 * D12), bet = 0.25 * (D11 - D22);
        // G = CB (s_I - s_II) / (t_I - t_II) = CB rho sin th / T_y.  The angle is accurate to an absolute 1e-16, so towards the axis
        // th -> 0 (t_I -> t_II) the quotient of the two small numbers is not.  There g(th) = 0 gives T_y / sin th = ((L / sin th)
        // (T.u - rho) + T_x) / cos th, a smooth even function of th, with L / sin th free of cancellation: the two near-equal powers
        // are 1 and (1 - dl)^(a-1), dl = 2 B_d / (|A_d| + B_d); (1 - (1 - dl)^(a-1)) / dl is the binomial series to the eighth power
        // where (a-1) dl < 0.05 (what it leaves out is below 0.05^8 / 9!), the difference of the loop's own powers beyond (its
        // rounding, (a-1) 1e-16 / 0.05, is 2e-13 at most).  Used where dl < 1/2 (B_d < |A_d| / 3: then |d_3| is not the largest of the
        // three); r == 0 exactly takes the limit 2 gam
        const double aA = c * sqA, Bd = s * sqB, Bp = c * sqB, sum = aA + Bd;
        const double dl = (2.0 * Bd) / sum;
        double G = 2.0 * gam;
        if (r > 0.0) {
          if (dl < 0.5) {
            double q;   // (1 - (1 - dl)^(a-1)) / dl
            if (am1 * dl < 0.05) {
              q = 1.0;
#pragma unroll
              for (int k = 8; k >= 1; --k) q = 1.0 - (((am1 - (double)k) * dl) / (double)(k + 1)) * q;
              q = am1 * q;
            } else {
              q = (1.0 - __builtin_fmin(v1, v2)) / dl;
            }
            const double ks = (2.0 * sqB) / sum;                                   // dl / sin th = r_3 / sin th
            const double Ns = (Bp * (q * ks) - sqA * (v1 + v2)) * R2 + (u3 * ks) * ((2.0 * Bp) * R2);
            const double Ls = Ns / (m * S0);
            G = prm.p[PSH_CB] * ((rho * c) / (Ls * ((Tx * c + Ty * s) - rho) + Tx));
          } else {
            G = prm.p[PSH_CB] * (b3 / (2.0 * r));
          }
        }
        // Q (D2 (+) G) Q^T: q1,2 = (u +- w)/2, u = [1, 1, 0], w = [cs, -cs, sqrt2 sn], q3 = [-sn/sqrt2, sn/sqrt2, cs]
        const double cc = cs * cs, ss = sn * sn, sc = sn * cs;
        const double gs = 0.5 * (G * ss);
        D[0] = ((alp + 2.0 * (bet * cs)) + gam * cc) + gs;
        D[1] = (alp - gam * cc) - gs;
        D[2] = ((bet * sn + gam * sc) / R2) - (G * sc) * R2;
        D[3] = ((alp - 2.0 * (bet * cs)) + gam * cc) + gs;
        D[4] = ((bet * sn - gam * sc) / R2) + (G * sc) * R2;
        D[5] = 2.0 * (gam * ss) + G * cc;
      }
    }
    if (valid && plastic) ++c_plastic;
    // a non-finite stress, state or tangent entry: v * 0 is NaN exactly for those
    double z = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) z = __builtin_fma(sig[k], 0.0, __builtin_fma(epo[k], 0.0, z));
    if constexpr (TANGENT) {
#pragma unroll
      for (int k = 0; k < PSH_REC; ++k) z = __builtin_fma(D[k], 0.0, z);
    }
    if (valid && !(z == 0.0)) ++c_nan;

    stage[lane * 3 + 0] = sig[0];
    stage[lane * 3 + 1] = sig[1];
    stage[lane * 3 + 2] = sig[2];
    if constexpr (TANGENT) {
#pragma unroll
      for (int k = 0; k < PSH_REC; ++k) rec[lane * PSH_REC + k] = D[k];
    }
    if (valid) {   // an elastic point writes back the bits it read
#pragma unroll
      for (int k = 0; k < 3; ++k) stream_store<1>(s1 + k * ld + gi, epo[k]);
    }
    wave_lds_sync();

    // ---- 3. the stress rows, as the strain came in ---------------------------------------------------------------------------
#include "tile_rows3_store.hpp"
    // ---- 4. the tangent in output order: entry e of the tile belongs to point e / 9, column e % 9 of the row-major 3 x 3 ----
    auto entry = [&](int e) -> double {
      const int p = e / W, col = e - p * W;
      if constexpr (TANGENT) {
        return rec[p * PSH_REC + sym3_slot(col)];
      } else {
        return (col == 0 || col == 4) ? c11 : ((col == 1 || col == 3) ? c12 : (col == 8 ? c33 : 0.0));
      }
    };
#include "tile_entries_store.hpp"
    wave_lds_sync();   // the LDS region is rewritten by the next tile
  }

  store_block_stats(stats, c_plastic, c_notconv, c_nan, c_iters, red);
}

const void* plane_stress_hosford_kernel_fn() { return (const void*)plane_stress_hosford_kernel<0>; }

void plane_stress_hosford_launch(int tangent, int grid, hipStream_t st, const PshParams& prm, int64_t cnt, const double* grad,
                                 const double* s0, double* s1, int64_t ld, double* flux, double* ct, BlockStats* bs) {
  if (tangent) hipLaunchKernelGGL((plane_stress_hosford_kernel<1>), dim3(grid), dim3(BLOCK), 0, st, prm, cnt, grad, s0, s1, ld, flux, ct, bs);
  else hipLaunchKernelGGL((plane_stress_hosford_kernel<0>), dim3(grid), dim3(BLOCK), 0, st, prm, cnt, grad, s0, s1, ld, flux, ct, bs);
}

}  // namespace dxm
