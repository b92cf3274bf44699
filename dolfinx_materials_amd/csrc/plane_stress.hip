// Plane-stress return mapping onto a convex yield set for gfx950: the perfectly plastic laws of the reference's
// demos/cvxpy/cvxpy_materials.py without a conic program.  Strain and stress are 3-vectors [xx, yy, sqrt(2) xy]; the update is
//   s_tr = C (eps - epsp_n),   s = argmin 1/2 (t - s_tr)^T C^-1 (t - s_tr) over t in K,   epsp = eps - C^-1 s  (yielded points)
// with C the plane-stress stiffness (cvxpy_materials.py:16-18) and the plastic strain the law's one, hidden, state field.
//
//   quadratic (PlaneStressvonMises, :89-93): K = {s^T Q s <= sig0^2}, Q = [[1, -1/2, 0], [-1/2, 1, 0], [0, 0, q]].  In the basis
//     a = (s0 + s1)/sqrt 2, b = (s0 - s1)/sqrt 2, c = s2 both C = diag(E/(1-nu), E/(1+nu), E/(1+nu)) and Q = diag(1/2, 3/2, q) are
//     diagonal: s_i = t_i / (1 + l k_i), k_i = Q_i C_i, with l >= 0 the root of g(l) = sum Q_i t_i^2 / (1 + l k_i)^2 - sig0^2.  g is
//     convex and decreasing: Newton from the lower bound l = (sqrt(t^T Q t)/sig0 - 1)/max k_i is monotone.  It ends on the residual
//     sqrt(sum ...) - sig0 <= tol; the step computed from that last residual is still taken.  A point at the cap is counted.
//   polygon (Rankine :54-65, L1Rankine :68-86): K = {n_k . (sI, sII) <= d_k}, at most four half-planes in the plane of the
//     principal stresses, closed under their exchange.  Trial and answer are coaxial; the candidates are the projections onto the
//     rows' lines (admissible if the other rows hold) and the polygon's vertices (found on the host); the nearest one in the
//     energy norm of the principal values is the answer.  No iteration.
//
// Every operation is individually rounded (no contraction), in the order written in the body, so that a restatement follows it.
//
// Mapping and memory as heat_transfer.hip: one thread per point, one wave per tile of 64 points, 256-thread workgroups, grid-stride
// over the tiles, wave-private LDS ordered by wave_lds_sync(), one BlockStats record per workgroup.  A tile's strain and stress
// rows of 3 move through LDS by tile_rows3_load.hpp / tile_rows3_store.hpp; the plastic strain is three 8 B-per-lane SoA streams.
// The 9-wide tangent is never held per thread: tile_entries_store.hpp writes it in output order (a tile's is 4608 B and starts on
// a multiple of 512 B: every 128 B line is written whole); with tangent = 0 an entry depends on its column only, with tangent = 1
// each point stages its six distinct numbers in LDS.  A ragged last tile is bounded by lane in those three texts.
#include "plane_stress.hpp"

namespace dxm {

template <int SURFACE, int TANGENT>
__global__ void __launch_bounds__(BLOCK)
plane_stress_kernel(const PsParams prm, const int64_t n, const double* __restrict__ grad, const double* __restrict__ s0,
                    double* __restrict__ s1, const int64_t ld, double* __restrict__ flux, double* __restrict__ ct,
                    BlockStats* __restrict__ stats) {
#pragma clang fp contract(off)
  static_assert(SURFACE == PS_QUADRATIC || TANGENT == 0, "the polygonal law writes the elastic tangent only");
  constexpr int W = 9;   // tangent entries per point: the row-major 3 x 3
  __shared__ __attribute__((aligned(16))) double lds_all[WAVES_PER_BLOCK * PS_LDS_PER_WAVE];
  __shared__ unsigned long long red[4 * WAVES_PER_BLOCK];
  static_assert(PS_LDS_BYTES == sizeof(lds_all) + sizeof(red), "plane_stress.hpp states the LDS of the kernel");
  static_assert((WAVE * 3) % 2 == 0 && (WAVE * W) % 2 == 0 && (PS_LDS_PER_WAVE * 8) % 16 == 0, "16 B accesses of whole tiles");

  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  double* stage = lds_all + wid * PS_LDS_PER_WAVE;            // 64 x 3: strain in, stress out
  double2_t* stage2 = reinterpret_cast<double2_t*>(stage);
  double* rec = stage + WAVE * 3;                             // 64 x (D00, D01, D02, D11, D12, D22)

  const int64_t ntiles = (n + WAVE - 1) / WAVE;
  const int64_t tile_stride = (int64_t)gridDim.x * WAVES_PER_BLOCK;
  unsigned long long c_plastic = 0, c_notconv = 0, c_nan = 0, c_iters = 0;
  const double c11 = prm.p[PS_C11], c12 = prm.p[PS_C12], c33 = prm.p[PS_C33];
  constexpr double R2 = 0.70710678118654752440;   // 1 / sqrt 2

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
      for (int a = 0; a < 3; ++a) epn[a] = stream_load<3>(s0 + a * ld + gi);
    }
    wave_lds_sync();
    const double eps[3] = {stage[lane * 3 + 0], stage[lane * 3 + 1], stage[lane * 3 + 2]};
    wave_lds_sync();   // the staging region is reused for the stress below

    // ---- 2. the law --------------------------------------------------------------------------------------------------------
    const double ee[3] = {eps[0] - epn[0], eps[1] - epn[1], eps[2] - epn[2]};
    double sig[3], epo[3] = {epn[0], epn[1], epn[2]};
    double D[PS_REC] = {c11, c12, 0.0, c11, 0.0, c33};
    bool plastic = false;
    if constexpr (SURFACE == PS_QUADRATIC) {
      const double CA = prm.p[PS_CA], CB = prm.p[PS_CB], QC = prm.p[PS_QC], sig0 = prm.p[PS_SIG0];
      const double ta = CA * ((ee[0] + ee[1]) * R2), tb = CB * ((ee[0] - ee[1]) * R2), tc = CB * ee[2];
      const double seq = __builtin_sqrt((0.5 * (ta * ta) + 1.5 * (tb * tb)) + QC * (tc * tc));
      plastic = seq > sig0 && seq <= 1.7976931348623157e308;
      double sa = ta, sb = tb, sc = tc;
      if (plastic) {
        const double ka = 0.5 * CA, kb = 1.5 * CB, kc = QC * CB;
        double lam = (seq / sig0 - 1.0) / prm.p[PS_KMAX];
        double da, db, dc;
        int it = 0;
        for (;;) {
          da = 1.0 / (1.0 + lam * ka); db = 1.0 / (1.0 + lam * kb); dc = 1.0 / (1.0 + lam * kc);
          sa = ta * da; sb = tb * db; sc = tc * dc;
          const double qa = 0.5 * (sa * sa), qb = 1.5 * (sb * sb), qc = QC * (sc * sc);
          const double S = (qa + qb) + qc;
          const bool conv = (__builtin_sqrt(S) - sig0) <= prm.p[PS_TOL];
          if (!conv && it >= prm.maxit) { ++c_notconv; break; }
          lam = lam + (S - prm.p[PS_SIG0SQ]) / (2.0 * ((qa * (ka * da) + qb * (kb * db)) + qc * (kc * dc)));
          if (conv) {   // the step of the last residual is taken: the stress is formed at the new multiplier
            da = 1.0 / (1.0 + lam * ka); db = 1.0 / (1.0 + lam * kb); dc = 1.0 / (1.0 + lam * kc);
            sa = ta * da; sb = tb * db; sc = tc * dc;
            break;
          }
          ++it;
        }
        c_iters = (unsigned long long)it > c_iters ? (unsigned long long)it : c_iters;
        // C^-1 s in the basis, rotated back
        const double xa = sa / CA, xb = sb / CB, xc = sc / CB;
        epo[0] = eps[0] - (xa + xb) * R2;
        epo[1] = eps[1] - (xa - xb) * R2;
        epo[2] = eps[2] - xc;
        if constexpr (TANGENT) {
          // A - (A n)(A n)^T / (n^T A n), A = diag(C_i / (1 + l k_i)), n = Q s, in the basis; then rotated back
          const double Aa = CA * da, Ab = CB * db, Ac = CB * dc;
          const double na = 0.5 * sa, nb = 1.5 * sb, nc = QC * sc;
          const double va = Aa * na, vb = Ab * nb, vc = Ac * nc;
          const double den = (na * va + nb * vb) + nc * vc;
          const double Taa = Aa - (va * va) / den, Tbb = Ab - (vb * vb) / den, Tcc = Ac - (vc * vc) / den;
          const double Tab = -((va * vb) / den), Tac = -((va * vc) / den), Tbc = -((vb * vc) / den);
          const double h = 0.5 * (Taa + Tbb);
          D[0] = h + Tab;
          D[1] = 0.5 * (Taa - Tbb);
          D[2] = (Tac + Tbc) * R2;
          D[3] = h - Tab;
          D[4] = (Tac - Tbc) * R2;
          D[5] = Tcc;
        }
      }
      sig[0] = (sa + sb) * R2;
      sig[1] = (sa - sb) * R2;
      sig[2] = sc;
    } else {
      const double E = prm.p[PS_E], nu = prm.p[PS_NU];
      const double t0 = c11 * ee[0] + c12 * ee[1], t1 = c12 * ee[0] + c11 * ee[1], t2 = c33 * ee[2];
      sig[0] = t0; sig[1] = t1; sig[2] = t2;
      const double mean = 0.5 * (t0 + t1), dlt = 0.5 * (t0 - t1), tau = t2 * R2;
      const double r = __builtin_sqrt(dlt * dlt + tau * tau);
      const double cs = r > 0.0 ? dlt / r : 1.0, sn = r > 0.0 ? tau / r : 0.0;
      const double p1 = mean + r, p2 = mean - r;
      double over = 0.0;   // the largest n . p / d: > 1 where a row is violated
#pragma unroll
      for (int k = 0; k < PS_MAX_PLANES; ++k) {
        if (k < prm.planes) {
          const double* pl = prm.p + PS_PLANE + k * PS_PLANE_REC;
          const double ratio = (pl[PL_N1] * p1 + pl[PL_N2] * p2) / pl[PL_D];
          over = ratio > over ? ratio : over;
        }
      }
      plastic = over > 1.0 && over <= 1.7976931348623157e308;
      if (plastic) {
        const double nu2 = 2.0 * nu;
        double best = __builtin_inf(), b1 = p1 / over, b2 = p2 / over;   // (no candidate admissible: the radial scaling, which is)
        auto nearer = [&](double x, double y, bool adm) {
          const double dx = x - p1, dy = y - p2;
          const double dist = (dx * dx + dy * dy) - (nu2 * dx) * dy;
          if (adm && dist < best) { best = dist; b1 = x; b2 = y; }
        };
#pragma unroll
        for (int k = 0; k < PS_MAX_PLANES; ++k) {
          if (k < prm.planes) {
            const double* pl = prm.p + PS_PLANE + k * PS_PLANE_REC;
            const double step = ((pl[PL_N1] * p1 + pl[PL_N2] * p2) - pl[PL_D]) / pl[PL_NW];
            const double x = p1 - pl[PL_W1] * step, y = p2 - pl[PL_W2] * step;
            bool adm = true;
#pragma unroll
            for (int j = 0; j < PS_MAX_PLANES; ++j) {
              if (j != k && j < prm.planes) {
                const double* pj = prm.p + PS_PLANE + j * PS_PLANE_REC;
                adm = adm && ((pj[PL_N1] * x + pj[PL_N2] * y) - pj[PL_D] <= pj[PL_SLACK]);
              }
            }
            nearer(x, y, adm);
          }
        }
#pragma unroll
        for (int v = 0; v < PS_MAX_VERTICES; ++v) {
          if (v < prm.vertices) nearer(prm.p[PS_VERTEX + 2 * v], prm.p[PS_VERTEX + 2 * v + 1], true);
        }
        const double sm = 0.5 * (b1 + b2), sr = 0.5 * (b1 - b2);
        sig[0] = sm + sr * cs;
        sig[1] = sm - sr * cs;
        sig[2] = (sr * sn) / R2;
        // C^-1 s = (1/E) [[1, -nu, 0], [-nu, 1, 0], [0, 0, 1 + nu]] s
        epo[0] = eps[0] - (sig[0] - nu * sig[1]) / E;
        epo[1] = eps[1] - (sig[1] - nu * sig[0]) / E;
        epo[2] = eps[2] - ((1.0 + nu) * sig[2]) / E;
      }
    }
    if (valid && plastic) ++c_plastic;
    // a non-finite stress, state or tangent entry: v * 0 is NaN exactly for those
    double z = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) z = __builtin_fma(sig[a], 0.0, __builtin_fma(epo[a], 0.0, z));
    if constexpr (TANGENT) {
#pragma unroll
      for (int a = 0; a < PS_REC; ++a) z = __builtin_fma(D[a], 0.0, z);
    }
    if (valid && !(z == 0.0)) ++c_nan;

    stage[lane * 3 + 0] = sig[0];
    stage[lane * 3 + 1] = sig[1];
    stage[lane * 3 + 2] = sig[2];
    if constexpr (TANGENT) {
#pragma unroll
      for (int a = 0; a < PS_REC; ++a) rec[lane * PS_REC + a] = D[a];
    }
    if (valid) {   // an elastic point writes back the bits it read
#pragma unroll
      for (int a = 0; a < 3; ++a) stream_store<1>(s1 + a * ld + gi, epo[a]);
    }
    wave_lds_sync();

    // ---- 3. the stress rows, as the strain came in ---------------------------------------------------------------------------
#include "tile_rows3_store.hpp"
    // ---- 4. the tangent in output order: entry e of the tile belongs to point e / 9, column e % 9 of the row-major 3 x 3 ----
    auto entry = [&](int e) -> double {
      const int p = e / W, col = e - p * W;
      if constexpr (TANGENT) {
        return rec[p * PS_REC + sym3_slot(col)];
      } else {
        return (col == 0 || col == 4) ? c11 : ((col == 1 || col == 3) ? c12 : (col == 8 ? c33 : 0.0));
      }
    };
#include "tile_entries_store.hpp"
    wave_lds_sync();   // the LDS region is rewritten by the next tile
  }

  store_block_stats(stats, c_plastic, c_notconv, c_nan, c_iters, red);
}

const void* plane_stress_quadratic_kernel_fn() { return (const void*)plane_stress_kernel<PS_QUADRATIC, 0>; }
const void* plane_stress_polygon_kernel_fn() { return (const void*)plane_stress_kernel<PS_POLYGON, 0>; }

void plane_stress_launch(int surface, int tangent, int grid, hipStream_t st, const PsParams& prm, int64_t cnt, const double* grad,
                         const double* s0, double* s1, int64_t ld, double* flux, double* ct, BlockStats* bs) {
#define DXM_LAUNCH_PS(S, T) \
  hipLaunchKernelGGL((plane_stress_kernel<S, T>), dim3(grid), dim3(BLOCK), 0, st, prm, cnt, grad, s0, s1, ld, flux, ct, bs)
  if (surface == PS_POLYGON) DXM_LAUNCH_PS(PS_POLYGON, 0);
  else if (tangent) DXM_LAUNCH_PS(PS_QUADRATIC, 1);
  else DXM_LAUNCH_PS(PS_QUADRATIC, 0);
#undef DXM_LAUNCH_PS
}

}  // namespace dxm
