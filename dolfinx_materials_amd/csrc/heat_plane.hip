// The two heat-transfer laws of heat_transfer.hip under a two-dimensional hypothesis (the reference's heat-transfer demos load
// theirs with hypothesis="plane_strain" and register a 2-wide grad(T)): gradient g = [dT/dx, dT/dy], flux j (2), external state
// variable T.  The arithmetic is that of heat_transfer.hip, operation for operation and in its order, on the same HeatParams: the
// results equal those of the 3-wide laws on [g0, g1, 0] bit for bit, n_nan included (a non-finite -k or slope shows in an entry that
// exists here too).
//
// Mapping: one thread per point, one wave per tile of 64 points, 256-thread workgroups, grid-stride over the tiles; no workgroup
// barrier inside the tile loop; one BlockStats record per workgroup.
// Memory: a gradient or flux row is 16 B and 16 B aligned, so each lane moves its own row with one 16 B access and the wave covers
// 1024 contiguous bytes: no staging.  T and the enthalpy are 8 B per lane.  The tangent is never held per thread: each point stages
// (-k, dj/dT[0..1], c) in wave-private LDS and tile_entries_store.hpp writes the 6 / 7 numbers per point in output order.  A tile's
// tangent is 3072 / 3584 B and starts on a multiple of that, so every 128 B line is written whole; the two structural zeros of -k I
// are written (the layout is the reference's jacobian_flatten).  A ragged last tile is bounded by lane.
//
// SRC = HP_SRC_NODAL: no gradient or temperature array exists.  Each lane evaluates T and grad(T) at its Gauss point from the nodal
// temperature with scalar_point(), the text the stand-alone scalar_gradient_kernel runs too, so the two routes agree bit for bit.
// What a lane reads per point are the mesh tables (a few hundred bytes, vector L1), its cell's indices and the nodal values they
// name: lanes of one cell ask for the same lines.
#include "heat_plane.hpp"

namespace dxm {

// Per point (xi: reference coordinates):
//   J[a][d] = sum_v X_v[a] gdphi[q][v][d]    dX_a / dxi_d from the nv vertices of the cell
//   r[d]    = sum_m T_m dphi[q][m][d]        dT / dxi_d from the nd dofs of the cell;   T = sum_m T_m phi[q][m]
//   g[a]    = sum_d r[d] Ji[d][a]            Ji the 2 x 2 cofactor inverse of J
// Every operation individually rounded, sums in index order from 0.0.
__device__ __forceinline__ void scalar_point(const ScalarSource& s, int64_t point, double& T, double& g0, double& g1) {
#pragma clang fp contract(off)
  const int64_t cell = point / s.nqp;
  const int q = (int)(point - cell * s.nqp);
  double J00 = 0.0, J01 = 0.0, J10 = 0.0, J11 = 0.0;
  {
    const int32_t* vs = s.conn + cell * s.nv;
    const double* tab = s.gdphi + (int64_t)q * s.nv * 2;
    for (int v = 0; v < s.nv; ++v) {
      const int64_t vert = vs[v];
      const double t0 = tab[2 * v], t1 = tab[2 * v + 1];
      const double X0 = s.coords[3 * vert], X1 = s.coords[3 * vert + 1];
      J00 = J00 + X0 * t0; J01 = J01 + X0 * t1;
      J10 = J10 + X1 * t0; J11 = J11 + X1 * t1;
    }
  }
  double val = 0.0, r0 = 0.0, r1 = 0.0;
  {
    const int32_t* dofs = s.dofmap + cell * s.nd;
    const double* tab = s.dphi + (int64_t)q * s.nd * 2;
    const double* ptab = s.phi + (int64_t)q * s.nd;
#pragma unroll 2
    for (int m = 0; m < s.nd; ++m) {
      const double Tm = s.t[dofs[m]];
      val = val + Tm * ptab[m];
      r0 = r0 + Tm * tab[2 * m];
      r1 = r1 + Tm * tab[2 * m + 1];
    }
  }
  const double idet = 1.0 / (J00 * J11 - J01 * J10);
  const double i00 = J11 * idet, i01 = -J01 * idet, i10 = -J10 * idet, i11 = J00 * idet;
  T = val;
  g0 = r0 * i00 + r1 * i10;
  g1 = r0 * i01 + r1 * i11;
}

__global__ void __launch_bounds__(SCALAR_GRAD_BLOCK)
scalar_gradient_kernel(const ScalarSource s, const int64_t npts, double* __restrict__ grad, double* __restrict__ value) {
  const int64_t gid = (int64_t)blockIdx.x * SCALAR_GRAD_BLOCK + threadIdx.x;
  if (gid >= npts) return;   // a ragged last block: a lane writes its own row or nothing
  double T, g0, g1;
  scalar_point(s, s.point0 + gid, T, g0, g1);
  reinterpret_cast<double2_t*>(grad)[gid] = double2_t{g0, g1};
  if (value) value[gid] = T;
}

template <int LAW, int SRC>
__global__ void __launch_bounds__(BLOCK)
heat_plane_kernel(const HeatParams prm, const int64_t n, const double* __restrict__ grad, const double t_uniform,
                  const double* __restrict__ tfield, const ScalarSource src, double* __restrict__ enthalpy, double* __restrict__ flux,
                  double* __restrict__ ct, BlockStats* __restrict__ stats) {
#pragma clang fp contract(off)
  constexpr int W = HP_WIDTH[LAW];
  __shared__ __attribute__((aligned(16))) double lds_all[WAVES_PER_BLOCK * HP_LDS_PER_WAVE];
  __shared__ unsigned long long red[4 * WAVES_PER_BLOCK];
  static_assert(HP_LDS_BYTES == sizeof(lds_all) + sizeof(red), "heat_plane.hpp states the LDS of the kernel");
  static_assert((WAVE * W) % 2 == 0 && (WAVE * W * 8) % 128 == 0, "a tile's tangent is whole 128 B lines, written as 16 B pairs");

  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  double* rec = lds_all + wid * HP_LDS_PER_WAVE;              // 64 x (-k, dj/dT[0..1], c)

  const int64_t ntiles = (n + WAVE - 1) / WAVE;
  const int64_t tile_stride = (int64_t)gridDim.x * WAVES_PER_BLOCK;
  unsigned long long c_nan = 0;

  for (int64_t tile = (int64_t)blockIdx.x * WAVES_PER_BLOCK + wid; tile < ntiles; tile += tile_stride) {
    const int64_t base = tile * WAVE;
    const int npts = (n - base) < WAVE ? (int)(n - base) : WAVE;
    const bool valid = lane < npts;
    const int64_t gi = base + lane;

    // ---- 1. the point's gradient row and temperature ---------------------------------------------------------------------
    double T = t_uniform;
    double g[2] = {0.0, 0.0};
    if constexpr (SRC == HP_SRC_NODAL) {
      if (valid) scalar_point(src, src.point0 + gi, T, g[0], g[1]);
    } else {
      if (valid) {
        const double2_t row = stream_load<2>(reinterpret_cast<const double2_t*>(grad) + gi);
        g[0] = row.x;
        g[1] = row.y;
        if (tfield) T = stream_load<3>(tfield + gi);
      }
    }

    // ---- 2. the law (heat_transfer.hip, step 2) --------------------------------------------------------------------------
    double nk, slope, c = 0.0, h = 0.0;   // -k, the factor of g in dj/dT
    if constexpr (LAW == HT_STATIONARY) {
      const double k = 1.0 / (prm.p[HT_A] + prm.p[HT_B] * T);
      nk = -k;
      slope = (prm.p[HT_B] * k) * k;
    } else {
      const double dT = T - prm.p[HT_TS];
      const bool solid = T < prm.p[HT_TS], liquid = T > prm.p[HT_TL];
      const double k_tr = prm.p[HT_KS] + (prm.p[HT_DK] * dT) / prm.p[HT_TSM];
      const double h_tr = prm.p[HT_CSTS] + prm.p[HT_CTR] * dT;
      const double h_liq = ((prm.p[HT_CL] * (T - prm.p[HT_TL]) + prm.p[HT_DHSL]) + prm.p[HT_CSTS]) + prm.p[HT_HL3];
      const double h_sol = prm.p[HT_CS] * T;
      const double k = solid ? prm.p[HT_KS] : (liquid ? prm.p[HT_KL] : k_tr);
      c = solid ? prm.p[HT_CS] : (liquid ? prm.p[HT_CL] : prm.p[HT_CTR]);
      h = solid ? h_sol : (liquid ? h_liq : h_tr);
      slope = (solid || liquid) ? 0.0 : prm.p[HT_NSLOPE];
      nk = -k;
    }
    const double j[2] = {nk * g[0], nk * g[1]};
    const double dj[2] = {slope * g[0], slope * g[1]};
    // a non-finite flux, state or tangent entry: v * 0 is NaN exactly for those
    double z = 0.0;
#pragma unroll
    for (int a = 0; a < 2; ++a) z = __builtin_fma(j[a], 0.0, __builtin_fma(dj[a], 0.0, z));
    z = __builtin_fma(nk, 0.0, z);
    if constexpr (LAW == HT_PHASE_CHANGE) z = __builtin_fma(c, 0.0, __builtin_fma(h, 0.0, z));
    if (valid && !(z == 0.0)) ++c_nan;

    rec[lane * HP_REC + 0] = nk;
    rec[lane * HP_REC + 1] = dj[0];
    rec[lane * HP_REC + 2] = dj[1];
    rec[lane * HP_REC + 3] = c;
    // ---- 3. the flux row, as the gradient row came in; the enthalpy ------------------------------------------------------
    if (valid) {
      stream_store<0>(reinterpret_cast<double2_t*>(flux) + gi, double2_t{j[0], j[1]});
      if constexpr (LAW == HT_PHASE_CHANGE) stream_store<1>(enthalpy + gi, h);
    }
    wave_lds_sync();

    // ---- 4. the tangent in output order: entry e of the tile belongs to point e / W, column e % W ------------------------
    auto entry = [&](int e) -> double {
      const int p = e / W, col = e - p * W;
      const double raw = rec[p * HP_REC + (col < 4 ? 0 : col - 3)];
      return col < 4 ? ((col == 0 || col == 3) ? raw : 0.0) : raw;
    };
#include "tile_entries_store.hpp"
    wave_lds_sync();   // the LDS region is rewritten by the next tile
  }

  store_block_stats(stats, 0, 0, c_nan, 0, red);
}

const void* heat_plane_stationary_kernel_fn() { return (const void*)heat_plane_kernel<HT_STATIONARY, HP_SRC_ARRAY>; }
const void* heat_plane_phase_change_kernel_fn() { return (const void*)heat_plane_kernel<HT_PHASE_CHANGE, HP_SRC_ARRAY>; }

void heat_plane_launch(int law, int grid, hipStream_t st, const HeatParams& prm, int64_t cnt, const double* grad, double t_uniform,
                       const double* tfield, const ScalarSource* src, double* enthalpy, double* flux, double* ct, BlockStats* bs) {
  const ScalarSource s = src ? *src : ScalarSource{};
#define DXM_LAUNCH_HP(L, S) \
  hipLaunchKernelGGL((heat_plane_kernel<L, S>), dim3(grid), dim3(BLOCK), 0, st, prm, cnt, grad, t_uniform, tfield, s, enthalpy, flux, ct, bs)
  if (law == HT_PHASE_CHANGE) { if (src) DXM_LAUNCH_HP(HT_PHASE_CHANGE, HP_SRC_NODAL); else DXM_LAUNCH_HP(HT_PHASE_CHANGE, HP_SRC_ARRAY); }
  else                        { if (src) DXM_LAUNCH_HP(HT_STATIONARY, HP_SRC_NODAL); else DXM_LAUNCH_HP(HT_STATIONARY, HP_SRC_ARRAY); }
#undef DXM_LAUNCH_HP
}

hipError_t scalar_gradient_launch(hipStream_t st, const ScalarSource& src, int64_t npts, double* grad, double* value) {
  if (npts <= 0) return hipSuccess;
  const dim3 grid((unsigned)((npts + SCALAR_GRAD_BLOCK - 1) / SCALAR_GRAD_BLOCK)), block(SCALAR_GRAD_BLOCK);
  hipLaunchKernelGGL(scalar_gradient_kernel, grid, block, 0, st, src, npts, grad, value);
  return hipGetLastError();
}

}  // namespace dxm
