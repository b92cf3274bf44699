// The two heat-transfer laws of the reference's MFront demos for gfx950 (gradient: temperature gradient g (3), flux: heat flux
// j (3), external state variable: the temperature T at the end of the step).
//
//   stationary (StationaryHeatTransfer.mfront):     k = 1 / (A + B T),  j = -k g,  dj/dg = -k I,  dj/dT = B k^2 g
//   phase change (HeatTransferPhaseChange.mfront:41-56), Ts = Tm - Tsmooth/2 and Tl = Tm + Tsmooth/2 formed on the host:
//     T < Ts: k = ks, c = cs, h = cs T, k' = 0
//     T > Tl: k = kl, c = cl, h = cl (T - Tl) + dhsl + cs Ts + (cs + cl) Tsmooth / 2, k' = 0
//     else:   k = ks + (kl - ks)(T - Ts)/Tsmooth, c = (cs + cl)/2 + dhsl/Tsmooth, h = cs Ts + c (T - Ts), k' = -(kl - ks)/Tsmooth
//     j = -k g,  dj/dg = -k I,  dj/dT = k' g,  dh/dT = c;  the enthalpy h is the law's one state field, written and never read
// Both are closed forms: every operation is individually rounded (no contraction), in the order written in the body, so that a
// restatement reproduces the bits and the uniform-T and T-field instantiations agree on a constant field.
//
// Mapping: one thread per point, one wave per tile of 64 points, 256-thread workgroups, grid-stride over the
// tiles; the lanes of a wave exchange through a wave-private LDS region ordered by wave_lds_sync(), no workgroup barrier inside the
// tile loop; one BlockStats record per workgroup.
// Memory: a tile's gradient and flux rows of 3 move through LDS by tile_rows3_load.hpp / tile_rows3_store.hpp; T and the enthalpy
// are 8 B per lane.  The tangent is never held per thread: each point stages (-k, dj/dT[0..2], c) in LDS and tile_entries_store.hpp
// writes the 12 / 13 numbers per point in output order.  A tile's tangent is 6144 / 6656 B and starts on a multiple of 512 B, so
// every 128 B line is written whole; the six structural zeros of -k I are written (the layout is the reference's jacobian_flatten).
// A ragged last tile is bounded by lane in those three texts.
#include "heat_transfer.hpp"

namespace dxm {

template <int LAW, int TFIELD>
__global__ void __launch_bounds__(BLOCK)
heat_transfer_kernel(const HeatParams prm, const int64_t n, const double* __restrict__ grad, const double t_uniform,
                     const double* __restrict__ tfield, double* __restrict__ enthalpy, double* __restrict__ flux,
                     double* __restrict__ ct, BlockStats* __restrict__ stats) {
#pragma clang fp contract(off)
  constexpr int W = HT_WIDTH[LAW];
  __shared__ __attribute__((aligned(16))) double lds_all[WAVES_PER_BLOCK * HT_LDS_PER_WAVE];
  __shared__ unsigned long long red[4 * WAVES_PER_BLOCK];
  static_assert(HT_LDS_BYTES == sizeof(lds_all) + sizeof(red), "heat_transfer.hpp states the LDS of the kernel");
  static_assert((WAVE * 3) % 2 == 0 && (WAVE * W) % 2 == 0 && (HT_LDS_PER_WAVE * 8) % 16 == 0, "16 B accesses of whole tiles");

  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  double* stage = lds_all + wid * HT_LDS_PER_WAVE;            // 64 x 3: gradient in, flux out
  double2_t* stage2 = reinterpret_cast<double2_t*>(stage);
  double* rec = stage + WAVE * 3;                             // 64 x (-k, dj/dT[0..2], c)

  const int64_t ntiles = (n + WAVE - 1) / WAVE;
  const int64_t tile_stride = (int64_t)gridDim.x * WAVES_PER_BLOCK;
  unsigned long long c_nan = 0;

  for (int64_t tile = (int64_t)blockIdx.x * WAVES_PER_BLOCK + wid; tile < ntiles; tile += tile_stride) {
    const int64_t base = tile * WAVE;
    const int npts = (n - base) < WAVE ? (int)(n - base) : WAVE;
    const bool valid = lane < npts;
    const int64_t gi = base + lane;

    // ---- 1. the tile's gradient rows into LDS; the temperature ------------------------------------------------------------
#include "tile_rows3_load.hpp"
    double T = t_uniform;
    if constexpr (TFIELD) {
      if (valid) T = stream_load<3>(tfield + gi);
    }
    wave_lds_sync();
    const double g[3] = {stage[lane * 3 + 0], stage[lane * 3 + 1], stage[lane * 3 + 2]};
    wave_lds_sync();   // the staging region is reused for the flux below

    // ---- 2. the law ------------------------------------------------------------------------------------------------------
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
    const double j[3] = {nk * g[0], nk * g[1], nk * g[2]};
    const double dj[3] = {slope * g[0], slope * g[1], slope * g[2]};
    // a non-finite flux, state or tangent entry: v * 0 is NaN exactly for those
    double z = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) z = __builtin_fma(j[a], 0.0, __builtin_fma(dj[a], 0.0, z));
    z = __builtin_fma(nk, 0.0, z);
    if constexpr (LAW == HT_PHASE_CHANGE) z = __builtin_fma(c, 0.0, __builtin_fma(h, 0.0, z));
    if (valid && !(z == 0.0)) ++c_nan;

    stage[lane * 3 + 0] = j[0];
    stage[lane * 3 + 1] = j[1];
    stage[lane * 3 + 2] = j[2];
    rec[lane * HT_REC + 0] = nk;
    rec[lane * HT_REC + 1] = dj[0];
    rec[lane * HT_REC + 2] = dj[1];
    rec[lane * HT_REC + 3] = dj[2];
    rec[lane * HT_REC + 4] = c;
    if constexpr (LAW == HT_PHASE_CHANGE) {
      if (valid) stream_store<1>(enthalpy + gi, h);
    }
    wave_lds_sync();

    // ---- 3. the flux rows, as they came in -------------------------------------------------------------------------------
#include "tile_rows3_store.hpp"
    // ---- 4. the tangent in output order: entry e of the tile belongs to point e / W, column e % W ------------------------
    auto entry = [&](int e) -> double {
      const int p = e / W, col = e - p * W;
      const double raw = rec[p * HT_REC + (col < 9 ? 0 : col - 8)];
      return col < 9 ? ((col & 3) == 0 ? raw : 0.0) : raw;
    };
#include "tile_entries_store.hpp"
    wave_lds_sync();   // the LDS region is rewritten by the next tile
  }

  store_block_stats(stats, 0, 0, c_nan, 0, red);
}

const void* heat_stationary_kernel_fn() { return (const void*)heat_transfer_kernel<HT_STATIONARY, 0>; }
const void* heat_phase_change_kernel_fn() { return (const void*)heat_transfer_kernel<HT_PHASE_CHANGE, 0>; }

void heat_transfer_launch(int law, int grid, hipStream_t st, const HeatParams& prm, int64_t cnt, const double* grad, double t_uniform,
                          const double* tfield, double* enthalpy, double* flux, double* ct, BlockStats* bs) {
#define DXM_LAUNCH_HT(L, F) \
  hipLaunchKernelGGL((heat_transfer_kernel<L, F>), dim3(grid), dim3(BLOCK), 0, st, prm, cnt, grad, t_uniform, tfield, enthalpy, flux, ct, bs)
  if (law == HT_PHASE_CHANGE) { if (tfield) DXM_LAUNCH_HT(HT_PHASE_CHANGE, 1); else DXM_LAUNCH_HT(HT_PHASE_CHANGE, 0); }
  else                        { if (tfield) DXM_LAUNCH_HT(HT_STATIONARY, 1); else DXM_LAUNCH_HT(HT_STATIONARY, 0); }
#undef DXM_LAUNCH_HT
}

}  // namespace dxm
