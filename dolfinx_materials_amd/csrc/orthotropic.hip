// Small-strain orthotropic elasticity with a material frame per handle or per Gauss point (gradient: strain (6), flux: stress (6),
// Mandel [11, 22, 33, sqrt2 12, sqrt2 13, sqrt2 23]) for gfx950.
//
// The law (the orthotropic form of the reference's StandardElasticity brick, restated from its equations): in the material frame
//   sigma_m = C eps_m,   C = [A 0; 0 diag(2 G12, 2 G13, 2 G23)],   A = S^-1,
//   S11 = 1/E1, S22 = 1/E2, S33 = 1/E3, S12 = -nu12/E1, S13 = -nu13/E1, S23 = -nu23/E2 (symmetric);
// A and the shear diagonal are formed on the host (orthotropic.hpp: OrthoStiffness).
// Frame: R is 3x3 row-major and its ROWS are the material axes in global coordinates, so
//   eps_m = R eps R^T,   sigma = R^T sigma_m R,   Ct = Q^T C Q,
// Q(R) the orthogonal 6x6 Mandel image of R: with I = (i, j), K = (k, l) the tensor indices of the Mandel components,
//   Q[I][K] = R_ik^2 (I, K < 3),  sqrt2 R_ik R_il (I < 3 <= K),  sqrt2 R_ik R_jk (K < 3 <= I),  R_ik R_jl + R_il R_jk (3 <= I, K).
// Per point: the 36 entries of Q, eps_m = Q eps, sigma_m = C eps_m, sigma = Q^T sigma_m, and column by column of the tangent
// X = C Q[:, K], Ct[I][K] = Q[:, I] . X for I <= K.  Every sum is an explicit chain of fused multiply-adds and nothing else is
// contracted: the instantiations differ only in where R comes from, so a field holding one constant frame gives the bits of the
// uniform frame.
//
// Three instantiations of one body by the frame of the handle: none (Q = I exactly: sigma = C eps, Ct = C, no rounding from a
// rotation), uniform (nine doubles, a kernel argument), field (nine SoA streams of the handle, 8 B per lane each like the state
// slots and the parameter streams).
//
// Mapping: the Hosford kernel's (hosford.hip): one thread per point, one wave per tile of 64, the tile I/O as the shared text of
// tile_rows6_*.hpp and tile_tri21_store.hpp; the frame of the point is loaded between the strain load and its LDS round trip.
#include "orthotropic.hpp"

namespace dxm {

template <int FRAME, int SYM>
__global__ void __launch_bounds__(BLOCK, 2)
orthotropic_kernel(const LawParams prm, const int64_t n, const double* __restrict__ eps, const Frame9 uniform,
                   const double* __restrict__ frames, const int64_t ldf, double* __restrict__ sig, double* __restrict__ ct,
                   BlockStats* __restrict__ stats) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) double lds_all[WAVES_PER_BLOCK * TRI21_LDS_PER_WAVE];
  __shared__ unsigned long long red[4 * WAVES_PER_BLOCK];
  static_assert(OR_LDS_BYTES == sizeof(lds_all) + sizeof(red), "orthotropic.hpp states the LDS of the kernel");

  int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  double* tri = lds_all + wid * TRI21_LDS_PER_WAVE;                       // 64 x 21 tangent entries
  double2_t* stage2 = reinterpret_cast<double2_t*>(tri + WAVE * TRI21);   // strain in / stress out staging

  const int64_t ntiles = (n + WAVE - 1) / WAVE;
  const int64_t tile_stride = (int64_t)gridDim.x * WAVES_PER_BLOCK;
  unsigned long long c_nan = 0;

  const OrthoStiffness C = ortho_load(prm);
  // the normal block is symmetric by construction (the host mirrors its upper triangle)
  const double A[3][3] = {{C.c[0], C.c[1], C.c[2]}, {C.c[1], C.c[4], C.c[5]}, {C.c[2], C.c[5], C.c[8]}};
  const double SQ2 = 1.4142135623730950488;

  for (int64_t tile = (int64_t)blockIdx.x * WAVES_PER_BLOCK + wid; tile < ntiles; tile += tile_stride) {
    const int64_t base = tile * WAVE;
    const int npts = (n - base) < WAVE ? (int)(n - base) : WAVE;
    // per-lane invariants are re-derived per tile from an opaque copy (small_strain.hpp: hoisted, they cost registers over the whole body)
    asm volatile("" : "+v"(lane));
    lane &= WAVE - 1;
    const bool valid = lane < npts;
    const int64_t gi = base + lane;

    // ---- 1. coalesced strain load (3 x 1 KiB per wave) into LDS; the frame of the point --------------------------
    double e[6];
#include "tile_rows6_load.hpp"
    double R[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    if constexpr (FRAME == OR_FRAME_FIELD) {
      if (valid) {
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k / 3][k % 3] = stream_load<3>(frames + (int64_t)k * ldf + gi);
      }
    } else if constexpr (FRAME == OR_FRAME_UNIFORM) {
      // an opaque copy per tile: the 36 entries of Q and the 21 of the tangent are not carried over the tile loop in registers
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        double r = uniform.r[k];
        asm volatile("" : "+v"(r));
        R[k / 3][k % 3] = r;
      }
    }
    wave_lds_sync();
#include "tile_rows6_take.hpp"
    wave_lds_sync();   // the staging region is reused for the stress below

    int ro = lane * TRI21;   // opaque: every access is base + small immediate
    asm volatile("" : "+v"(ro));
    double* rec = tri + ro;
    double cchk = 0.0;   // sum of everything the point writes
    double sg[6];

    if constexpr (FRAME == OR_FRAME_NONE) {
      // ---- 2. Q = I: sigma = C eps, Ct = C ------------------------------------------------------------------------
#pragma unroll
      for (int a = 0; a < 3; ++a) sg[a] = __builtin_fma(A[a][2], e[2], __builtin_fma(A[a][1], e[1], A[a][0] * e[0]));
#pragma unroll
      for (int s = 0; s < 3; ++s) sg[3 + s] = C.g2[s] * e[3 + s];
#pragma unroll
      for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int k = i; k < 6; ++k) rec[TRI21_AT(i, k)] = (k < 3) ? A[i][k] : ((i == k) ? C.g2[i - 3] : 0.0);
    } else {
      // ---- 2. the Mandel image of R -------------------------------------------------------------------------------
      double Q[6][6];
#pragma unroll
      for (int I = 0; I < 6; ++I)
#pragma unroll
        for (int K = 0; K < 6; ++K) {
          const int i = SI[I], j = SJ[I], k = SI[K], l = SJ[K];
          if (I < 3 && K < 3) Q[I][K] = R[i][k] * R[i][k];
          else if (I < 3) Q[I][K] = SQ2 * (R[i][k] * R[i][l]);
          else if (K < 3) Q[I][K] = SQ2 * (R[i][k] * R[j][k]);
          else Q[I][K] = __builtin_fma(R[i][k], R[j][l], R[i][l] * R[j][k]);
        }
      // ---- 3. eps_m = Q eps, sigma_m = C eps_m, sigma = Q^T sigma_m ---------------------------------------------
      double em[6], sm[6];
#pragma unroll
      for (int I = 0; I < 6; ++I) {
        double t = Q[I][0] * e[0];
#pragma unroll
        for (int K = 1; K < 6; ++K) t = __builtin_fma(Q[I][K], e[K], t);
        em[I] = t;
      }
#pragma unroll
      for (int a = 0; a < 3; ++a) sm[a] = __builtin_fma(A[a][2], em[2], __builtin_fma(A[a][1], em[1], A[a][0] * em[0]));
#pragma unroll
      for (int s = 0; s < 3; ++s) sm[3 + s] = C.g2[s] * em[3 + s];
#pragma unroll
      for (int K = 0; K < 6; ++K) {
        double t = Q[0][K] * sm[0];
#pragma unroll
        for (int r = 1; r < 6; ++r) t = __builtin_fma(Q[r][K], sm[r], t);
        sg[K] = t;
      }
      // ---- 4. Ct = Q^T C Q, column by column, the upper triangle into the point's LDS record ----------------------
#pragma unroll
      for (int K = 0; K < 6; ++K) {
        double X[6];
#pragma unroll
        for (int a = 0; a < 3; ++a) X[a] = __builtin_fma(A[a][2], Q[2][K], __builtin_fma(A[a][1], Q[1][K], A[a][0] * Q[0][K]));
#pragma unroll
        for (int s = 0; s < 3; ++s) X[3 + s] = C.g2[s] * Q[3 + s][K];
#pragma unroll
        for (int I = 0; I <= K; ++I) {
          double t = Q[0][I] * X[0];
#pragma unroll
          for (int r = 1; r < 6; ++r) t = __builtin_fma(Q[r][I], X[r], t);
          rec[TRI21_AT(I, K)] = t;
          cchk += t;
        }
      }
    }
    stage2[lane * 3 + 0] = double2_t{sg[0], sg[1]};
    stage2[lane * 3 + 1] = double2_t{sg[2], sg[3]};
    stage2[lane * 3 + 2] = double2_t{sg[4], sg[5]};
#pragma unroll
    for (int c = 0; c < 6; ++c) cchk += sg[c];
    // stress and tangent (quadrature_map.py:322-324 asserts on both)
    if (valid && !(fabs(cchk) <= 1.79769313486231570e308)) ++c_nan;
    wave_lds_sync();

    // ---- 5. coalesced stress store; 6. tangent, in output order from the staged records ------------------------
#include "tile_rows6_store.hpp"
#include "tile_tri21_store.hpp"
    wave_lds_sync();   // the LDS region is rewritten by the next tile
  }

  store_block_stats(stats, 0, 0, c_nan, 0, red);
}

// (n, 9) row-major -> nine streams of leading dimension ldf (dxm_set_frame_field, dxm_set_frame_field_device: once at set time)
__global__ void __launch_bounds__(256) orthotropic_frames_kernel(const double* __restrict__ aos, int64_t n, double* __restrict__ frames, int64_t ldf) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * 9) return;
  const int64_t i = t / 9;
  const int k = (int)(t - i * 9);
  frames[(int64_t)k * ldf + i] = aos[t];
}

const void* orthotropic_kernel_fn() { return (const void*)orthotropic_kernel<OR_FRAME_NONE, 0>; }

void orthotropic_launch(int frame, int tl, int grid, hipStream_t st, const LawParams& prm, int64_t cnt, const double* grad,
                        const Frame9& uniform, const double* frames, int64_t ldf, double* flux, double* ct, BlockStats* bs) {
#define DXM_LAUNCH_OR(F, S) \
  hipLaunchKernelGGL((orthotropic_kernel<F, S>), dim3(grid), dim3(BLOCK), 0, st, prm, cnt, grad, uniform, frames, ldf, flux, ct, bs)
#define DXM_LAUNCH_OR_S(F) do { if (tl == 1) DXM_LAUNCH_OR(F, 1); else DXM_LAUNCH_OR(F, 0); } while (0)
  if (frame == OR_FRAME_FIELD) DXM_LAUNCH_OR_S(OR_FRAME_FIELD);
  else if (frame == OR_FRAME_UNIFORM) DXM_LAUNCH_OR_S(OR_FRAME_UNIFORM);
  else DXM_LAUNCH_OR_S(OR_FRAME_NONE);
#undef DXM_LAUNCH_OR_S
#undef DXM_LAUNCH_OR
}

void orthotropic_frames_to_streams(int64_t n, const double* aos, double* frames, int64_t ldf, hipStream_t st) {
  if (n <= 0) return;
  const int64_t blocks = (n * 9 + 255) / 256;
  hipLaunchKernelGGL(orthotropic_frames_kernel, dim3((unsigned)blocks), dim3(256), 0, st, aos, n, frames, ldf);
}

}  // namespace dxm
