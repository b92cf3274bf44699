// Host entry points of the orthotropic elasticity kernels (orthotropic.hip).  A translation unit of its own, like ramberg_osgood.hip,
// hyperelastic.hip and hosford.hip: compiled into the device module of dxmat.hip, new kernels change the code generated for the
// existing ones (ramberg_osgood.hpp).  A custom-hardening build compiles dxmat.hip alone and never serves this law.
#pragma once
#include <hip/hip_runtime.h>

#include "dxm_common.hpp"

namespace dxm {

// The stiffness in the material frame, formed on the host once per dxm_set_params (dxmat.hip::build_orthotropic): the 3x3 normal
// block (the inverse of the compliance block, row-major: 9 numbers) and the Mandel shear diagonal 2 G12, 2 G13, 2 G23 (3 numbers).
// LawParams has no field of that shape and its layout is part of every other kernel's argument list, so the twelve numbers sit in
// its twelve free doubles, addressed through these names only
struct OrthoStiffness {
  double c[9];    // normal block, row-major
  double g2[3];   // 2 G12, 2 G13, 2 G23: the Mandel order [12, 13, 23]
};
inline void ortho_store(LawParams& q, const OrthoStiffness& s) {
  q.lambda = s.c[0]; q.mu = s.c[1]; q.kappa = s.c[2]; q.sig0 = s.c[3]; q.h1 = s.c[4]; q.h2 = s.c[5];
  q.c[0] = s.c[6]; q.c[1] = s.c[7]; q.c[2] = s.c[8]; q.c[3] = s.g2[0]; q.c[4] = s.g2[1]; q.c[5] = s.g2[2];
}
__host__ __device__ inline OrthoStiffness ortho_load(const LawParams& q) {
  return OrthoStiffness{{q.lambda, q.mu, q.kappa, q.sig0, q.h1, q.h2, q.c[0], q.c[1], q.c[2]}, {q.c[3], q.c[4], q.c[5]}};
}

// the material frame of a launch: none (identity), one per handle (a kernel argument), one per Gauss point (nine SoA streams)
constexpr int OR_FRAME_NONE = 0, OR_FRAME_UNIFORM = 1, OR_FRAME_FIELD = 2;
struct Frame9 { double r[9]; };   // row-major 3x3: the rows are the material axes in global coordinates

// Launch shape: the Hosford / Ramberg-Osgood grid, unmeasured for this kernel (DESIGN.md section "Orthotropic elasticity")
constexpr int OR_BLOCKS_PER_CU = 64;

// static LDS of one workgroup: per wave the 64 x 21 staged tangent entries and the strain / stress staging, plus the block-stats words
constexpr int OR_LDS_BYTES = WAVES_PER_BLOCK * TRI21_LDS_PER_WAVE * 8 + 4 * WAVES_PER_BLOCK * 8;

// the full-layout kernel without a frame (what dxm_create asks the resources of)
__attribute__((visibility("hidden"))) const void* orthotropic_kernel_fn();

// one launch of orthotropic_kernel<frame, tl>, tl = TL_FULL (36 per point) or TL_SYM (21).  frames: stream k of the field is
// frames[k * ldf + point], at the first point of the launch (OR_FRAME_FIELD only)
__attribute__((visibility("hidden"))) void orthotropic_launch(int frame, int tl, int grid, hipStream_t st, const LawParams& prm, int64_t cnt,
                                                              const double* grad, const Frame9& uniform, const double* frames, int64_t ldf,
                                                              double* flux, double* ct, BlockStats* bs);

// (n, 9) row-major frames in device memory -> the nine SoA streams of a handle, asynchronous on st
__attribute__((visibility("hidden"))) void orthotropic_frames_to_streams(int64_t n, const double* aos, double* frames, int64_t ldf, hipStream_t st);

}  // namespace dxm
