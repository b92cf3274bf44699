// Host entry points of the plane-strain kernels (plane_strain.hip): isotropic elasticity and J2 plasticity with linear or Voce
// hardening in the four components [xx, yy, zz, sqrt(2) xy] of a plane-strain state.  A translation unit of its own, like the
// other laws added after the first five: compiled into the device module of dxmat.hip, new kernels change the code generated for
// the existing ones (ramberg_osgood.hpp).  A custom-hardening build compiles dxmat.hip alone and never serves these laws.
#pragma once
#include <hip/hip_runtime.h>

#include "dxm_common.hpp"

namespace dxm {

// template argument of plane_strain_kernel: the 6-wide law it is the plane-strain form of (small_strain.hpp: LAW_ELASTIC,
// LAW_J2_LINEAR, LAW_J2_VOCE, whose hardening_R / hardening_dR the kernel calls)
constexpr int PE_ELASTIC = 0, PE_J2_LINEAR = 1, PE_J2_VOCE = 2;

constexpr int PE_DIM = 4;      // strain, stress, plastic strain
constexpr int PE_CT = 16;      // the 4x4 tangent, row-major: exactly one 128 B line per point
constexpr int PE_NSLOTS = 5;   // SoA state of the J2 laws: 0 = p, 1..4 = eps_p

// Launch shape.  The precedent of the 6-wide kernels (the comment above the rows in dxmat.hip) is 32 workgroups per CU for the laws
// whose tiles all cost the same and one workgroup per 256 points, up to 256 per CU, for the law with a local Newton.  One sweep at
// 1e7 points (profiles/r21_plane_strain.md: 32 / 64 / 128 / 256, one timing each) has the elastic kernel 7 % and the
// linear-hardening kernel 2.7 % faster at 128 than at 32, and 256 within 0.7 % of 128; Voce is within 1.5 % at every size.  128 is
// taken for the first two on that run; a second run on another lease gives the same order.  Other sizes: not measured.
constexpr int PE_BLOCKS_PER_CU = 128;
constexpr int PE_BLOCKS_PER_CU_VOCE = 256;

// per wave: the 64 x 4 strain-in / stress-out staging, then 64 records (c1, c2, c3, n0..n3) of Ct = c1 1x1 + c2 I + c3 n x n
// (the elastic law stages no record and leaves that region unused: one LDS size for the three instantiations)
constexpr int PE_REC = 7;
constexpr int PE_LDS_PER_WAVE = WAVE * PE_DIM + WAVE * PE_REC;                                  // 704 doubles
constexpr int PE_LDS_BYTES = WAVES_PER_BLOCK * PE_LDS_PER_WAVE * 8 + 4 * WAVES_PER_BLOCK * 8;   // 22 656 B per workgroup
static_assert(PE_LDS_PER_WAVE == 64 * (4 + 7) && PE_LDS_BYTES == 22656, "the LDS that DESIGN.md states for the plane-strain kernels");

// the kernel of a law (what dxm_create asks the resources of)
__attribute__((visibility("hidden"))) const void* plane_strain_elastic_kernel_fn();
__attribute__((visibility("hidden"))) const void* plane_strain_j2_linear_kernel_fn();
__attribute__((visibility("hidden"))) const void* plane_strain_j2_voce_kernel_fn();

// one launch of plane_strain_kernel<law>; s0 / s1: slot 0 of the initial / final state at the first point of the launch (not read
// by the elastic law)
__attribute__((visibility("hidden"))) void plane_strain_launch(int law, int grid, hipStream_t st, const LawParams& prm, int64_t cnt,
                                                               const double* grad, const double* s0, double* s1, int64_t ld, double* flux,
                                                               double* ct, BlockStats* bs);

}  // namespace dxm
