// Host entry points of the plane-strain Hosford kernel (hosford_plane.hip): law 10 (hosford.hip) in the four components
// [xx, yy, zz, sqrt(2) xy] of a plane-strain state.  A translation unit of its own, like the other laws added after the first five
// (ramberg_osgood.hpp says why); this header declares host functions and constants only, so dxmat.hip's device code does not see the
// law.  A custom-hardening build compiles dxmat.hip alone and never serves this law.
// The parameter record is law 10's: LawParams as dxmat.hip::build_hosford fills it (the HF_* slots of hosford.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include "dxm_common.hpp"

namespace dxm {

constexpr int HFP_DIM = 4;   // strain, stress, elastic and plastic strain
constexpr int HFP_CT = 16;   // the 4x4 tangent, row-major: exactly one 128 B line per point

// SoA state slots, law 10's fields at their plane-strain width: ElasticStrain 0..3 (written by every update, never read),
// EquivalentPlasticStrain 4, and the hidden field the update is driven by, the plastic strain 5..8 (hosford.hpp)
constexpr int HFP_SLOT_EEL = 0, HFP_SLOT_P = 4, HFP_SLOT_EP = 5, HFP_NSLOTS = 9;

// per wave: the 64 x 4 strain-in / stress-out staging, then 64 records of the 10 upper-triangle entries of the symmetric 4x4 tangent,
// row by row (hfp_tri10)
constexpr int HFP_TRI = 10;
constexpr int hfp_tri10(int i, int k) { return i <= k ? i * 4 - i * (i - 1) / 2 + (k - i) : k * 4 - k * (k - 1) / 2 + (i - k); }
constexpr int HFP_LDS_PER_WAVE = WAVE * HFP_DIM + WAVE * HFP_TRI;                                 // 896 doubles
constexpr int HFP_LDS_BYTES = WAVES_PER_BLOCK * HFP_LDS_PER_WAVE * 8 + 4 * WAVES_PER_BLOCK * 8;   // 28 800 B per workgroup
static_assert(HFP_LDS_PER_WAVE == 64 * (4 + 10) && HFP_LDS_BYTES == 28800 && hfp_tri10(3, 3) == HFP_TRI - 1 && hfp_tri10(2, 1) == 5,
              "the LDS that DESIGN.md states for the plane-strain Hosford kernel");

// Launch shape: law 10's grid (hosford.hpp).  One sweep at 1e7 points, half of them yielding (profiles/r27_hosford_plane.md: 32 / 64 /
// 128 / 256, one timing each): 1.6828 / 1.6715 / 1.6845 / 1.6918 ms, all within 1.2 %; 64 stays.  Other sizes: not measured.
constexpr int HFP_BLOCKS_PER_CU = 64;

__attribute__((visibility("hidden"))) const void* hosford_plane_kernel_fn();

// one launch of hosford_plane_kernel over cnt points; s0 / s1: slot 0 of the two state buffers at the first point of the launch
__attribute__((visibility("hidden"))) void hosford_plane_launch(int grid, hipStream_t st, const LawParams& prm, int64_t cnt,
                                                                const double* grad, const double* s0, double* s1, int64_t ld, double* flux,
                                                                double* ct, BlockStats* bs);

}  // namespace dxm
