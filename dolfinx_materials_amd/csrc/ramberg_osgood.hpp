// Host entry points of the Ramberg-Osgood kernels (ramberg_osgood.hip).  Their instantiations of small_strain_kernel live in
// a translation unit of their own: compiled into the device module of dxmat.hip, they change the generated code of the
// Voce and FeFp kernels (the scheduling of their block-status reduction; the math-library code behind the law's exp / log
// and those kernels' exp is the likely link), whereas the module without them compiles to exactly the instruction streams
// it had before the law existed.  A custom-hardening build compiles dxmat.hip alone and never serves this law.
#pragma once
#include <hip/hip_runtime.h>

#include "dxm_common.hpp"
#include "gradient.hpp"

namespace dxm {

// Launch shape ("Ramberg-Osgood"): workgroups per CU of the grid -- 64: 0.770 ms per 1e7 points, as 32,
// against 0.791 for 256 (one process; another lease 0.786 against 0.791-0.820 for 8 ... 256; profiles/r07_ramberg_osgood.md) --
// and the dynamic LDS on top of the kernel's static 30.1 KiB: none, the 98-107 VGPRs of the array-input kernels already hold
// residency at four waves per SIMD (the J2 kernels pad their LDS to get there)
constexpr int RO_BLOCKS_PER_CU = 64;
constexpr int RO_DYN_LDS = 0;

// the full-layout array-input kernel (what dxm_create sizes the grid from)
__attribute__((visibility("hidden"))) const void* ramberg_osgood_kernel();

// one launch of small_strain_kernel<LAW_RAMBERG_OSGOOD, tl, grad_kind> (tl: TL_*; grad_kind: MeshSource kind, 0 = strain array)
__attribute__((visibility("hidden"))) void ramberg_osgood_launch(int tl, int grad_kind, int grid, hipStream_t st, const LawParams& prm,
                                                                 int64_t cnt, const double* grad, double* flux, double* ct,
                                                                 BlockStats* bs, const MeshSource& src);

}  // namespace dxm
