// Host entry points of the logarithmic-strain J2 plasticity kernel (log_strain.hip).  A translation unit of its own, like
// hyperelastic.hip and hosford.hip (hyperelastic.hpp says why: a new kernel inside an existing device module changes the code
// generated for the kernels already there); this header declares host functions only.
// A custom-hardening build compiles dxmat.hip alone and never serves this law.
#pragma once
#include <hip/hip_runtime.h>

#include "dxm_common.hpp"

namespace dxm {

// SoA state slots, those of the Hosford law for the same names: ElasticStrain 0..5 (written by every update, never read),
// EquivalentPlasticStrain 6, and the hidden field the update is driven by, the logarithmic plastic strain 7..12: the kernel
// receives the TOTAL F, so its trial elastic strain eel_n + (E - E_n) is E - Ep_n (DESIGN.md section "Logarithmic-strain J2")
constexpr int LS_SLOT_EEL = 0, LS_SLOT_P = 6, LS_SLOT_EP = 7, LS_NSLOTS = 13;

// Launch shape: one workgroup per 256 points up to 256 per CU, as for the Ogden kernel whose I/O skeleton this kernel shares;
// unmeasured for this law
constexpr int LS_BLOCKS_PER_CU = 256;

__attribute__((visibility("hidden"))) const void* log_strain_kernel_fn();

// one launch over cnt points: F (cnt, 9) -> PK1 (cnt, 9), dP/dF (cnt, 81); s0 / s1: the two state buffers at the first point
// (LS_NSLOTS slots of leading dimension ld)
__attribute__((visibility("hidden"))) void log_strain_launch(int grid, hipStream_t st, const LawParams& prm, int64_t cnt, const double* F,
                                                             const double* s0, double* s1, int64_t ld, double* P, double* ct,
                                                             BlockStats* bs);

}  // namespace dxm
