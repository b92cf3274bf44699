// Host entry points of the Hosford plasticity kernels (hosford.hip).  A translation unit of its own, like ramberg_osgood.hip and
// hyperelastic.hip: compiled into the device module of dxmat.hip, new kernels change the code generated for the existing ones
// (ramberg_osgood.hpp), whereas the module without them compiles to the instruction streams it had before the law existed.
// A custom-hardening build compiles dxmat.hip alone and never serves this law.
#pragma once
#include <hip/hip_runtime.h>

#include "dxm_common.hpp"

namespace dxm {

// SoA state slots: ElasticStrain 0..5 (written by every update, never read), EquivalentPlasticStrain 6, and the hidden field the
// update is driven by, the plastic strain 7..12: the kernel receives the TOTAL strain, so its trial elastic strain
// eps_el,n + (eps - eps_n) is eps - eps_p,n (DESIGN.md section "Hosford")
constexpr int HF_SLOT_EEL = 0, HF_SLOT_P = 6, HF_SLOT_EP = 7, HF_NSLOTS = 13;

// per-handle constants in LawParams::c (formed on the host: dxmat.hip::build_params)
constexpr int HF_A = 0, HF_AM2 = 1, HF_INVA = 2, HF_AM1 = 3;

// Launch shape: the Ramberg-Osgood grid, unmeasured for this kernel (DESIGN.md section "Hosford")
constexpr int HF_BLOCKS_PER_CU = 64;

// the full-layout kernel (what dxm_create asks the resources of)
__attribute__((visibility("hidden"))) const void* hosford_kernel_fn();

// one launch of hosford_kernel<tl>, tl = TL_FULL (36 per point) or TL_SYM (21); s0 / s1: the two state buffers at the first point
__attribute__((visibility("hidden"))) void hosford_launch(int tl, int grid, hipStream_t st, const LawParams& prm, int64_t cnt,
                                                          const double* grad, const double* s0, double* s1, int64_t ld, double* flux,
                                                          double* ct, BlockStats* bs);

}  // namespace dxm
