// Host entry points of the two heat-transfer kernels (heat_transfer.hip).  A translation unit of its own, like the other laws
// added after the first five: compiled into the device module of dxmat.hip, new kernels change the code generated for the
// existing ones (ramberg_osgood.hpp).  A custom-hardening build compiles dxmat.hip alone and never serves these laws.
#pragma once
#include <hip/hip_runtime.h>

#include "dxm_common.hpp"

namespace dxm {

constexpr int HT_STATIONARY = 0, HT_PHASE_CHANGE = 1;

// What the kernels read, formed on the host once per launch from the handle's parameters (dxmat.hip::launch_heat_*): every entry
// is either a parameter or ONE individually rounded operation on parameters, named below, so that a restatement forms the same bits.
//   stationary:   [HT_A] = A, [HT_B] = B
//   phase change: the names below
struct HeatParams { double p[13]; };
constexpr int HT_A = 0, HT_B = 1;
constexpr int HT_TS = 0,      // Tm - Tsmooth / 2
              HT_TL = 1,      // Tm + Tsmooth / 2
              HT_KS = 2, HT_KL = 3, HT_CS = 4, HT_CL = 5,
              HT_DK = 6,      // kl - ks
              HT_TSM = 7,     // Tsmooth
              HT_CTR = 8,     // (cs + cl) / 2 + dhsl / Tsmooth
              HT_NSLOPE = 9,  // -(kl - ks) / Tsmooth: the file's dk/dT of the transition, the factor of g in dj/dT
              HT_DHSL = 10,
              HT_CSTS = 11,   // cs * Ts
              HT_HL3 = 12;    // ((cs + cl) * Tsmooth) / 2

// doubles per point of the tangent: -k I (9) | dj/dT (3) [| dh/dT (1)]
constexpr int HT_WIDTH[2] = {12, 13};

// Launch shape: DESIGN.md section 3's streaming grid (the elastic kernel's), unmeasured for these kernels
constexpr int HT_BLOCKS_PER_CU = 32;

// per wave: the 64 x 3 gradient-in / flux-out staging, then 64 records (-k, dj/dT[0..2], c) the tangent is written from
constexpr int HT_REC = 5;
constexpr int HT_LDS_PER_WAVE = WAVE * 3 + WAVE * HT_REC;
constexpr int HT_LDS_BYTES = WAVES_PER_BLOCK * HT_LDS_PER_WAVE * 8 + 4 * WAVES_PER_BLOCK * 8;

// the uniform-temperature kernel of a law (what dxm_create asks the resources of)
__attribute__((visibility("hidden"))) const void* heat_stationary_kernel_fn();
__attribute__((visibility("hidden"))) const void* heat_phase_change_kernel_fn();

// one launch of heat_transfer_kernel<law, field>: tfield null = the uniform temperature t_uniform, else one value per point at
// the first point of the launch; enthalpy: slot 0 of the final state at that point (phase change only)
__attribute__((visibility("hidden"))) void heat_transfer_launch(int law, int grid, hipStream_t st, const HeatParams& prm, int64_t cnt,
                                                                const double* grad, double t_uniform, const double* tfield,
                                                                double* enthalpy, double* flux, double* ct, BlockStats* bs);

}  // namespace dxm
