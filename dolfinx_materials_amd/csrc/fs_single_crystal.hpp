// Host entry points of the finite-strain FCC single-crystal viscoplasticity kernels (fs_single_crystal.hip).  A translation unit of
// its own, like single_crystal.hip: compiled into an existing device module, new kernels change the code generated for the kernels
// already there.  A custom-hardening build compiles dxmat.hip alone and never serves this law.
#pragma once
#include <hip/hip_runtime.h>

#include "dxm_common.hpp"
#include "orthotropic.hpp"      // Frame9, OR_FRAME_*
#include "single_crystal.hpp"   // the twelve systems and their interaction classes (SC), SC_NSYS

namespace dxm {

// SoA state slots: every field is user-visible and in consecutive slots (pack_consecutive_slots).  Fp is a 9-vector in the order of
// the gradient, [11, 22, 33, 12, 21, 13, 31, 23, 32]: its first three slots are the diagonal (LawDesc::unit_fields)
constexpr int FX_SLOT_G = 0, FX_SLOT_P = 12, FX_SLOT_A = 24, FX_SLOT_FP = 36, FX_NSLOTS = 45;

// The record of the law's own, a kernel argument next to LawParams (of which the kernel reads rtol and maxit): formed on the host
// by the launcher from the handle's 16 parameters and the dt of the call
struct FxParams {
  double c11, c12, g2;   // the cubic stiffness: S_ii = c11 E_ii + c12 (E_jj + E_kk), S_ij = g2 E_ij (g2 = 2 G)
  double n, K, tau0, b, d, C;
  double qh[6];          // Q x the six interaction coefficients, by class
  double dt;
};

// Launch shape: law 14's grid, unmeasured for this kernel
constexpr int FX_BLOCKS_PER_CU = 64;

// Wave-private LDS map (doubles):
//   [out-tile of a tangent round: 16 x 81, padded to the whole KiBs the copy-out reads | F in / PK1 out staging 64 x 9 |
//    per point Fe_tr (9), Fp_n^-1 (9), det Fp_n | per Newton row 21 exchanged 3x3 tensors | per point of a tangent round 16 hand-over words]
constexpr int FX_PPR = 16;                                            // points per tangent round (tile_out81_copyout.hpp: F2_PPR)
constexpr int FX_OUT = ((FX_PPR * 81 + 2 * WAVE - 1) / (2 * WAVE)) * (2 * WAVE);   // 1408
constexpr int FX_STAGE = WAVE * 9;
constexpr int FX_PARK = 19;                                           // odd: the owners write conflict-free
constexpr int FX_XCH = 21 * 9;                                        // twelve slip variations and nine F variations of a row
constexpr int FX_HAND = 16;
constexpr int FX_LDS_PER_WAVE = FX_OUT + FX_STAGE + WAVE * FX_PARK + 4 * FX_XCH + FX_PPR * FX_HAND;   // 4212 doubles
constexpr int FX_SYS = 21;                                            // per slip system, shared by the waves: mu_i (9), row i of Q h (12)
// Workgroups of two waves at one wave per SIMD, as for law 14 (the register budget of the Newton rounds)
constexpr int FX_BLOCK = 128, FX_WAVES = FX_BLOCK / WAVE;
constexpr int FX_LDS_BYTES = FX_WAVES * FX_LDS_PER_WAVE * 8 + 16 * FX_SYS * 8 + 4 * FX_WAVES * 8;   // 70 144
static_assert(2 * FX_LDS_BYTES <= 160 * 1024, "two workgroups per CU");

// the kernel without a frame (what dxm_create asks the resources of)
__attribute__((visibility("hidden"))) const void* fs_single_crystal_kernel_fn();

// one launch of fs_single_crystal_kernel<frame> over cnt points: F (cnt, 9) -> PK1 (cnt, 9), dP/dF (cnt, 81); frames as in
// orthotropic_launch; s0 / s1: the two state buffers at the first point (FX_NSLOTS slots of leading dimension ld)
__attribute__((visibility("hidden"))) void fs_single_crystal_launch(int frame, int grid, hipStream_t st, const LawParams& prm, const FxParams& sp,
                                                                    int64_t cnt, const double* F, const Frame9& uniform, const double* frames,
                                                                    int64_t ldf, const double* s0, double* s1, int64_t ld, double* P, double* ct,
                                                                    BlockStats* bs);

}  // namespace dxm
