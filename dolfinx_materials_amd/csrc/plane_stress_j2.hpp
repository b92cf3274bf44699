// Host entry points of the plane-stress J2 kernels with isotropic hardening (plane_stress_j2.hip): laws 1 and 2 under
// sig_zz = sig_xz = sig_yz = 0, in the three components [xx, yy, sqrt(2) xy] of laws 23 and 24.  A translation unit of its own, like
// the other laws added after the first five: compiled into the device module of dxmat.hip, new kernels change the code generated
// for the existing ones (ramberg_osgood.hpp).  A custom-hardening build compiles dxmat.hip alone and never serves these laws.
#pragma once
#include <hip/hip_runtime.h>

#include "dxm_common.hpp"

namespace dxm {

// template argument of plane_stress_j2_kernel: the 6-wide law whose hardening it takes (small_strain.hpp: LAW_J2_LINEAR,
// LAW_J2_VOCE, whose hardening_R / hardening_dR the kernel calls)
constexpr int PSJ_LINEAR = 1, PSJ_VOCE = 2;

// What the kernels read: the record of the 6-wide law (build_linear_hardening / build_voce_hardening: sig0, h1, h2, tol, rtol,
// maxit) and the plane-stress constants, formed on the host once per launch from E and nu (dxmat.hip::launch_plane_stress_j2): every
// entry is a few individually rounded operations on parameters, written out there, so that a restatement forms the same bits.
// In the basis a = (s0 + s1) / sqrt 2, b = (s0 - s1) / sqrt 2, c = s2 the stiffness is diag(CA, CB, CB) and the deviatoric
// projector diag(1/3, 1, 1): k_i = C_i P_i = (CA / 3, CB, CB).
struct PsJ2Params {
  LawParams law;
  double c11, c12, c33;   // E / (1 - nu^2) [[1, nu, 0], [nu, 1, 0], [0, 0, 1 - nu]]: the tangent of an elastic point
  double CA, CB;          // E / (1 - nu), E / (1 + nu)
  double ka;              // CA / 3
  double kmax, kmin;      // of (ka, CB)
};

// Launch shape: started from the plane-stress precedent (plane_stress.hpp), 32 workgroups per CU.  One sweep at 1e7 points
// (profiles/r22_plane_stress_j2.md: 32 / 64 / 128 / 256, one timing each): 128 and 256 are 4.5 % faster on a wholly elastic batch of
// the linear law and 4-9 % slower on every batch with yielded points of both laws, 64 is within 3 % of 32.  32 stays
constexpr int PSJ_BLOCKS_PER_CU = 32;

// per wave: the 64 x 3 strain-in / stress-out staging, then 64 records of the six distinct tangent entries
// (D00, D01, D02, D11, D12, D22)
constexpr int PSJ_REC = 6;
constexpr int PSJ_LDS_PER_WAVE = WAVE * 3 + WAVE * PSJ_REC;                                       // 576 doubles
constexpr int PSJ_LDS_BYTES = WAVES_PER_BLOCK * PSJ_LDS_PER_WAVE * 8 + 4 * WAVES_PER_BLOCK * 8;   // 18 560 B per workgroup
static_assert(PSJ_LDS_PER_WAVE == 64 * (3 + 6) && PSJ_LDS_BYTES == 18560, "the LDS that DESIGN.md states for the plane-stress J2 kernels");
constexpr int PSJ_NSLOTS = 4;   // SoA state: 0 = p, 1..3 = eps_p [xx, yy, sqrt(2) xy]

// the kernel of a law (what dxm_create asks the resources of)
__attribute__((visibility("hidden"))) const void* plane_stress_j2_linear_kernel_fn();
__attribute__((visibility("hidden"))) const void* plane_stress_j2_voce_kernel_fn();

// one launch of plane_stress_j2_kernel<hard>; s0 / s1: slot 0 of the initial / final state at the first point of the launch
__attribute__((visibility("hidden"))) void plane_stress_j2_launch(int hard, int grid, hipStream_t st, const PsJ2Params& prm, int64_t cnt,
                                                                  const double* grad, const double* s0, double* s1, int64_t ld,
                                                                  double* flux, double* ct, BlockStats* bs);

}  // namespace dxm
