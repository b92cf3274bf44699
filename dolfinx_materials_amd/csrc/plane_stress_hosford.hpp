// Host entry points of the plane-stress Hosford return-mapping kernel (plane_stress_hosford.hip).  A translation unit of its own,
// like the other laws added after the first five: compiled into the device module of dxmat.hip, new kernels change the code
// generated for the existing ones (ramberg_osgood.hpp).  A custom-hardening build compiles dxmat.hip alone and never serves it.
#pragma once
#include <hip/hip_runtime.h>

#include "dxm_common.hpp"

namespace dxm {

// What the kernel reads, formed on the host once per launch from the handle's parameters (dxmat.hip::launch_ps_hosford): every
// entry is a parameter or a few individually rounded operations on parameters, written out there, so that a restatement forms the
// same bits.  The stiffness is that of cvxpy_materials.py:16-18, C11 = E / (1 - nu^2), C12 = C11 nu, C33 = C11 (1 - nu).
struct PshParams {
  double p[16];
  int32_t maxit;   // cap of the root's iteration (dxm_set_newton)
  int32_t pad;
};
constexpr int PSH_C11 = 0, PSH_C12 = 1, PSH_C33 = 2,
              PSH_E = 3, PSH_NU = 4,
              PSH_SQA = 5,    // sqrt(E / (1 - nu)): the scale of A = (sI + sII) / sqrt 2
              PSH_SQB = 6,    // sqrt(E / (1 + nu)): the scale of B = (sI - sII) / sqrt 2
              PSH_SIG0 = 7,
              PSH_A = 8,      // the exponent a
              PSH_AM1 = 9,    // a - 1
              PSH_AM2 = 10,   // a - 2
              PSH_INVA = 11,  // 1 / a
              PSH_TOL = 12,   // max(rtol, 2^-49): the bound on the last step of the angle, in radians
              PSH_CB = 13,    // E / (1 + nu)
              PSH_KLO = 14,   // (1/2)^(1/a) (1 - 4 eps) and
              PSH_KHI = 15;   // (3/2)^(1/a) (1 + 4 eps): phi / max(|t_I|, |t_II|, |t_I - t_II|) lies between them

// The exponent's range (dxm_create refuses what lies outside): below 2 the Hessian of phi is unbounded on the axes; 100 is the
// largest exponent at which the accuracy was measured
constexpr double PSH_A_MIN = 2.0, PSH_A_MAX = 100.0;

// Launch shape: DESIGN.md section 3's streaming grid, at the value of the other plane-stress kernels (plane_stress.hpp).  The root's
// iteration makes the tiles cost unequally, as the quadratic law's multiplier does
constexpr int PSH_BLOCKS_PER_CU = 32;

// per wave: the 64 x 3 strain-in / stress-out staging, then 64 records of the six distinct tangent entries (tangent = 1 only
// writes them)
constexpr int PSH_REC = 6;
constexpr int PSH_LDS_PER_WAVE = WAVE * 3 + WAVE * PSH_REC;
constexpr int PSH_LDS_BYTES = WAVES_PER_BLOCK * PSH_LDS_PER_WAVE * 8 + 4 * WAVES_PER_BLOCK * 8;
static_assert(PSH_LDS_BYTES == 18560, "DESIGN.md states the LDS of plane_stress_hosford_kernel");
constexpr int PSH_NSLOTS = 3;   // the hidden PlasticStrain: three SoA streams

// the kernel of a law with tangent = 0 (what dxm_create asks the resources of)
__attribute__((visibility("hidden"))) const void* plane_stress_hosford_kernel_fn();

// one launch of plane_stress_hosford_kernel<tangent>; s0 / s1: slot 0 of the initial / final state at the first point of the launch
__attribute__((visibility("hidden"))) void plane_stress_hosford_launch(int tangent, int grid, hipStream_t st, const PshParams& prm, int64_t cnt,
                                                                       const double* grad, const double* s0, double* s1, int64_t ld,
                                                                       double* flux, double* ct, BlockStats* bs);

}  // namespace dxm
