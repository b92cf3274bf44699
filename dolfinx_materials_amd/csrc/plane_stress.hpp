// Host entry points of the plane-stress return-mapping kernels (plane_stress.hip).  A translation unit of its own, like the other
// laws added after the first five: compiled into the device module of dxmat.hip, new kernels change the code generated for the
// existing ones (ramberg_osgood.hpp).  A custom-hardening build compiles dxmat.hip alone and never serves these laws.
#pragma once
#include <hip/hip_runtime.h>

#include "dxm_common.hpp"

namespace dxm {

constexpr int PS_QUADRATIC = 0, PS_POLYGON = 1;
constexpr int PS_MAX_PLANES = 4, PS_MAX_VERTICES = 6;

// What the kernels read, formed on the host once per launch from the handle's parameters (dxmat.hip::launch_plane_stress): every
// entry is a parameter or a few individually rounded operations on parameters, written out there, so that a restatement forms the
// same bits.
//   both surfaces: the plane-stress stiffness of cvxpy_materials.py:16-18, C11 = E / (1 - nu^2), C12 = C11 nu, C33 = C11 (1 - nu)
//   quadratic:     the basis a = (s0 + s1) / sqrt 2, b = (s0 - s1) / sqrt 2, c = s2 diagonalises C and Q at once
//   polygon:       per half-plane n . (sI, sII) <= d: n, d, w = M^-1 n (M^-1 the stiffness of the principal values) and n . w; then
//                  the admissible vertices of the polygon, which depend on the parameters alone and are found on the host
struct PsParams {
  double p[12 + 8 * PS_MAX_PLANES + 2 * PS_MAX_VERTICES];
  int32_t maxit;     // quadratic: cap of the multiplier's Newton (dxm_set_newton)
  int32_t planes;    // polygon: M
  int32_t vertices;  // polygon: admissible intersections of two non-parallel rows
  int32_t pad;
};
constexpr int PS_C11 = 0, PS_C12 = 1, PS_C33 = 2,
              PS_E = 3, PS_NU = 4,
              PS_CA = 5,     // E / (1 - nu): C on a
              PS_CB = 6,     // E / (1 + nu): C on b and c
              PS_QC = 7,     // q: Q on c (Q on a and b: 1/2 and 3/2)
              PS_SIG0 = 8,
              PS_TOL = 9,    // rtol sig0: the bound on sqrt(s^T Q s) - sig0
              PS_KMAX = 10,  // max_i Q_i C_i
              PS_SIG0SQ = 11,
              PS_PLANE = 12; // first half-plane; each takes PS_PLANE_REC doubles
constexpr int PS_PLANE_REC = 8;
constexpr int PS_VERTEX = PS_PLANE + PS_PLANE_REC * PS_MAX_PLANES;   // first vertex, (sI, sII) each
constexpr int PL_N1 = 0, PL_N2 = 1, PL_D = 2, PL_W1 = 3, PL_W2 = 4, PL_NW = 5,
              PL_SLACK = 6;   // 8 eps d: what an admissible candidate may exceed a row it was not built from by

// Launch shape: DESIGN.md section 3's streaming grid (the heat-transfer kernels').  The multiplier's Newton makes the tiles of the
// quadratic law cost unequally, as the Voce kernel's do, which prefers 256: here 256 is 4-10 % slower than 32 on mixed and yielded
// batches of both laws at 1e7 points and equal on elastic ones, 64 is within the spread of 32 (profiles/r20_plane_stress.md)
constexpr int PS_BLOCKS_PER_CU = 32;

// per wave: the 64 x 3 strain-in / stress-out staging, then 64 records of the six distinct tangent entries (tangent = 1 only
// writes them)
constexpr int PS_REC = 6;
constexpr int PS_LDS_PER_WAVE = WAVE * 3 + WAVE * PS_REC;
constexpr int PS_LDS_BYTES = WAVES_PER_BLOCK * PS_LDS_PER_WAVE * 8 + 4 * WAVES_PER_BLOCK * 8;
constexpr int PS_NSLOTS = 3;   // the hidden PlasticStrain: three SoA streams

// the kernel of a law with tangent = 0 (what dxm_create asks the resources of)
__attribute__((visibility("hidden"))) const void* plane_stress_quadratic_kernel_fn();
__attribute__((visibility("hidden"))) const void* plane_stress_polygon_kernel_fn();

// one launch of plane_stress_kernel<surface, tangent>; s0 / s1: slot 0 of the initial / final state at the first point of the launch
__attribute__((visibility("hidden"))) void plane_stress_launch(int surface, int tangent, int grid, hipStream_t st, const PsParams& prm, int64_t cnt,
                                                               const double* grad, const double* s0, double* s1, int64_t ld, double* flux,
                                                               double* ct, BlockStats* bs);

}  // namespace dxm
