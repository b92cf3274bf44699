// Host entry points of the two-dimensional heat-transfer kernels (heat_plane.hip): the laws of heat_transfer.hip with a 2-wide
// temperature gradient and heat flux, and the evaluation of a scalar Lagrange field and its gradient at the Gauss points of a plane
// mesh.  A translation unit of its own, like the other laws added after the first five (heat_transfer.hpp): dxmat.hip names no kernel
// of this unit, its device module does not change.  A custom-hardening build compiles dxmat.hip alone and never serves these.
#pragma once
#include <hip/hip_runtime.h>

#include "dxm_common.hpp"
#include "heat_transfer.hpp"   // HeatParams, HT_*: the record and the laws' constants are those of the 3-wide kernels

namespace dxm {

// doubles per point of the tangent: -k I (4, both zeros written) | dj/dT (2) [| dh/dT (1)]
constexpr int HP_WIDTH[2] = {6, 7};

// Launch shape: one sweep at 1e7 points with a temperature stream (32 / 64 / 128 / 256 workgroups per CU: 0.1332 / 0.1322 / 0.1312 /
// 0.1311 ms for law 35, 0.1871 / 0.1840 / 0.1793 / 0.1797 ms for law 36, repeats within 0.5 %; profiles/r25_heat_plane.md): 128 is
// 1.5 % and 4.2 % faster than the streaming grid of heat_transfer.hpp (32), more than the run's spread.  Other sizes, the uniform
// temperature and the nodal form were not swept
constexpr int HP_BLOCKS_PER_CU = 128;

// per wave: 64 records (-k, dj/dT[0..1], c) the tangent is written from; the 16 B gradient and flux rows need no staging
constexpr int HP_REC = 4;
constexpr int HP_LDS_PER_WAVE = WAVE * HP_REC;
constexpr int HP_LDS_BYTES = WAVES_PER_BLOCK * HP_LDS_PER_WAVE * 8 + 4 * WAVES_PER_BLOCK * 8;
// the stand-alone gradient kernel: one thread per point, no LDS
constexpr int SCALAR_GRAD_BLOCK = 256;
constexpr int SCALAR_GRAD_LDS_BYTES = 0;

// where the gradient and the temperature of a point come from
constexpr int HP_SRC_ARRAY = 0;   // a gradient array (n, 2) and a uniform temperature or one value per point
constexpr int HP_SRC_NODAL = 1;   // the nodal temperature: every lane evaluates T and grad(T) at its Gauss point (ScalarSource)

// A scalar Lagrange field on a plane mesh whose indices the host has checked (dxm_mesh_create_plane_scalar): conn (n_cells, nv) into
// coords (.., 3), dofmap (n_cells, nd) into t (n_dofs); gdphi (nqp, nv, 2), phi (nqp, nd) and dphi (nqp, nd, 2) in device memory.
// Point point0 + i of the mesh is point i of the launch.
struct ScalarSource {
  const double* coords;
  const int32_t* conn;
  const int32_t* dofmap;
  const double* gdphi;
  const double* phi;
  const double* dphi;
  const double* t;
  int64_t point0;
  int32_t nqp, nv, nd;
};

// the uniform-temperature kernel of a law (what dxm_create asks the resources of)
__attribute__((visibility("hidden"))) const void* heat_plane_stationary_kernel_fn();
__attribute__((visibility("hidden"))) const void* heat_plane_phase_change_kernel_fn();

// one launch of heat_plane_kernel<law, src != null>.  src null: the gradient rows at grad and the uniform temperature t_uniform, or
// with tfield one value per point at the first point of the launch.  src not null: grad, t_uniform and tfield are not read.
// enthalpy: slot 0 of the final state at the first point (phase change only)
__attribute__((visibility("hidden"))) void heat_plane_launch(int law, int grid, hipStream_t st, const HeatParams& prm, int64_t cnt,
                                                             const double* grad, double t_uniform, const double* tfield,
                                                             const ScalarSource* src, double* enthalpy, double* flux, double* ct,
                                                             BlockStats* bs);

// grad(T) = Ji^T sum_m T_m dphi_m (npts, 2) and, where value is not null, T = sum_m T_m phi_m (npts) at the first npts points from
// src.point0 on.  Returns the launch's hipError_t.
__attribute__((visibility("hidden"))) hipError_t scalar_gradient_launch(hipStream_t st, const ScalarSource& src, int64_t npts, double* grad,
                                                                       double* value);

}  // namespace dxm
