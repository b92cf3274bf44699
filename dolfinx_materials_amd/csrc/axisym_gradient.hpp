// Host entry point of the axisymmetric gradient kernels (axisym_gradient.hip): the displacement gradient at the Gauss points of a
// MERIDIAN mesh -- triangles or bilinear quadrilaterals in the (r, z) half plane with a Lagrange displacement (u_r, u_z) of any order
// -- written as what the laws read under MGIS's axisymmetric hypothesis: the 4-vector [rr, zz, tt, sqrt(2) rz], the 5-wide F
// [F_rr, F_zz, F_tt, F_rz, F_zr], or either embedded in the 6-wide Mandel strain / the 9-wide F.  The slots are those of the plane-strain
// hypothesis; what differs is the hoop term eps_tt = u_r / r, F_tt = 1 + u_r / r, which needs the VALUES of the field's shape functions
// (u_r) and of the geometry's (r) at the Gauss points beside the derivative tables plane_gradient.hip reads.  A translation unit of its
// own, like plane_gradient.hip: dxmat.hip names no kernel of this unit, its device module does not change.
//
// Mapping: the one plane_gradient.hpp documents (x = r, y = z).  One thread per Gauss point, 256-thread blocks; every lane gathers the
// vertices and dofs of its own cell (the lanes of a cell ask for the same lines), the four tables are a few hundred bytes and stay in
// the vector L1.  No LDS, no barrier.  The sums run in the tables' local order from 0.0, each product fused with its sum as in
// plane_gradient.hip (axisym_gradient.hip says why), so a restatement in the same order is comparable at rounding level.
//
// Output rows, by the reasoning plane_gradient.hpp records.  Kinds 0 (32 B) and 2 (48 B): two / three aligned 16 B stores per lane.
// Kinds 1 (40 B) and 3 (72 B): a row is 16 B aligned at even points only, so the source writes 8 B stores, which the compiler may pair
// at 8 B alignment (global stores need dword alignment only); the stores of a wave cover the same 2560 / 4608 contiguous bytes between
// them, which the L2 merges into whole lines.  A lane writes its own row or nothing.  The optional radius array takes one 8 B store
// per lane (512 contiguous bytes per wave).  Measured (profiles/r29_axisym_gradient.md): kind 0 takes 1.05-1.12 of the time of
// plane_gradient_kernel<2> on the same cells, 1.08-1.22 with the radius.  OPEN: kinds 1 to 3, and the 40 B / 72 B rows staged through LDS,
// are UNMEASURED; the tool is tools/bench_axisym_gradient.py.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dxm {

// what dxm_mesh_axisymmetric_gradient_device calls `kind` (numbered by that entry point alone); hoop = u_r / r, s = sqrt(2)/2
constexpr int AXI_STRAIN4 = 0;   // [H00, H11, hoop, s (H01 + H10)]
constexpr int AXI_F5 = 1;        // [1 + H00, 1 + H11, 1 + hoop, H01, H10]
constexpr int AXI_STRAIN6 = 2;   // [H00, H11, hoop, s (H01 + H10), 0, 0]
constexpr int AXI_F9 = 3;        // [1 + H00, 1 + H11, 1 + hoop, H01, H10, 0, 0, 0, 0]
constexpr int AXISYM_GRAD_WIDTH[4] = {4, 5, 6, 9};   // doubles per output row

constexpr int AXISYM_GRAD_BLOCK = 256;
constexpr int AXISYM_GRAD_LDS_BYTES = 0;

// A displacement on a meridian mesh whose indices, det J and radii the host has checked (dxm_mesh_create_axisymmetric): conn
// (n_cells, nv) into coords (.., 3) with column 0 = r and column 1 = z, dofmap (n_cells, nd) into u (.., 2); gphi (nqp, nv), gdphi
// (nqp, nv, 2), phi (nqp, nd) and dphi (nqp, nd, 2) in device memory.
struct AxisymSource {
  const double* coords;
  const int32_t* conn;
  const int32_t* dofmap;
  const double* gphi;
  const double* gdphi;
  const double* phi;
  const double* dphi;
  const double* u;
  int64_t npts;
  int32_t nqp, nv, nd;
};

// one launch of axisym_gradient_kernel<kind, radius != null> over the s.npts points: grad (npts, AXISYM_GRAD_WIDTH[kind]), 16 B
// aligned for kinds 0 and 2; radius (npts) or null.  Returns the launch's hipError_t.
__attribute__((visibility("hidden"))) hipError_t axisym_gradient_launch(int kind, hipStream_t st, const AxisymSource& s, double* grad,
                                                                       double* radius);

}  // namespace dxm
