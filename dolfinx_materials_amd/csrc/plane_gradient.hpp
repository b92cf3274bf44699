// Host entry point of the plane gradient kernels (plane_gradient.hip): the displacement gradient at the Gauss points of a
// two-dimensional mesh -- triangles or bilinear quadrilaterals with a Lagrange displacement of any order -- written as what the 2-D
// laws read: the plane-strain 4-vector of plane_strain.hip, the in-plane 3-vector of plane_stress*.hip, or embedded in the 6-wide
// Mandel strain / the 9-wide F of the other laws.  A translation unit of its own, like the laws added after the first five
// (plane_strain.hpp): dxmat.hip names no kernel of this unit, its device module does not change.
//
// Mapping: the one gradient.hpp documents.  One thread per Gauss point, 256-thread blocks; every lane gathers the vertices and dofs
// of its own cell (the lanes of a cell ask for the same lines), the two tables are a few hundred bytes and stay in the vector L1.
// No LDS, no barrier.
//
// Output rows.  Kind 2 (32 B): two aligned 16 B stores per lane, like the 48 B rows of kind 0.  Kind 3 (24 B): a row is 16 B aligned
// at even points only, so the source writes it with three 8 B stores per lane, which the compiler issues as one 16 B and one 8 B
// store at 8 B alignment (global stores need dword alignment only); the store instructions of a wave cover the same 1536 contiguous
// bytes between them, which the L2 merges into whole lines before they leave for HBM (the 9-wide rows of kind 1 have been written
// this way since the first gradient kernel).  Chosen because it needs no LDS, no barrier and no special case for the ragged last
// block: a lane writes its own row or nothing.  Measured (profiles/r24_plane_gradient.md): 0.69-0.76 of the time of the 48 B rows of
// simplex_gradient_kernel<0> where the bytes written say 0.5, kind 2 0.76-0.81 where they say 0.67 -- the reads and the arithmetic
// do not shrink with the row.  OPEN: staging a wave's 1536 B through LDS and writing them as 96 aligned 16 B stores is UNMEASURED
// against this; the tool is tools/bench_plane_gradient.py.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dxm {

// what dxm_mesh_gradient_device calls `kind`
constexpr int GRAD_STRAIN6 = 0;         // [H00, H11, 0, r (H01 + H10), 0, 0] on a plane mesh, r = sqrt(2)/2
constexpr int GRAD_F9 = 1;              // F = I + H, F_zz = 1
constexpr int GRAD_PLANE_STRAIN4 = 2;   // [H00, H11, 0.0, r (H01 + H10)]
constexpr int GRAD_IN_PLANE3 = 3;       // [H00, H11, r (H01 + H10)]
constexpr int PLANE_GRAD_WIDTH[4] = {6, 9, 4, 3};   // doubles per output row

constexpr int PLANE_GRAD_BLOCK = 256;
constexpr int PLANE_GRAD_LDS_BYTES = 0;
constexpr int PLANE_GRAD_MAX_ND = 64, PLANE_GRAD_MAX_NQP = 64;   // the bounds of dxm_mesh_create_simplex

// one launch of plane_gradient_kernel<kind> over the n_cells * nqp points of a mesh whose indices the caller has checked:
// conn (n_cells, nv) into coords (.., 3), dofmap (n_cells, nd) into u (.., 2); gdphi (nqp, nv, 2) and dphi (nqp, nd, 2) in device
// memory.  Returns the launch's hipError_t.
__attribute__((visibility("hidden"))) hipError_t plane_gradient_launch(int kind, hipStream_t st, const double* coords, const int32_t* conn,
                                                                      int nv, const int32_t* dofmap, int nd, const double* gdphi,
                                                                      const double* dphi, int nqp, int64_t n_cells, const double* u,
                                                                      double* grad);

}  // namespace dxm
