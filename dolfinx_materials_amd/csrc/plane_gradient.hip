// The plane gradient kernels: plane_gradient.hpp has the mapping and the choice of the output-row stores.
//
// Per point (xi: reference coordinates, gdphi: the geometry's table, dphi: the field's):
//   J[a][d]  = sum_v X_v[a] gdphi[q][v][d]      dX_a / dxi_d from the nv vertices of the cell
//   Ji       = the 2 x 2 cofactor inverse of J   dxi_d / dX_a
//   B[i][d]  = sum_m u_m[i] dphi[q][m][d]        du_i / dxi_d from the nd dofs of the cell
//   H        = B Ji                              H[i][a] = du_i / dX_a
// J is rebuilt at every point: it is constant on a triangle, not on a quadrilateral, and one kernel serves both (six more fused
// multiply-adds per vertex against a kernel that is bound by its output stream).
#include "plane_gradient.hpp"

#include "dxm_common.hpp"

namespace dxm {

struct PlaneSource {
  const double* coords;     // (n_vertices, 3), third column ignored
  const int32_t* conn;      // (n_cells, nv)
  const int32_t* dofmap;    // (n_cells, nd)
  const double* gdphi;      // (nqp, nv, 2)
  const double* dphi;       // (nqp, nd, 2)
  const double* u;          // (n_dofs, 2)
  int64_t npts;
  int32_t nqp, nv, nd;
};

template <int KIND>
__global__ void __launch_bounds__(PLANE_GRAD_BLOCK)
plane_gradient_kernel(const PlaneSource s, double* __restrict__ grad) {
  const int64_t gid = (int64_t)blockIdx.x * PLANE_GRAD_BLOCK + threadIdx.x;
  if (gid >= s.npts) return;   // a ragged last block: a lane writes its own row or nothing
  const int64_t cell = gid / s.nqp;
  const int q = (int)(gid - cell * s.nqp);

  double J00 = 0.0, J01 = 0.0, J10 = 0.0, J11 = 0.0;
  {
    const int32_t* vs = s.conn + cell * s.nv;
    const double* tab = s.gdphi + (int64_t)q * s.nv * 2;
    for (int v = 0; v < s.nv; ++v) {
      const int64_t vert = vs[v];
      const double t0 = tab[2 * v], t1 = tab[2 * v + 1];
      const double X0 = s.coords[3 * vert], X1 = s.coords[3 * vert + 1];
      J00 += X0 * t0; J01 += X0 * t1;
      J10 += X1 * t0; J11 += X1 * t1;
    }
  }
  double B00 = 0.0, B01 = 0.0, B10 = 0.0, B11 = 0.0;
  {
    const int32_t* dofs = s.dofmap + cell * s.nd;
    const double* tab = s.dphi + (int64_t)q * s.nd * 2;
#pragma unroll 2
    for (int m = 0; m < s.nd; ++m) {
      const int64_t dof = dofs[m];
      const double t0 = tab[2 * m], t1 = tab[2 * m + 1];
      const double U0 = s.u[2 * dof], U1 = s.u[2 * dof + 1];
      B00 += U0 * t0; B01 += U0 * t1;
      B10 += U1 * t0; B11 += U1 * t1;
    }
  }
  const double idet = 1.0 / (J00 * J11 - J01 * J10);
  const double i00 = J11 * idet, i01 = -J01 * idet, i10 = -J10 * idet, i11 = J00 * idet;
  const double H00 = B00 * i00 + B01 * i10, H01 = B00 * i01 + B01 * i11;
  const double H10 = B10 * i00 + B11 * i10, H11 = B10 * i01 + B11 * i11;
  const double r = 0.70710678118654752440;   // sqrt(2) * (1/2)
  const double shear = r * (H01 + H10);

  if constexpr (KIND == GRAD_STRAIN6) {
    double2_t* o2 = reinterpret_cast<double2_t*>(grad + gid * 6);   // 48 B per point: 16 B aligned
    o2[0] = double2_t{H00, H11};
    o2[1] = double2_t{0.0, shear};
    o2[2] = double2_t{0.0, 0.0};
  } else if constexpr (KIND == GRAD_F9) {
    double* o = grad + gid * 9;
    o[0] = 1.0 + H00; o[1] = 1.0 + H11; o[2] = 1.0;
    o[3] = H01; o[4] = H10; o[5] = 0.0; o[6] = 0.0; o[7] = 0.0; o[8] = 0.0;
  } else if constexpr (KIND == GRAD_PLANE_STRAIN4) {
    double2_t* o2 = reinterpret_cast<double2_t*>(grad + gid * 4);   // 32 B per point: 16 B aligned
    o2[0] = double2_t{H00, H11};
    o2[1] = double2_t{0.0, shear};
  } else {
    double* o = grad + gid * 3;                                     // 24 B per point: 8 B stores (plane_gradient.hpp)
    o[0] = H00; o[1] = H11; o[2] = shear;
  }
}

hipError_t plane_gradient_launch(int kind, hipStream_t st, const double* coords, const int32_t* conn, int nv, const int32_t* dofmap,
                                 int nd, const double* gdphi, const double* dphi, int nqp, int64_t n_cells, const double* u,
                                 double* grad) {
  PlaneSource s{};
  s.coords = coords; s.conn = conn; s.dofmap = dofmap; s.gdphi = gdphi; s.dphi = dphi; s.u = u;
  s.npts = n_cells * nqp; s.nqp = nqp; s.nv = nv; s.nd = nd;
  if (s.npts <= 0) return hipSuccess;
  const dim3 grid((unsigned)((s.npts + PLANE_GRAD_BLOCK - 1) / PLANE_GRAD_BLOCK)), block(PLANE_GRAD_BLOCK);
  switch (kind) {
    case GRAD_STRAIN6: hipLaunchKernelGGL(plane_gradient_kernel<GRAD_STRAIN6>, grid, block, 0, st, s, grad); break;
    case GRAD_F9: hipLaunchKernelGGL(plane_gradient_kernel<GRAD_F9>, grid, block, 0, st, s, grad); break;
    case GRAD_PLANE_STRAIN4: hipLaunchKernelGGL(plane_gradient_kernel<GRAD_PLANE_STRAIN4>, grid, block, 0, st, s, grad); break;
    case GRAD_IN_PLANE3: hipLaunchKernelGGL(plane_gradient_kernel<GRAD_IN_PLANE3>, grid, block, 0, st, s, grad); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace dxm
