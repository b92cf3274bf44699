// The axisymmetric gradient kernels: axisym_gradient.hpp has the mapping and the choice of the output-row stores.
//
// Per point, with x = r and y = z (xi: reference coordinates; gphi / gdphi: the geometry's tables, phi / dphi: the field's):
//   J[a][d]  = sum_v X_v[a] gdphi[q][v][d]      dX_a / dxi_d from the nv vertices of the cell
//   rad      = sum_v X_v[0] gphi[q][v]          r at the point
//   Ji       = the 2 x 2 cofactor inverse of J   dxi_d / dX_a
//   B[i][d]  = sum_m u_m[i] dphi[q][m][d]        du_i / dxi_d from the nd dofs of the cell
//   ur       = sum_m u_m[0] phi[q][m]           u_r at the point
//   H        = B Ji                              H[i][a] = du_i / dX_a;   hoop = ur / rad
// J, B, Ji and H are the text of plane_gradient.hip; the sums run in the tables' local order from 0.0.  The library is compiled with
// -ffp-contract=fast, under which the compiler fuses each product with the sum it feeds whatever a contraction pragma says (28
// v_fmac_f64 per instantiation): a restatement that rounds every operation on its own agrees at rounding level, not bit for bit.
#include "axisym_gradient.hpp"

#include "dxm_common.hpp"

namespace dxm {

template <int KIND, bool RADIUS>
__global__ void __launch_bounds__(AXISYM_GRAD_BLOCK)
axisym_gradient_kernel(const AxisymSource s, double* __restrict__ grad, double* __restrict__ radius) {
  const int64_t gid = (int64_t)blockIdx.x * AXISYM_GRAD_BLOCK + threadIdx.x;
  if (gid >= s.npts) return;   // a ragged last block: a lane writes its own row or nothing
  const int64_t cell = gid / s.nqp;
  const int q = (int)(gid - cell * s.nqp);

  double J00 = 0.0, J01 = 0.0, J10 = 0.0, J11 = 0.0, rad = 0.0;
  {
    const int32_t* vs = s.conn + cell * s.nv;
    const double* tab = s.gdphi + (int64_t)q * s.nv * 2;
    const double* ptab = s.gphi + (int64_t)q * s.nv;
    for (int v = 0; v < s.nv; ++v) {
      const int64_t vert = vs[v];
      const double t0 = tab[2 * v], t1 = tab[2 * v + 1];
      const double X0 = s.coords[3 * vert], X1 = s.coords[3 * vert + 1];
      J00 = J00 + X0 * t0; J01 = J01 + X0 * t1;
      J10 = J10 + X1 * t0; J11 = J11 + X1 * t1;
      rad = rad + X0 * ptab[v];
    }
  }
  double B00 = 0.0, B01 = 0.0, B10 = 0.0, B11 = 0.0, ur = 0.0;
  {
    const int32_t* dofs = s.dofmap + cell * s.nd;
    const double* tab = s.dphi + (int64_t)q * s.nd * 2;
    const double* ptab = s.phi + (int64_t)q * s.nd;
#pragma unroll 2
    for (int m = 0; m < s.nd; ++m) {
      const int64_t dof = dofs[m];
      const double t0 = tab[2 * m], t1 = tab[2 * m + 1];
      const double U0 = s.u[2 * dof], U1 = s.u[2 * dof + 1];
      B00 = B00 + U0 * t0; B01 = B01 + U0 * t1;
      B10 = B10 + U1 * t0; B11 = B11 + U1 * t1;
      ur = ur + U0 * ptab[m];
    }
  }
  const double idet = 1.0 / (J00 * J11 - J01 * J10);
  const double i00 = J11 * idet, i01 = -J01 * idet, i10 = -J10 * idet, i11 = J00 * idet;
  const double H00 = B00 * i00 + B01 * i10, H01 = B00 * i01 + B01 * i11;
  const double H10 = B10 * i00 + B11 * i10, H11 = B10 * i01 + B11 * i11;
  const double hoop = ur / rad;
  const double r = 0.70710678118654752440;   // sqrt(2) * (1/2)
  const double shear = r * (H01 + H10);

  if constexpr (KIND == AXI_STRAIN4) {
    double2_t* o2 = reinterpret_cast<double2_t*>(grad + gid * 4);   // 32 B per point: 16 B aligned
    o2[0] = double2_t{H00, H11};
    o2[1] = double2_t{hoop, shear};
  } else if constexpr (KIND == AXI_STRAIN6) {
    double2_t* o2 = reinterpret_cast<double2_t*>(grad + gid * 6);   // 48 B per point: 16 B aligned
    o2[0] = double2_t{H00, H11};
    o2[1] = double2_t{hoop, shear};
    o2[2] = double2_t{0.0, 0.0};
  } else if constexpr (KIND == AXI_F5) {
    double* o = grad + gid * 5;                                     // 40 B per point: 8 B stores (axisym_gradient.hpp)
    o[0] = 1.0 + H00; o[1] = 1.0 + H11; o[2] = 1.0 + hoop;
    o[3] = H01; o[4] = H10;
  } else {
    double* o = grad + gid * 9;                                     // 72 B per point: 8 B stores
    o[0] = 1.0 + H00; o[1] = 1.0 + H11; o[2] = 1.0 + hoop;
    o[3] = H01; o[4] = H10; o[5] = 0.0; o[6] = 0.0; o[7] = 0.0; o[8] = 0.0;
  }
  if constexpr (RADIUS) radius[gid] = rad;
}

template <int KIND>
static void launch_kind(dim3 grid, dim3 block, hipStream_t st, const AxisymSource& s, double* grad, double* radius) {
  if (radius) hipLaunchKernelGGL((axisym_gradient_kernel<KIND, true>), grid, block, 0, st, s, grad, radius);
  else hipLaunchKernelGGL((axisym_gradient_kernel<KIND, false>), grid, block, 0, st, s, grad, radius);
}

hipError_t axisym_gradient_launch(int kind, hipStream_t st, const AxisymSource& s, double* grad, double* radius) {
  if (s.npts <= 0) return hipSuccess;
  const dim3 grid((unsigned)((s.npts + AXISYM_GRAD_BLOCK - 1) / AXISYM_GRAD_BLOCK)), block(AXISYM_GRAD_BLOCK);
  switch (kind) {
    case AXI_STRAIN4: launch_kind<AXI_STRAIN4>(grid, block, st, s, grad, radius); break;
    case AXI_F5: launch_kind<AXI_F5>(grid, block, st, s, grad, radius); break;
    case AXI_STRAIN6: launch_kind<AXI_STRAIN6>(grid, block, st, s, grad, radius); break;
    case AXI_F9: launch_kind<AXI_F9>(grid, block, st, s, grad, radius); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace dxm
