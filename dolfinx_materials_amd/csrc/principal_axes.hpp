// What the laws evaluated in principal axes share (hyperelastic.hip: C = F^T F; hosford.hip: the deviatoric trial stress): the
// register-only cyclic Jacobi rotation, the series of sinh(y) / y that their divided differences switch to near repeated
// eigenvalues.  Ordinary functions, unlike the tile I/O steps (tile_*.hpp): both kernels compile to the same code with them here.
#pragma once
#include "dxm_common.hpp"

namespace dxm {

// one Jacobi rotation in the (p, q) plane of a symmetric 3x3 (r: the third index); vp / vq: the two eigenvector columns
__device__ __forceinline__ void jacobi_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double* vp, double* vq) {
  const double d = aqq - app;
  const double den = d + copysign(sqrt(d * d + 4.0 * apq * apq), d);
  // t = tan of the rotation angle, the smaller root; an already-zero entry (den == 0 needs apq == 0 too) is left alone
  const double t = den != 0.0 ? 2.0 * apq * fast_rcp(den) : 0.0;
  const double c = fast_rcp(sqrt(t * t + 1.0));
  const double s = t * c;
  app -= t * apq;
  aqq += t * apq;
  apq = 0.0;
  const double rp = arp, rq = arq;
  arp = c * rp - s * rq;
  arq = s * rp + c * rq;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double xp = vp[k], xq = vq[k];
    vp[k] = c * xp - s * xq;
    vq[k] = s * xp + c * xq;
  }
}

// sinh(y) / y from y^2, |y| <= 0.1 (five terms of the even series: 2e-22 at |y| = 0.1)
__device__ __forceinline__ double sinhc_series(double y2) {
  return 1.0 + y2 * (1.0 / 6.0) * (1.0 + y2 * (1.0 / 20.0) * (1.0 + y2 * (1.0 / 42.0) * (1.0 + y2 * (1.0 / 72.0) * (1.0 + y2 * (1.0 / 110.0)))));
}

}  // namespace dxm
