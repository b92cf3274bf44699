// The Ramberg-Osgood instantiations of small_strain_kernel (ramberg_osgood.hpp says why they are not in dxmat.hip).
#include "ramberg_osgood.hpp"

#define DXM_UPDATE_KERNELS_ONLY
#include "small_strain.hpp"

namespace dxm {

const void* ramberg_osgood_kernel() { return (const void*)small_strain_kernel<LAW_RAMBERG_OSGOOD, TL_FULL, 0>; }

void ramberg_osgood_launch(int tl, int grad_kind, int grid, hipStream_t st, const LawParams& prm, int64_t cnt, const double* grad,
                           double* flux, double* ct, BlockStats* bs, const MeshSource& src) {
  // no state: the kernel never reads s0 or writes s1
#define DXM_LAUNCH_RO(TL, G)                                                                                              \
  hipLaunchKernelGGL((small_strain_kernel<LAW_RAMBERG_OSGOOD, TL, G>), dim3(grid), dim3(BLOCK), RO_DYN_LDS, st, prm, cnt, grad, \
                     nullptr, nullptr, (int64_t)0, flux, ct, bs, src)
#define DXM_LAUNCH_RO_G(TL) do { if (grad_kind == 0) DXM_LAUNCH_RO(TL, 0); else if (grad_kind == 1) DXM_LAUNCH_RO(TL, 1); \
                                 else if (grad_kind == 2) DXM_LAUNCH_RO(TL, 2); else DXM_LAUNCH_RO(TL, 3); } while (0)
  if (tl == TL_SYM) DXM_LAUNCH_RO_G(TL_SYM);
  else if (tl == TL_FULL) DXM_LAUNCH_RO_G(TL_FULL);
  else if (tl == TL_PACK4) DXM_LAUNCH_RO_G(TL_PACK4);
  else DXM_LAUNCH_RO_G(TL_COEF);
#undef DXM_LAUNCH_RO_G
#undef DXM_LAUNCH_RO
}

}  // namespace dxm
