// The per-point parameter-field instantiations of the J2 small-strain kernels (param_fields.hpp says why they are not in dxmat.hip).
#include "param_fields.hpp"

#define DXM_UPDATE_KERNELS_ONLY
#include "small_strain.hpp"

namespace dxm {

// Lame coefficients per point: dxmat.hip::build_params' two lines.  No product feeds an add here except 2 nu (exact), so a
// contraction cannot change a bit; the divisions are the correctly rounded ones.
__global__ void __launch_bounds__(256)
elastic_streams_kernel(const int64_t n, const double* __restrict__ E_dev, const double E_u, const double* __restrict__ nu_dev,
                       const double nu_u, double* __restrict__ lambda, double* __restrict__ mu) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double E = E_dev ? E_dev[i] : E_u;
    const double nu = nu_dev ? nu_dev[i] : nu_u;
    lambda[i] = E * nu / (1 + nu) / (1 - 2 * nu);
    mu[i] = E / 2 / (1 + nu);
  }
}

void param_fields_elastic_streams(int64_t n, const double* E_dev, double E_u, const double* nu_dev, double nu_u, double* lambda_dev,
                                  double* mu_dev, hipStream_t st) {
  if (n <= 0) return;
  int64_t blocks = (n + 255) / 256;
  if (blocks > 65536) blocks = 65536;   // grid-stride beyond
  hipLaunchKernelGGL(elastic_streams_kernel, dim3((unsigned)blocks), dim3(256), 0, st, n, E_dev, E_u, nu_dev, nu_u, lambda_dev, mu_dev);
}

template <int LAW>
static void launch_fields(int tl, int g, int grid, int dyn_lds, hipStream_t st, const LawParams& prm, const ParamStreams& pf, int64_t cnt,
                          const double* grad, const double* s0, double* s1, int64_t ld, double* flux, double* ct, BlockStats* bs,
                          const MeshSource& src) {
#define DXM_LAUNCH_PF(TL, G)                                                                                                      \
  hipLaunchKernelGGL((small_strain_field_kernel<LAW, TL, G>), dim3(grid), dim3(BLOCK), dyn_lds, st, prm, pf, cnt, grad, s0, s1, ld, \
                     flux, ct, bs, src)
#define DXM_LAUNCH_PF_G(TL) do { if (g == 0) DXM_LAUNCH_PF(TL, 0); else if (g == 1) DXM_LAUNCH_PF(TL, 1); \
                                 else if (g == 2) DXM_LAUNCH_PF(TL, 2); else DXM_LAUNCH_PF(TL, 3); } while (0)
  if (tl == TL_SYM) DXM_LAUNCH_PF_G(TL_SYM);
  else if (tl == TL_FULL) DXM_LAUNCH_PF_G(TL_FULL);
  else if (tl == TL_PACK4) DXM_LAUNCH_PF_G(TL_PACK4);
  else DXM_LAUNCH_PF_G(TL_COEF);
#undef DXM_LAUNCH_PF_G
#undef DXM_LAUNCH_PF
}

bool param_fields_launch(int law, int tl, int grad_kind, int grid, int dyn_lds, hipStream_t st, const LawParams& prm,
                         const ParamStreams& pf, int64_t cnt, const double* grad, const double* s0, double* s1, int64_t ld, double* flux,
                         double* ct, BlockStats* bs, const MeshSource& src) {
  if (law == LAW_J2_LINEAR) launch_fields<LAW_J2_LINEAR>(tl, grad_kind, grid, dyn_lds, st, prm, pf, cnt, grad, s0, s1, ld, flux, ct, bs, src);
  else if (law == LAW_J2_VOCE) launch_fields<LAW_J2_VOCE>(tl, grad_kind, grid, dyn_lds, st, prm, pf, cnt, grad, s0, s1, ld, flux, ct, bs, src);
  else return false;
  return true;
}

}  // namespace dxm
