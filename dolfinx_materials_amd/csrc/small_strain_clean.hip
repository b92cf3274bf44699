// The J2 update kernels that skip the state store of tiles whose state did not change (small_strain_clean.hpp says what they keep
// and why they are not in dxmat.hip): small_strain_body.hpp with CLEAN = true, strain-array form, uniform parameters.
#include "small_strain_clean.hpp"

#define DXM_UPDATE_KERNELS_ONLY
#include "small_strain.hpp"

namespace dxm {

template <int LAW, int TL, int GRAD = 0>
__global__ void __launch_bounds__(BLOCK, 4)
small_strain_clean_kernel(const LawParams prm, const int64_t n, const double* __restrict__ eps,
                          const double* __restrict__ s0, double* __restrict__ s1, const int64_t ld,
                          double* __restrict__ sig, double* __restrict__ ct,
                          BlockStats* __restrict__ stats, uint32_t* __restrict__ stamps, const uint32_t stamp) {
  static_assert(ss_has_state<LAW> && GRAD == 0, "the J2 laws, strain from the (N, 6) array");
  constexpr bool FIELDS = false;
  constexpr ParamStreams pf = {};
  constexpr bool CLEAN = true;
  constexpr int PACKED = 0;
  constexpr unsigned long long* pack_mask = nullptr;   // named by the discarded PACKED blocks of the body only
  constexpr double* pack_buf = nullptr;
  MeshSource src{};   // named by the discarded GRAD != 0 blocks of the body only (not const: they divide by a member of it)
#include "small_strain_body.hpp"
}

const void* small_strain_clean_kernel_ptr() { return (const void*)small_strain_clean_kernel<LAW_J2_LINEAR, TL_FULL>; }

bool small_strain_clean_launch(int law, int tl, int grid, int dyn_lds, hipStream_t st, const LawParams& prm, int64_t cnt,
                               const double* grad, const double* s0, double* s1, int64_t ld, double* flux, double* ct,
                               BlockStats* bs, uint32_t* stamps, uint32_t stamp) {
#define DXM_LAUNCH_CLEAN(LAW, TL)                                                                                      \
  hipLaunchKernelGGL((small_strain_clean_kernel<LAW, TL>), dim3(grid), dim3(BLOCK), dyn_lds, st, prm, cnt, grad, s0, s1, ld, \
                     flux, ct, bs, stamps, stamp)
#define DXM_LAUNCH_CLEAN_TL(LAW) do { if (tl == TL_SYM) DXM_LAUNCH_CLEAN(LAW, TL_SYM); else if (tl == TL_FULL) DXM_LAUNCH_CLEAN(LAW, TL_FULL); \
                                      else if (tl == TL_PACK4) DXM_LAUNCH_CLEAN(LAW, TL_PACK4); else DXM_LAUNCH_CLEAN(LAW, TL_COEF); } while (0)
  if (law == LAW_J2_LINEAR) DXM_LAUNCH_CLEAN_TL(LAW_J2_LINEAR);
  else if (law == LAW_J2_VOCE) DXM_LAUNCH_CLEAN_TL(LAW_J2_VOCE);
  else return false;
#undef DXM_LAUNCH_CLEAN_TL
#undef DXM_LAUNCH_CLEAN
  return true;
}

}  // namespace dxm
