// The J2 update kernels that read the old state of a load step from a packed copy of s0 (small_strain_clean.hpp says what the copy
// holds): small_strain_body.hpp with CLEAN = true and PACKED = 1 (build) or 2 (use), strain-array form, uniform parameters.  A
// translation unit of their own for the reason small_strain_clean.hpp gives: the device modules of the other units -- that of
// small_strain_clean.hip among them -- compile to the instruction streams they had before these kernels existed.
#include "small_strain_clean.hpp"

#define DXM_UPDATE_KERNELS_ONLY
#include "small_strain.hpp"

namespace dxm {

// The clean kernel with the packed copy of s0 (small_strain_clean.hpp): PACKED = 1 reads s0 and builds the copy, PACKED = 2 reads the
// copy instead of s0.
template <int LAW, int TL, int PACKED>
__global__ void __launch_bounds__(BLOCK, 4)
small_strain_packed_kernel(const LawParams prm, const int64_t n, const double* __restrict__ eps,
                           const double* __restrict__ s0, double* __restrict__ s1, const int64_t ld,
                           double* __restrict__ sig, double* __restrict__ ct,
                           BlockStats* __restrict__ stats, uint32_t* __restrict__ stamps, const uint32_t stamp,
                           unsigned long long* __restrict__ pack_mask, double* __restrict__ pack_buf) {
  static_assert(ss_has_state<LAW> && (PACKED == 1 || PACKED == 2), "the J2 laws; build or use");
  constexpr int GRAD = 0;
  constexpr bool FIELDS = false;
  constexpr ParamStreams pf = {};
  constexpr bool CLEAN = true;
  MeshSource src{};
#include "small_strain_body.hpp"
}

const void* small_strain_packed_kernel_ptr(int packed) {
  return packed == 1 ? (const void*)small_strain_packed_kernel<LAW_J2_LINEAR, TL_FULL, 1> : (const void*)small_strain_packed_kernel<LAW_J2_LINEAR, TL_FULL, 2>;
}

bool small_strain_packed_launch(int packed, int law, int tl, int grid, int dyn_lds, hipStream_t st, const LawParams& prm, int64_t cnt,
                                const double* grad, const double* s0, double* s1, int64_t ld, double* flux, double* ct, BlockStats* bs,
                                uint32_t* stamps, uint32_t stamp, unsigned long long* pack_mask, double* pack_buf) {
#define DXM_LAUNCH_PACKED(LAW, TL, P)                                                                                       \
  hipLaunchKernelGGL((small_strain_packed_kernel<LAW, TL, P>), dim3(grid), dim3(BLOCK), dyn_lds, st, prm, cnt, grad, s0, s1, ld, \
                     flux, ct, bs, stamps, stamp, pack_mask, pack_buf)
#define DXM_LAUNCH_PACKED_TL(LAW, P) do { if (tl == TL_SYM) DXM_LAUNCH_PACKED(LAW, TL_SYM, P); else if (tl == TL_FULL) DXM_LAUNCH_PACKED(LAW, TL_FULL, P); \
                                          else if (tl == TL_PACK4) DXM_LAUNCH_PACKED(LAW, TL_PACK4, P); else DXM_LAUNCH_PACKED(LAW, TL_COEF, P); } while (0)
  if (packed != 1 && packed != 2) return false;
  if (law == LAW_J2_LINEAR) { if (packed == 1) DXM_LAUNCH_PACKED_TL(LAW_J2_LINEAR, 1); else DXM_LAUNCH_PACKED_TL(LAW_J2_LINEAR, 2); }
  else if (law == LAW_J2_VOCE) { if (packed == 1) DXM_LAUNCH_PACKED_TL(LAW_J2_VOCE, 1); else DXM_LAUNCH_PACKED_TL(LAW_J2_VOCE, 2); }
  else return false;
#undef DXM_LAUNCH_PACKED_TL
#undef DXM_LAUNCH_PACKED
  return true;
}

}  // namespace dxm
