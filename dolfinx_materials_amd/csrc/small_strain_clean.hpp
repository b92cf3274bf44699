// Host entry points of the J2 update kernels that keep unchanged tiles' state in place (small_strain_clean.hip).  A translation unit
// of their own for the reason ramberg_osgood.hpp gives: the device modules of the other units must compile to the instruction
// streams they had before these kernels existed (tools/check_device_asm.py --parent REV).
//
// The invariant they keep: one 32-bit stamp per 64-point tile of the handle, and
//     stamps[t] == the handle's current stamp   =>   the bytes of tile t are the same in both state buffers, slot for slot.
// A tile without a yielding point stores into s1 exactly what it read from s0; where its stamp is current those seven stores are
// skipped.  Every other writer of either buffer makes all stamps stale by moving the handle's stamp on (dxmat.hip: bump_clean_stamp).
#pragma once
#include <hip/hip_runtime.h>

#include "dxm_common.hpp"

namespace dxm {

// the full-layout linear-hardening kernel (named for tools and tests; the grid is sized as for small_strain_kernel)
__attribute__((visibility("hidden"))) const void* small_strain_clean_kernel_ptr();

// one launch of small_strain_clean_kernel<law, tl> (law: LAW_J2_LINEAR or LAW_J2_VOCE; tl: TL_*) over cnt points whose first is the
// first point of tile stamps[0]; dyn_lds: the J2 kernels' pad (four workgroups per CU).  False: no such instantiation in this build
// (Voce may be left on the plain kernel), nothing was launched.
__attribute__((visibility("hidden"))) bool small_strain_clean_launch(int law, int tl, int grid, int dyn_lds, hipStream_t st, const LawParams& prm,
                                                                     int64_t cnt, const double* grad, const double* s0, double* s1, int64_t ld,
                                                                     double* flux, double* ct, BlockStats* bs, uint32_t* stamps, uint32_t stamp);

// ---- the packed copy of s0 (option pack_old_state; DESIGN.md section 2, host_side.hpp: PackEpoch) -----------------------------
// s0 does not change between the updates of one load step, and a point that has never yielded holds seven zeros in it.  Per 64-point
// tile t of the handle:  pack_mask[t]  bit l set  <=>  one of point l's seven slots in s0 is not bit-zero (-0.0 and NaN count), and
// pack_buf + t * 7 * 64 holds the k = popcount(mask) such points densely: slot c of the r-th of them (r = set bits below l) at
// c k + r, so that only the first 56 k bytes of the tile's pitch are ever touched and no offset table is needed.
// small_strain_packed_kernel<law, tl, 1> (small_strain_packed.hip) is the clean kernel that also writes both (build); <law, tl, 2> reads them instead of s0 (use):
// a lane whose bit is clear takes zeros, a tile with k = 0 loads no state.  The store side and the stamps are the clean kernel's.
// Full-range launches only: stamps, pack_mask and pack_buf are the handle's arrays, tile 0 first.  False: nothing was launched.
__attribute__((visibility("hidden"))) const void* small_strain_packed_kernel_ptr(int packed);
__attribute__((visibility("hidden"))) bool small_strain_packed_launch(int packed, int law, int tl, int grid, int dyn_lds, hipStream_t st,
                                                                      const LawParams& prm, int64_t cnt, const double* grad, const double* s0,
                                                                      double* s1, int64_t ld, double* flux, double* ct, BlockStats* bs,
                                                                      uint32_t* stamps, uint32_t stamp, unsigned long long* pack_mask,
                                                                      double* pack_buf);

}  // namespace dxm
