// Host entry points of the plane-strain Ogden kernel (ogden_plane.hip): law 7 (hyperelastic.hip) on the 5-wide deformation gradient
// [F00, F11, F22, F01, F10] of a 2x2 tensor with its out-of-plane stretch (utils.py:168-172).  A translation unit of its own, like
// the other laws added after the first five (ramberg_osgood.hpp says why); this header declares host functions and constants only, so
// dxmat.hip's device code does not see the law.  A custom-hardening build compiles dxmat.hip alone and never serves this law.
// The parameter record is law 7's: LawParams as dxmat.hip::build_ogden fills it (the OG_* slots of hyperelastic.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include "dxm_common.hpp"

namespace dxm {

constexpr int OGP_DIM = 5;      // F and PK1: [00, 11, 22, 01, 10]
constexpr int OGP_CT = 25;      // the 5x5 dP/dF, row-major: 200 B per point, a tile's 64 are exactly 100 lines of 128 B
constexpr int OGP_NSLOTS = 4;   // PK2Stress (the isochoric part only) as MFront's 2-D symmetric tensor [xx, yy, zz, sqrt(2) xy]

// The out-tile holds ROUNDS OF 32 POINTS, as fefp.hpp stages its 81-entry tangent in rounds: in round rd the lanes 32 rd .. 32 rd + 31
// form their 25 entries and write them to the out-tile, then the whole wave copies the round's 6400 B (50 lines of 128 B) out.  The
// kernel needs 113 VGPRs, which allow 4 waves per SIMD; a whole-tile out-tile (12 800 B per wave, 51 200 B per workgroup) would hold the
// kernel at 3 workgroups per CU = 3 waves per SIMD by LDS.  With rounds of 32: 6400 B per wave, 25 600 B per workgroup, 6 workgroups
// per CU by LDS, so the registers decide: 4 waves per SIMD (ogden_kernel: 2).  Rounds of 16 (12 800 B per workgroup) give the same 4
// and twice the round overhead.  The lanes of a round form the entries under a branch, so the wave spends the ~100 multiply-adds of
// that step twice; keeping every lane's 25 entries in registers across the rounds instead would cost 50 VGPRs and the fourth wave.
// The 64 x 5 staging of F and of PK1 (320 doubles) aliases the start of the out-tile (800); the workgroup reduction of the stats
// borrows the first words of every wave's region once the tile loop is over.
constexpr int OGP_PPR = 32;                                             // points per tangent round
constexpr int OGP_LDS_PER_WAVE = OGP_PPR * OGP_CT;                      // 800 doubles
constexpr int OGP_LDS_BYTES = WAVES_PER_BLOCK * OGP_LDS_PER_WAVE * 8;   // 25 600 B per workgroup
static_assert(OGP_LDS_BYTES == 25600 && WAVE * OGP_DIM <= OGP_LDS_PER_WAVE && WAVE % OGP_PPR == 0 && OGP_PPR % 2 == 0,
              "the LDS that DESIGN.md states for the plane-strain Ogden kernel; the staging fits; whole rounds; 16 B aligned round bases");

// Launch shape.  The precedent is 32 workgroups per CU for the laws whose tiles all cost the same (the comment above the rows in
// dxmat.hip) unless a sweep says otherwise.  One sweep at 1e7 points (profiles/r26_ogden_plane.md: 32 / 64 / 128 / 256, one timing
// each) has the kernel at 0.5696 / 0.5435 / 0.5325 / 0.5245 ms: 256 is 8 % faster than 32 and is taken.  Other sizes: not measured.
constexpr int OGP_BLOCKS_PER_CU = 256;

__attribute__((visibility("hidden"))) const void* ogden_plane_kernel_fn();

// one launch over cnt points: F (cnt, 5) -> PK1 (cnt, 5), dP/dF (cnt, 25), s1 = PK2Stress (4 slots of leading dimension ld)
__attribute__((visibility("hidden"))) void ogden_plane_launch(int grid, hipStream_t st, const LawParams& prm, int64_t cnt, const double* F,
                                                              double* s1, int64_t ld, double* P, double* ct, BlockStats* bs);

}  // namespace dxm
