// Host entry points of the plane-strain logarithmic-strain J2 kernel (log_strain_plane.hip): law 19 (log_strain.hip) on the 5-wide
// deformation gradient [F00, F11, F22, F01, F10] of a 2x2 tensor with its out-of-plane stretch (utils.py:168-172).  A translation
// unit of its own, like the other laws added after the first five (ramberg_osgood.hpp says why); this header declares host functions
// and constants only, so dxmat.hip's device code does not see the law.  A custom-hardening build compiles dxmat.hip alone and never
// serves this law.  The parameter record is law 19's: LawParams as dxmat.hip::build_log_strain fills it.
#pragma once
#include <hip/hip_runtime.h>

#include "dxm_common.hpp"

namespace dxm {

constexpr int LSP_DIM = 5;   // F and PK1: [00, 11, 22, 01, 10]
constexpr int LSP_CT = 25;   // the 5x5 dP/dF, row-major: 200 B per point, a tile's 64 are exactly 100 lines of 128 B
constexpr int LSP_SYM = 4;   // the symmetric tensors of the law as MFront's 2-D vector [xx, yy, zz, sqrt(2) xy]

// SoA state slots, law 19's fields at their plane-strain width, in the arrangement of hosford_plane.hpp: ElasticStrain 0..3 (written
// by every update, never read), EquivalentPlasticStrain 4, and the hidden field the update is driven by, the logarithmic plastic
// strain 5..8 (log_strain.hpp: the kernel receives the TOTAL F, so its trial elastic strain is E - Ep_n)
constexpr int LSP_SLOT_EEL = 0, LSP_SLOT_P = 4, LSP_SLOT_EP = 5, LSP_NSLOTS = 9;

// The tangent leaves in ROUNDS OF 32 POINTS through the wave's out-tile, as ogden_plane.hpp argues for the same 25 entries: 6400 B per
// wave, 25 600 B per workgroup, 6 workgroups per CU by LDS.  The kernel needs 167 VGPRs (no scratch, no spilled VGPR, no occupancy
// argument), which allow 3 waves per SIMD = 3 workgroups per CU (law 19: 2), so the registers decide.  A whole-tile out-tile (51 200 B
// per workgroup) would still hold 3 workgroups, with 153 600 of the CU's 163 840 B; it saves one round's two syncs per tile and is
// unmeasured, as are rounds of 16.  The lanes of a round form the entries under a branch, so the wave spends the ~100 multiply-adds of
// that step twice; keeping every lane's 25 entries in registers across the rounds instead would cost 50 VGPRs and the third wave.
// The 64 x 5 staging of F and of PK1 (320 doubles) aliases the start of the out-tile (800); the workgroup reduction of the stats
// borrows the first words of every wave's region after the tile loop.
constexpr int LSP_PPR = 32;                                             // points per tangent round
constexpr int LSP_LDS_PER_WAVE = LSP_PPR * LSP_CT;                      // 800 doubles
constexpr int LSP_LDS_BYTES = WAVES_PER_BLOCK * LSP_LDS_PER_WAVE * 8;   // 25 600 B per workgroup
static_assert(LSP_LDS_BYTES == 25600 && WAVE * LSP_DIM <= LSP_LDS_PER_WAVE && WAVE % LSP_PPR == 0 && LSP_PPR % 2 == 0,
              "the LDS that DESIGN.md states for the plane-strain logarithmic-strain kernel; the staging fits; whole rounds; 16 B aligned round bases");

// Launch shape: law 19's and plane-strain Ogden's 256 workgroups per CU (one workgroup per 256 points up to that), whose I/O skeleton
// this kernel shares.  What a sweep over 32 / 64 / 128 / 256 at 1e7 points says for this law: profiles/r28_log_strain_plane.md.
constexpr int LSP_BLOCKS_PER_CU = 256;

__attribute__((visibility("hidden"))) const void* log_strain_plane_kernel_fn();

// one launch over cnt points: F (cnt, 5) -> PK1 (cnt, 5), dP/dF (cnt, 25); s0 / s1: slot 0 of the two state buffers at the first
// point of the launch (LSP_NSLOTS slots of leading dimension ld)
__attribute__((visibility("hidden"))) void log_strain_plane_launch(int grid, hipStream_t st, const LawParams& prm, int64_t cnt, const double* F,
                                                                   const double* s0, double* s1, int64_t ld, double* P, double* ct,
                                                                   BlockStats* bs);

}  // namespace dxm
