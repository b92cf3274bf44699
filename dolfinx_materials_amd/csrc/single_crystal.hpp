// Host entry points of the FCC single-crystal viscoplasticity kernels (single_crystal.hip).  A translation unit of its own, like
// orthotropic.hip: compiled into the device module of dxmat.hip, new kernels change the code generated for the existing ones
// (ramberg_osgood.hpp).  A custom-hardening build compiles dxmat.hip alone and never serves this law.
#pragma once
#include <hip/hip_runtime.h>

#include "dxm_common.hpp"
#include "orthotropic.hpp"   // OrthoStiffness in the twelve free doubles of LawParams, Frame9, OR_FRAME_*

namespace dxm {

constexpr int SC_NSYS = 12;   // {111}<01-1>
// SoA state slots: every field is user-visible (DESIGN.md section "Single-crystal viscoplasticity")
constexpr int SC_SLOT_EEL = 0, SC_SLOT_G = 6, SC_SLOT_P = 18, SC_SLOT_A = 30, SC_NSLOTS = 42;

// interaction classes, in the order of the six coefficients [self, coplanar, Hirth, collinear, glissile, Lomer]
constexpr int SC_SELF = 0, SC_COPLANAR = 1, SC_HIRTH = 2, SC_COLLINEAR = 3, SC_GLISSILE = 4, SC_LOMER = 5;

// The geometry of the twelve systems, decided once at compile time from integer vectors: plane-major over the planes
// (1,1,1), (-1,1,1), (1,-1,1), (1,1,-1), within a plane the directions (0,1,-1), (1,0,-1), (1,-1,0), (0,1,1), (1,0,1), (1,1,0) that
// lie in it.  mu_i = Mandel(sym(s_i x n_i)) with |n| = sqrt3, |s| = sqrt2; rows 12..15 are zero (the idle lanes of a 16-lane row).
struct ScTables {
  int n[SC_NSYS][3], s[SC_NSYS][3], plane[SC_NSYS];
  double mu[16][6];
  int cls[16][SC_NSYS];
};
constexpr ScTables sc_make_tables() {
  ScTables t{};
  const int P[4][3] = {{1, 1, 1}, {-1, 1, 1}, {1, -1, 1}, {1, 1, -1}};
  const int D[6][3] = {{0, 1, -1}, {1, 0, -1}, {1, -1, 0}, {0, 1, 1}, {1, 0, 1}, {1, 1, 0}};
  int k = 0;
  for (int p = 0; p < 4; ++p)
    for (int d = 0; d < 6; ++d)
      if (P[p][0] * D[d][0] + P[p][1] * D[d][1] + P[p][2] * D[d][2] == 0 && k < SC_NSYS) {
        for (int c = 0; c < 3; ++c) { t.n[k][c] = P[p][c]; t.s[k][c] = D[d][c]; }
        t.plane[k] = p;
        ++k;
      }
  const double INV_SQRT6 = 0.40824829046386301637, INV_2SQRT3 = 0.28867513459481288225;
  for (int i = 0; i < SC_NSYS; ++i)
    for (int I = 0; I < 6; ++I) {
      const int a = SI[I], b = SJ[I];
      t.mu[i][I] = I < 3 ? INV_SQRT6 * (t.s[i][a] * t.n[i][a]) : INV_2SQRT3 * (t.s[i][a] * t.n[i][b] + t.s[i][b] * t.n[i][a]);
    }
  for (int i = 0; i < SC_NSYS; ++i)
    for (int j = 0; j < SC_NSYS; ++j) {
      const int* si = t.s[i]; const int* sj = t.s[j]; const int* ni = t.n[i]; const int* nj = t.n[j];
      const int cx = si[1] * sj[2] - si[2] * sj[1], cy = si[2] * sj[0] - si[0] * sj[2], cz = si[0] * sj[1] - si[1] * sj[0];
      const int c[3] = {ni[1] * nj[2] - ni[2] * nj[1], ni[2] * nj[0] - ni[0] * nj[2], ni[0] * nj[1] - ni[1] * nj[0]};   // n_i x n_j
      auto parallel = [&](const int* v) {
        return v[1] * c[2] - v[2] * c[1] == 0 && v[2] * c[0] - v[0] * c[2] == 0 && v[0] * c[1] - v[1] * c[0] == 0;
      };
      int k2 = SC_LOMER;
      if (i == j) k2 = SC_SELF;
      else if (t.plane[i] == t.plane[j]) k2 = SC_COPLANAR;
      else if (cx == 0 && cy == 0 && cz == 0) k2 = SC_COLLINEAR;
      else if (si[0] * sj[0] + si[1] * sj[1] + si[2] * sj[2] == 0) k2 = SC_HIRTH;
      else if (parallel(si) || parallel(sj)) k2 = SC_GLISSILE;
      t.cls[i][j] = k2;
    }
  return t;
}
constexpr ScTables SC = sc_make_tables();

constexpr bool sc_classes_ok() {
  const int want[6] = {1, 2, 2, 1, 4, 2};   // self, coplanar, Hirth, collinear, glissile, Lomer
  for (int i = 0; i < SC_NSYS; ++i) {
    int cnt[6] = {0, 0, 0, 0, 0, 0};
    for (int j = 0; j < SC_NSYS; ++j) {
      ++cnt[SC.cls[i][j]];
      if (SC.cls[i][j] != SC.cls[j][i]) return false;
    }
    for (int k = 0; k < 6; ++k)
      if (cnt[k] != want[k]) return false;
  }
  return true;
}
static_assert(sc_classes_ok(), "each system meets 1 self, 2 coplanar, 2 Hirth, 1 collinear, 4 glissile and 2 Lomer partners, symmetrically");

// The record of the law's own, a kernel argument next to LawParams (whose twelve free doubles carry the stiffness and whose layout
// is part of every other kernel's argument list): formed on the host by the launcher from the handle's 22 parameters and the dt of
// the call
struct ScParams {
  double n, K, tau0, b, d, C;
  double qh[6];     // Q x the six interaction coefficients, by class
  double guard;     // 1.1 K: an iterate with any f_i above it is rejected
  double floor_f;   // 1e-12 D_00: the floor of f in dv = n (f/K)^n / max(f, floor)
  double dt;
};

// Launch shape: the Hosford grid, unmeasured for this kernel (DESIGN.md section "Single-crystal viscoplasticity")
constexpr int SC_BLOCKS_PER_CU = 64;

// static LDS of one workgroup: per wave the 64 x 36 staged tangent entries (their head doubles as the strain / stress staging of
// tile_rows6_*.hpp) and the 4 x 14 hand-over words of a Newton round, plus the block-stats words
constexpr int SC_ROUND = 14;   // per round slot: the twelve slip increments, status, iterations
constexpr int SC_LDS_PER_WAVE = WAVE * 36 + 4 * SC_ROUND;
constexpr int SC_SYS = 30;     // per slip system, shared by the waves: B_i (6), row i of M (12), row i of Q h (12)
// Workgroups of two waves: the kernel takes 280 / 304 / 304 registers per lane (256 VGPRs and 24 / 48 / 48 AGPRs that hold copies of
// VGPRs: none / uniform / field frame), which one wave per SIMD has and two have not: 2 workgroups x 2 waves per CU (the
// first thing to measure, and an open item)
constexpr int SC_BLOCK = 128, SC_WAVES = SC_BLOCK / WAVE;
constexpr int SC_LDS_BYTES = SC_WAVES * SC_LDS_PER_WAVE * 8 + 16 * SC_SYS * 8 + 36 * 8 + 4 * SC_WAVES * 8;

// the kernel without a frame (what dxm_create asks the resources of)
__attribute__((visibility("hidden"))) const void* single_crystal_kernel_fn();

// one launch of single_crystal_kernel<frame>; frames as in orthotropic_launch
__attribute__((visibility("hidden"))) void single_crystal_launch(int frame, int grid, hipStream_t st, const LawParams& prm, const ScParams& sp,
                                                                 int64_t cnt, const double* grad, const Frame9& uniform, const double* frames,
                                                                 int64_t ldf, const double* s0, double* s1, int64_t ld, double* flux, double* ct,
                                                                 BlockStats* bs);

// `width` consecutive SoA slots from `first` on -> (n, width) row-major rows, for any law whose visible state is wider than the slot
// map of dxmat.hip's pack kernel (PackMap: 16) and sits in consecutive slots.  Nothing of it is specific to this law; it lives in
// this unit because a kernel added to dxmat.hip, or a wider PackMap, changes that unit's device assembly, which is pinned
__attribute__((visibility("hidden"))) void pack_consecutive_slots(const double* soa, int64_t ld, int64_t n, int first, int width, double* aos,
                                                                     hipStream_t st);

}  // namespace dxm
