// Rows of five, global -> LDS: NOT a header of its own.  Included inside the tile loop of the finite-strain kernels whose gradient is
// an (N, 5) array of the plane deformation gradient [F00, F11, F22, F01, F10] (ogden_plane.hip).  A tile's 64 rows are 2560
// contiguous bytes whose base is 16 B aligned (a multiple of 2560; a row on its own is only 8 B aligned): a full tile moves its
// 64 x 5 doubles = 160 double2 as 16 B per lane; a ragged last tile as 8 B accesses bounded per element, with the identity for the
// missing points.  Followed by a wave_lds_sync() and plane5_rows5_take.hpp.
// The five plane5_*.hpp files are written in the shape of the tile_rows9_* / tile_rows3_* sets, for the later 5-wide forms (logarithmic
// strain, FeFp, the finite-strain single crystal) to include; the prefix tile_ is kept for text that at least two kernels include
// (tests/test_tile_fragments.py), which these become with their second user.
// Reads: Fin, base, npts, lane, stage, stage2.  Defines nothing.
if (npts == WAVE) {
  const double2_t* gsrc = reinterpret_cast<const double2_t*>(Fin + base * 5);
  double2_t v[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int idx = k * WAVE + lane;
    v[k] = (idx < 160) ? stream_load<2>(gsrc + idx) : double2_t{0.0, 0.0};
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int idx = k * WAVE + lane;
    if (idx < 160) stage2[idx] = v[k];
  }
} else {
  const double* gsrc = Fin + base * 5;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const int idx = k * WAVE + lane;
    const int c = idx % 5;
    stage[idx] = (idx < npts * 5) ? gsrc[idx] : (c < 3 ? 1.0 : 0.0);
  }
}
