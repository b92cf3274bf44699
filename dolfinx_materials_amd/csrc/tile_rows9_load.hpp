// Rows of nine, global -> LDS: NOT a header of its own.  Included inside the tile loop of the finite-strain kernels whose gradient
// is an (N, 9) array of F (fefp.hpp with GRAD == 0, hyperelastic.hip).  A full tile moves its 64 x 9 doubles = 288 double2 as 16 B
// per lane; a ragged last tile as 8 B accesses, with the identity for the missing points.  The kernel issues its own state loads
// after this text and before the wave_lds_sync() that precedes tile_rows9_take.hpp.
// Reads: Fin, base, npts, lane, stage, stage2.  Defines nothing.
if (npts == WAVE) {
  const double2_t* gsrc = reinterpret_cast<const double2_t*>(Fin + base * 9);
  double2_t v[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const int idx = k * WAVE + lane;
    v[k] = (idx < 288) ? stream_load<2>(gsrc + idx) : double2_t{0.0, 0.0};
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const int idx = k * WAVE + lane;
    if (idx < 288) stage2[idx] = v[k];
  }
} else {
  const double* gsrc = Fin + base * 9;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const int idx = k * WAVE + lane;
    const int c = idx % 9;
    stage[idx] = (idx < npts * 9) ? gsrc[idx] : (c < 3 ? 1.0 : 0.0);
  }
}
