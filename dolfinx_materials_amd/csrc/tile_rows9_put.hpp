// Rows of nine, my point's row-major PK1 -> LDS in the order of the 9-vector: NOT a header of its own.  The inverse of
// tile_rows9_take.hpp; followed by a wave_lds_sync() and tile_rows9_store.hpp.
// Reads: P[9], stage, lane.  Defines nothing.
{
  double* f = stage + lane * 9;
  f[0] = P[0]; f[1] = P[4]; f[2] = P[8]; f[3] = P[1]; f[4] = P[3];
  f[5] = P[2]; f[6] = P[6]; f[7] = P[5]; f[8] = P[7];
}
