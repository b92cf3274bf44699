// Rows of nine, LDS -> my point's F, row-major: NOT a header of its own.  Included after tile_rows9_load.hpp and a wave_lds_sync().
// The staged 9-vector is in the order [11, 22, 33, 12, 21, 13, 31, 23, 32] (TI / TJ); tile_rows9_put.hpp is the inverse.
// Reads: stage, lane.  Writes: F[9] (declared by the kernel).
{
  const double* f = stage + lane * 9;
  F[0] = f[0]; F[4] = f[1]; F[8] = f[2]; F[1] = f[3]; F[3] = f[4];
  F[2] = f[5]; F[6] = f[6]; F[5] = f[7]; F[7] = f[8];
}
