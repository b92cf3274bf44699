// Rows of five, my point's flux in the order of the 5-vector -> LDS: NOT a header of its own.  The inverse of plane5_rows5_take.hpp;
// followed by a wave_lds_sync() and plane5_rows5_store.hpp.
// Reads: P5[5], stage, lane.  Defines nothing.
{
  double* f = stage + lane * 5;
#pragma unroll
  for (int t = 0; t < 5; ++t) f[t] = P5[t];
}
