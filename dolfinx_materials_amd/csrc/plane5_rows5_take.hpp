// Rows of five, LDS -> my point's row: NOT a header of its own.  Included after plane5_rows5_load.hpp and a wave_lds_sync().  The row
// stays in the order of the 5-vector [00, 11, 22, 01, 10] (utils.py:168-172); plane5_rows5_put.hpp is the inverse.  The rows are 10
// dwords apart: the 8 B reads of 32 lanes fall on 32 distinct bank pairs (10 l mod 64).
// Reads: stage, lane.  Writes: F5[5] (declared by the kernel).
{
  const double* f = stage + lane * 5;
#pragma unroll
  for (int t = 0; t < 5; ++t) F5[t] = f[t];
}
