// Rows of three, global -> LDS: NOT a header of its own.  Included inside the tile loop of the kernels whose gradient has three
// entries per point (plane_stress.hip, plane_stress_j2.hip, plane_stress_hosford.hip, heat_transfer.hip).  The wave reads the tile's
// 64 x 3 doubles as 96 accesses of 16 B over two passes, zero beyond the tile's last point, into its private staging region; an odd
// number of points ends on one 8 B read.  The kernel issues its own state / temperature / parameter loads after this text and before
// the first wave_lds_sync().
// Reads: grad, base, npts, lane, stage2.  Defines nothing.
{
  const double* g0 = grad + base * 3;
  const int nd = npts * 3;
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const int q = lane + pass * WAVE;
    if (q < WAVE * 3 / 2) {
      double2_t v = {0.0, 0.0};
      if (2 * q + 1 < nd) v = stream_load<2>(reinterpret_cast<const double2_t*>(g0) + q);
      else if (2 * q < nd) v.x = stream_load<2>(g0 + 2 * q);
      stage2[q] = v;
    }
  }
}
