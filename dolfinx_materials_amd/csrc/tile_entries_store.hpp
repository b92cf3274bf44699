// The tangent in output order: NOT a header of its own.  Included inside the tile loop of plane_stress.hip, plane_stress_j2.hip,
// plane_stress_hosford.hip (W = 9) and heat_transfer.hip (W = 12 / 13), after tile_rows3_store.hpp.  Entry e of the tile belongs to
// point e / W, column e % W; the kernel says what it is in a callable `double entry(int e)` defined just before this text.  The
// wave writes the tile's 64 x W entries as pairs, 16 B-per-lane non-temporal stores, one of 8 B where an odd number of entries ends,
// nothing beyond the tile's last point.
// Reads: ct, base, npts, lane, W (constexpr int), entry.  Defines nothing.
{
  double* c0 = ct + base * W;
  const int nd = npts * W;
  constexpr int NQ = WAVE * W / 2;
#pragma unroll
  for (int pass = 0; pass < (NQ + WAVE - 1) / WAVE; ++pass) {
    const int q = lane + pass * WAVE;
    if (q < NQ && 2 * q < nd) {
      const double2_t v = {entry(2 * q), entry(2 * q + 1)};
      if (2 * q + 1 < nd) stream_store<0>(reinterpret_cast<double2_t*>(c0) + q, v);
      else stream_store<0>(c0 + 2 * q, v.x);
    }
  }
}
