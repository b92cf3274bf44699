// Rows of three, LDS -> global: NOT a header of its own.  Included inside the tile loop of plane_stress.hip, plane_stress_j2.hip,
// plane_stress_hosford.hip and heat_transfer.hip, after the wave_lds_sync() that follows the lanes' three stage[lane * 3 + k] writes.
// The walk of tile_rows3_load.hpp outwards: 96 non-temporal stores of 16 B, one of 8 B where an odd number of points ends, nothing
// beyond the tile's last point.
// Reads: flux, base, npts, lane, stage2.  Defines nothing.
{
  double* f0 = flux + base * 3;
  const int nd = npts * 3;
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const int q = lane + pass * WAVE;
    if (q < WAVE * 3 / 2) {
      const double2_t v = stage2[q];
      if (2 * q + 1 < nd) stream_store<0>(reinterpret_cast<double2_t*>(f0) + q, v);
      else if (2 * q < nd) stream_store<0>(f0 + 2 * q, v.x);
    }
  }
}
