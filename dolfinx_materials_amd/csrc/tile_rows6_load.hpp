// Rows of six, global -> LDS: NOT a header of its own.  Included inside the tile loop of the kernels whose gradient is a strain array
// (small_strain_body.hpp, hosford.hip, orthotropic.hip).  The wave reads the tile's 64 x 6 doubles as 3 x 1 KiB, 16 B per lane, zero
// beyond the tile's last point, into its private staging region.  The kernel issues its own state / parameter / frame loads after
// this text and before the wave_lds_sync() that precedes tile_rows6_take.hpp.
// Reads: eps, base, npts, lane, stage2.  Defines nothing.
{
  const double2_t* gsrc = reinterpret_cast<const double2_t*>(eps + base * 6);
  double2_t v[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int idx = k * WAVE + lane;
    v[k] = (idx < npts * 3) ? stream_load<2>(gsrc + idx) : double2_t{0.0, 0.0};
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) stage2[k * WAVE + lane] = v[k];
}
