// Tangent write-out of a full, non-symmetric 6x6 per point: NOT a header of its own.  Included inside the tile loop of the kernels
// whose small-strain tangent has no symmetric form (single_crystal.hip), after every lane has written the 36 row-major entries of
// its point to t36[lane * 36 + 6 * i + k] and a wave_lds_sync().  The staged region IS the (npts, 36) output: the wave writes it in
// order, 16 B per lane, 18 whole 1 KiB runs per full tile, non-temporal, predicated for a ragged tile.
// (Not named tile_*.hpp: that prefix is kept for text that two or more kernels include; this one has a single user so far.)
// Reads: ct, base, npts, lane, t36.  Defines nothing.
{
  double2_t* gct = reinterpret_cast<double2_t*>(ct + base * 36);
  const double2_t* t2 = reinterpret_cast<const double2_t*>(t36);
  const int lim = npts * 18;
#pragma unroll
  for (int it = 0; it < 18; ++it) {
    const int k = it * WAVE + lane;
    if (k < lim) stream_store<0>(gct + k, t2[k]);
  }
}
