// Rows of six, LDS -> my point's six numbers: NOT a header of its own.  Included after tile_rows6_load.hpp and a wave_lds_sync(); the
// kernel syncs again before it reuses the staging region for the stress.
// Reads: stage2, lane.  Writes: e[6] (declared by the kernel).
{
  const double2_t a = stage2[lane * 3 + 0], b = stage2[lane * 3 + 1], c = stage2[lane * 3 + 2];
  e[0] = a.x; e[1] = a.y; e[2] = b.x; e[3] = b.y; e[4] = c.x; e[5] = c.y;
}
