// Rows of six, LDS -> global: NOT a header of its own.  Included after every lane has staged its point's stress as
// stage2[lane * 3 + 0..2] and a wave_lds_sync(): the wave writes the tile's 64 x 6 doubles as 3 x 1 KiB, 16 B per lane, predicated
// for a ragged tile.
// Reads: sig, base, npts, lane, stage2.  Defines nothing.
{
  double2_t* gdst = reinterpret_cast<double2_t*>(sig + base * 6);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int idx = k * WAVE + lane;
    if (idx < npts * 3) stream_store<0>(gdst + idx, stage2[idx]);
  }
}
