// Rows of nine, LDS -> global: NOT a header of its own.  Included after tile_rows9_put.hpp and a wave_lds_sync(): 16 B per lane for
// a full tile, predicated 8 B accesses for a ragged one.
// Reads: Pout, base, npts, lane, stage, stage2.  Defines nothing.
if (npts == WAVE) {
  double2_t* gdst = reinterpret_cast<double2_t*>(Pout + base * 9);
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const int idx = k * WAVE + lane;
    if (idx < 288) stream_store<0>(gdst + idx, stage2[idx]);
  }
} else {
  double* gdst = Pout + base * 9;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const int idx = k * WAVE + lane;
    if (idx < npts * 9) gdst[idx] = stage[idx];
  }
}
