// Rows of five, LDS -> global: NOT a header of its own.  Included after plane5_rows5_put.hpp and a wave_lds_sync(): 16 B per lane for
// a full tile (160 stores), predicated 8 B accesses for a ragged one, which touch nothing past 5 npts doubles.
// Reads: Pout, base, npts, lane, stage, stage2.  Defines nothing.
if (npts == WAVE) {
  double2_t* gdst = reinterpret_cast<double2_t*>(Pout + base * 5);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int idx = k * WAVE + lane;
    if (idx < 160) stream_store<0>(gdst + idx, stage2[idx]);
  }
} else {
  double* gdst = Pout + base * 5;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const int idx = k * WAVE + lane;
    if (idx < npts * 5) gdst[idx] = stage[idx];
  }
}
