// Copy-out of one round of 25-entry tangent blocks: NOT a header of its own.  Included after the lanes of round rd (points p0 ..
// p0 + OGP_PPR of the tile) have written their point's 25 doubles to the out-tile (record of point slot s at outt + 25 s: 50 dwords
// apart, the 8 B writes of 32 lanes fall on 32 distinct bank pairs) and a wave_lds_sync(); the kernel syncs again after it.  A round's
// OGP_PPR x 25 doubles are whole lines of 128 B (32 points: 6400 B = 50 lines; a tile's 64: 100 lines) whose base is 16 B aligned:
// they leave in output order as 16 B per lane, non-temporal, every line written whole.  A ragged last tile is bounded per element and
// touches nothing past 25 npts doubles.
// Reads: npts, p0, ct, base, outt, lane; OGP_PPR (ogden_plane.hpp).  Defines nothing.
{
  static_assert((OGP_PPR * 25 * 8) % 128 == 0, "a round is whole 128 B lines");
  constexpr int NV = OGP_PPR * 25 / 2;                     // double2 per round
  constexpr int NIT = (NV + WAVE - 1) / WAVE;              // wave stores per round, the last one partial
  int nv = npts - p0;                                      // valid points of this round
  nv = nv < 0 ? 0 : (nv > OGP_PPR ? OGP_PPR : nv);
  const double2_t* o2 = reinterpret_cast<const double2_t*>(outt);
  double* gct = ct + (base + p0) * 25;                     // 16 B aligned: base + p0 is even
  if (nv == OGP_PPR) {
    double2_t* g2p = reinterpret_cast<double2_t*>(gct) + lane;
#pragma unroll
    for (int it = 0; it < NV / WAVE; ++it) stream_store<0>(g2p + it * WAVE, o2[it * WAVE + lane]);
    if constexpr (NV % WAVE != 0) {
      if (lane < NV % WAVE) stream_store<0>(g2p + (NV / WAVE) * WAVE, o2[(NV / WAVE) * WAVE + lane]);
    }
  } else {
    const int nent = nv * 25;                              // wave-uniform
#pragma unroll 1
    for (int it = 0; it < NIT; ++it) {
      const int i2 = it * WAVE + lane, e0 = i2 * 2;
      if (e0 + 1 < nent) stream_store<0>(reinterpret_cast<double2_t*>(gct + e0), o2[i2]);
      else if (e0 < nent) stream_store<0>(gct + e0, outt[e0]);
    }
  }
}
