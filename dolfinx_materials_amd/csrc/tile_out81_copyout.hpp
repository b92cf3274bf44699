// Copy-out of one round of the 81-entry tangent: NOT a header of its own.  Included at the end of a tangent round of fefp.hpp and
// hyperelastic.hip, after the column lanes have written the round's F2_PPR x 81 doubles to the out-tile and a wave_lds_sync(); the
// kernel syncs again after it.  The round leaves as contiguous 1 KiB wave stores, 16 B per lane, non-temporal: straight-line for the
// round shapes of a full tile, element-wise bounds for a ragged one.
// Reads: npts, p0, cnt, ct, base, outt, lane; F2_PPR, F2_NIT (fefp.hpp); OUT81_WHOLE_KIB, a constexpr bool of the including kernel:
// whether the ragged branch tests "whole KiB valid" with a scalar compare before the per-lane bounds (FeFp: true; Ogden: false, and
// giving it the test changes 485 lines of its assembly: a measured change of its own).  Defines nothing.
{
  int nv = npts - p0;                                      // valid points of this round
  nv = nv < 0 ? 0 : (nv > cnt ? cnt : nv);
  const int nent = nv * 81;                                // wave-uniform
  double* gct = ct + (base + p0) * 81;                     // 16 B aligned: (base + p0) * 81 is even
  const double2_t* o2 = reinterpret_cast<const double2_t*>(outt);
  constexpr int NIT = F2_NIT;
  double2_t v[NIT];
#pragma unroll
  for (int it = 0; it < NIT; ++it) v[it] = o2[it * WAVE + lane];   // the last, partial KiB reads on into the records: inside the wave's region
  double2_t* g2p = reinterpret_cast<double2_t*>(gct) + lane;
  // the two shapes every full tile consists of: straight-line stores, no per-KiB bookkeeping
  constexpr int E_FULL = F2_PPR * 81, E_LAST = (WAVE % F2_PPR) * 81;
  if (nent == E_FULL) {
#pragma unroll
    for (int it = 0; it < E_FULL / (2 * WAVE); ++it) stream_store<0>(g2p + it * WAVE, v[it]);
    if constexpr (E_FULL % (2 * WAVE) != 0) {
      static_assert(E_FULL % 2 == 0, "whole 16 B elements");
      if (lane < (E_FULL % (2 * WAVE)) / 2) stream_store<0>(g2p + (E_FULL / (2 * WAVE)) * WAVE, v[E_FULL / (2 * WAVE)]);
    }
  } else if (E_LAST > 0 && nent == E_LAST) {
#pragma unroll
    for (int it = 0; it < E_LAST / (2 * WAVE); ++it) stream_store<0>(g2p + it * WAVE, v[it]);
    if constexpr (E_LAST % (2 * WAVE) != 0) {
      static_assert(E_LAST % 2 == 0, "whole 16 B elements");
      if (lane < (E_LAST % (2 * WAVE)) / 2) stream_store<0>(g2p + (E_LAST / (2 * WAVE)) * WAVE, v[E_LAST / (2 * WAVE)]);
    }
  } else {   // ragged tile: element-wise bounds
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int e0 = (it * WAVE + lane) * 2;
      if (OUT81_WHOLE_KIB && (it + 1) * 2 * WAVE <= nent) {   // scalar branch: whole KiB valid
        stream_store<0>(reinterpret_cast<double2_t*>(gct + e0), v[it]);
      } else if (e0 + 1 < nent) {
        stream_store<0>(reinterpret_cast<double2_t*>(gct + e0), v[it]);
      } else if (e0 < nent) {
        stream_store<0>(gct + e0, v[it].x);
      }
    }
  }
}
