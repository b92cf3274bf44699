// Tangent write-out from the staged upper triangles: NOT a header of its own.  Included inside the tile loop of the kernels whose
// tangent is a general symmetric 6x6 (hosford.hip, orthotropic.hip), after every lane has written the 21 upper-triangle entries of
// its point to tri[lane * TRI21 + TRI21_AT(i, k)] and a wave_lds_sync().  The wave writes the output stream in order, 16 B per lane,
// whole 1 KiB runs, non-temporal; entry (i, j) and (j, i) are the same staged number.
// Reads: SYM (compile-time: the tangent layout), ct, base, npts, lane, tri; TRI21, TRI21_AT (dxm_common.hpp).  Defines nothing.
if constexpr (SYM) {
  // the staged region IS the (npts, 21) output: 672 pairs per full tile
  double* gct = ct + base * TRI21;
  const double2_t* t2 = reinterpret_cast<const double2_t*>(tri);
  const int lim = npts * TRI21;
#pragma unroll
  for (int it = 0; it < 11; ++it) {
    const int k = it * WAVE + lane;
    const int e0 = 2 * k;
    if (e0 + 1 < lim) stream_store<0>(reinterpret_cast<double2_t*>(gct + e0), t2[k]);
    else if (e0 < lim) stream_store<0>(gct + e0, tri[e0]);
  }
} else {
  // full 6x6, row-major: 18 pairs per point, 18 x 1 KiB per full tile; pair (i, j..j+1) of point q reads the staged (min, max) entries
  double2_t* gct = reinterpret_cast<double2_t*>(ct + base * 36);
  const int lim = npts * 18;
#pragma unroll 2
  for (int it = 0; it < 18; ++it) {
    const int k = it * WAVE + lane;
    const int q = k / 18;
    const int r = k - q * 18;
    const int i = r / 3;
    const int j = (r - i * 3) * 2;
    const int lo0 = i < j ? i : j, hi0 = i < j ? j : i;
    const int lo1 = i < j + 1 ? i : j + 1, hi1 = i < j + 1 ? j + 1 : i;
    const double* rq = tri + q * TRI21;
    const double2_t v = {rq[TRI21_AT(lo0, hi0)], rq[TRI21_AT(lo1, hi1)]};
    if (k < lim) stream_store<0>(gct + k, v);
  }
}
