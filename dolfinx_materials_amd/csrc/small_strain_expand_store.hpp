// The full-tangent store loop of the two rebuild kernels: NOT a header of its own.  small_strain.hpp includes this text inside the tile
// loops of expand_tangent_kernel and expand_pack4_kernel, where coef (the tile's 64 x 9 staged coefficients in LDS), npts, lane, base
// and ct are defined.  Step 7 of the update kernel (TL_FULL, groups of three) with predicated stores for a ragged tile.
    double2_t* gct = reinterpret_cast<double2_t*>(ct + base * 36);
    const int lim = npts * 18;
#pragma unroll 1
    for (int g = 0; g < 6; ++g) {
      double2_t v[3];
#pragma unroll
      for (int u = 0; u < 3; ++u) {
        const int k = (g * 3 + u) * WAVE + lane;
        const int q = k / 18;
        const int r = k - q * 18;
        const int i = r / 3;
        v[u] = tangent_pair(coef + q * 9, i, (r - i * 3) * 2);
      }
#pragma unroll
      for (int u = 0; u < 3; ++u) {
        const int k = (g * 3 + u) * WAVE + lane;
        if (k < lim) stream_store<0>(gct + k, v[u]);
      }
    }
