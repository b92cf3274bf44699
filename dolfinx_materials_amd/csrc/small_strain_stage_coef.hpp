// The nine staged numbers (c1, c2, c3, n[6]) of this lane's point: NOT a header of its own.  Included where step 5 of the update
// kernels and expand_pack4_kernel form them from s[6], c1, c2, c3, wn (coef: the tile's coefficient region in LDS).  n = dev(sigma) wn
// with every operation individually rounded: the host rebuilds it with the same three lines (host_side.hpp).
{
  double* cf = coef + lane * 9;
  cf[0] = c1; cf[1] = c2; cf[2] = c3;
  const double third = opaque((s[0] + s[1] + s[2]) * SS_THIRD);
  cf[3] = (s[0] - third) * wn; cf[4] = (s[1] - third) * wn; cf[5] = (s[2] - third) * wn;
  cf[6] = s[3] * wn; cf[7] = s[4] * wn; cf[8] = s[5] * wn;
}
