// The role of a lane in the 81-entry tangent epilogue: NOT a header of its own.  Included at the top of the tile loop of fefp.hpp
// and hyperelastic.hip, after the per-tile opaque re-read of the lane index.  Lane = (point slot ps, tangent column cc = (kk, LL));
// seven point slots x nine columns, lane 63 idles.
// Reads: lane.  Defines: ps, cc, kk, LL, mk0, mk1, mk2 (the (i == kk) masks as doubles).
const int ps = lane / 9;
const int cc = lane - ps * 9;
const int kk = (0x26124 >> (2 * cc)) & 3;   // TI[cc] packed 2 bits each: 0,1,2,0,1,0,2,1,2
const int LL = (0x18864 >> (2 * cc)) & 3;   // TJ[cc]: 0,1,2,1,0,2,0,2,1
const double mk0 = kk == 0 ? 1.0 : 0.0, mk1 = kk == 1 ? 1.0 : 0.0, mk2 = kk == 2 ? 1.0 : 0.0;
