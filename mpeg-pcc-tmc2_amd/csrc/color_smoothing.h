// color_smoothing.h -- the arithmetic of T6 (PCCCodec::colorSmoothing, PccLibCommon/source/PCCCodec.cpp:151-238) that the device
// kernels (color_smoothing.hip) and the host restatement (color_smoothing_host.cpp) share word for word, on the grid of
// cell_grid.h: the verdict on one cell (mean against median of its lumas) and the filter of one point (gridFilteringColor :1193-1277 +
// smoothPointCloudColorLC :1279-1317).  Everything is fp64 on values that fit an int, divided with one rounding.
//
// The three abs() of the reference take a double and are the INTEGER abs (the difference is truncated toward zero first):
// that is how the reference is compiled, the fixture tests/golden/color_smoothing.npz holds cases that depend on it.
#pragma once
#include <cstdint>

#include "cell_grid.h"

namespace tmc2 {

// gridSize 2 / 4 / 8 / 16 and 3D bit depths whose grid has at most 2^31 cells (the reference names a cell by an int)
inline bool colorGridSupported( int gridSize, int bits3d ) {
  if ( gridSize != 2 && gridSize != 4 && gridSize != 8 && gridSize != 16 ) return false;
  if ( bits3d < 5 || bits3d > 14 ) return false;
  const uint64_t w = ( uint64_t( 1 ) << bits3d ) / uint64_t( gridSize );
  return w * w * w <= ( uint64_t( 1 ) << 31 );
}
TMC2_HD bool csInCube( const CellGrid& g, int x, int y, int z ) {
  return x >= 0 && y >= 0 && z >= 0 && x < g.th && y < g.th && z < g.th;
}
TMC2_HD double csDiv( double a, double b ) {
#if defined( __HIP_DEVICE_COMPILE__ )
  return __ddiv_rn( a, b );
#else
  return a / b;
#endif
}
TMC2_HD double csIntAbs( double v ) {  // abs( int( v ) ): what the reference's abs() on a double is
  const int t = int( v );
  return double( t < 0 ? -t : t );
}

// one marked cell as the filter reads it: colorSmoothingCount_ / colorSmoothingCenter_ (the float sums as the reference's
// additions in point order leave them) / colorSmoothingDoSmooth_ and the outcome of the cell's mean-against-median test
struct ColorCell {
  uint32_t count;
  float    sum[3];
  uint32_t flags;
};
constexpr uint32_t kCellDoSmooth = 1u, kCellVaried = 2u;
constexpr uint32_t kCellMaxCount = 65535u;       // colorGridCount is a uint16_t: beyond it the reference wraps
constexpr uint32_t kCellExactSum = 1u << 24;     // below it a float sum of integers is exact in any order

// lumaSum: exact sum of the cell's lumas; medianLo / medianHi: its values of rank n/2 - 1 and n/2 in sorted order
TMC2_HD uint32_t csCellFlags( uint32_t count, uint64_t lumaSum, uint32_t medianLo, uint32_t medianHi, bool twoPatches,
                                 double thresholdColorVariation ) {
  uint32_t flags = twoPatches ? kCellDoSmooth : 0u;
  if ( count > 1 ) {
    const double mean   = csDiv( double( lumaSum ), double( count ) );
    const double median = ( count % 2 == 0 ) ? csDiv( double( medianHi ) + double( medianLo ), 2.0 ) : double( medianHi );
    if ( csIntAbs( mean - median ) > thresholdColorVariation * 256.0 ) flags |= kCellVaried;
  }
  return flags;
}

// The filter of one boundary point inside the faces.  cellAt( cx, cy, cz ) returns the ColorCell of a grid cell (count 0 for
// one that holds nothing).  Returns true and the new colour when the point changes.
template <typename CellAt>
TMC2_HD bool csFilterPoint( const CellGrid& g, const int P[3], const uint16_t own[3], const CellAt& cellAt, double thresholdSmoothing,
                               double thresholdDifference, uint16_t out[3] ) {
  const int S[3] = {g.lowerCell( P[0] ), g.lowerCell( P[1] ), g.lowerCell( P[2] )};
  ColorCell cell[8];
  bool      other = false;
  for ( int k = 0; k < 8; ++k ) {
    cell[k] = cellAt( S[0] + ( k & 1 ), S[1] + ( ( k >> 1 ) & 1 ), S[2] + ( k >> 2 ) );
    if ( ( cell[k].flags & kCellDoSmooth ) && cell[k].count != 0 ) other = true;
  }
  if ( !other ) return false;
  const double cur[3]  = {double( own[0] ), double( own[1] ), double( own[2] )};
  const double yThresh = thresholdDifference * 256.0;
  double       c3[8][3];
  double       Y0 = 0.0;
  for ( int k = 0; k < 8; ++k ) {
    bool keepOwn = cell[k].count == 0;
    if ( !keepOwn ) {
      const double n = double( cell[k].count );
      for ( int c = 0; c < 3; ++c ) c3[k][c] = csDiv( double( cell[k].sum[c] ), n );
      const bool varied = cell[k].count > 1 && ( cell[k].flags & kCellVaried );
      if ( k == 0 ) {
        if ( varied ) return false;  // the result is the point's own colour: nothing changes
      } else {
        keepOwn = csIntAbs( Y0 - c3[k][0] ) > yThresh || varied;
      }
    }
    if ( keepOwn )
      for ( int c = 0; c < 3; ++c ) c3[k][c] = cur[c];
    if ( k == 0 ) Y0 = c3[0][0];
  }
  const int gridSize2 = g.gridSize * 2;
  int       Wt[3], Q[3];
  for ( int k = 0; k < 3; ++k ) {
    Wt[k] = ( P[k] - S[k] * g.gridSize - g.half ) * 2 + 1;
    Q[k]  = gridSize2 - Wt[k];
  }
  double cen[3] = {0.0, 0.0, 0.0};
  for ( int k = 0; k < 8; ++k ) {
    const double wd = double( ( ( k & 1 ) ? Wt[0] : Q[0] ) * ( ( ( k >> 1 ) & 1 ) ? Wt[1] : Q[1] ) * ( ( k >> 2 ) ? Wt[2] : Q[2] ) );
    for ( int c = 0; c < 3; ++c ) cen[c] += c3[k][c] * wd;
  }
  const double norm = double( gridSize2 * gridSize2 * gridSize2 );
  for ( int c = 0; c < 3; ++c ) cen[c] = double( int64_t( csDiv( cen[c], norm ) + 0.5 ) );
  if ( csDiv( csIntAbs( cen[0] - cur[0] ) * 10.0, 256.0 ) >= thresholdSmoothing ) {
    for ( int c = 0; c < 3; ++c ) out[c] = uint16_t( int64_t( cen[c] ) );
    return true;
  }
  return false;
}

}  // namespace tmc2
