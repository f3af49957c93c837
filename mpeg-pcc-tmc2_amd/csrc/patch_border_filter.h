// patch_border_filter.h -- the rule of T7, occupancy synthesis (the reference: patch border filtering, pbfEnableFlag_), that the
// device kernels (patch_border_filter.hip) and the host restatement (patch_border_filter_host.cpp) share word for word.
// Replaces PatchBlockFiltering::patchBorderFiltering with PCCPatch::setLocalData / generateBorderPoints3D / filtering / isBorder
// (PccLibCommon/source/PCCPatch.cpp:797-976).
//
// Per patch a padded occupancy map and a padded int16 depth map (ring of pbfBorder pixels, all zero); an occupied pixel with an
// empty pixel among its 12 neighbours gives a border point; the border points of the patches whose boxes meet the patch's land
// on the patch's own map as "neighbour depths"; passesCount ping-pong passes then keep or drop every pixel of the rim by
// comparing two sums of distances to the neighbour depths in an oriented window (pbfKeepPixel).
//
// Arithmetic: every square root is of an int, taken in fp64; the two sums are FLOAT, each step float( double( sum ) + root ).
// The int under the root is formed with the wrap-around of 32-bit arithmetic (depths are arbitrary int16: a difference squared
// can pass 2^31; the root of the negative int is a NaN, which loses every comparison -- on both sides alike).
#pragma once
#include <cmath>
#include <cstdint>

#if defined( __HIPCC__ )
#include <hip/hip_runtime.h>
#define TMC2_PBF_HD __host__ __device__ __forceinline__
#else
#define TMC2_PBF_HD inline
#endif

namespace tmc2 {

constexpr int     kPbfUndefined  = 32767;  // a neighbour depth that is not there (and one that happens to have this value)
constexpr int     kPbfBoxGrow    = 8;      // a border point lands on a patch if it lies in the patch's box grown by this much
constexpr int     kPbfMaxPatches = 65535;  // the source patch of a landing takes 16 bits of the scatter's key

struct PbfParams {
  int thresholdLossyOM, passesCount, filterSize, log2Threshold;
};

TMC2_PBF_HD int pbfBorder( int occupancyPrecision ) { return occupancyPrecision >= 8 ? 16 : 8; }

// what is refused, by name (nullptr: supported): the reference keeps the three parameters in an int8_t, shifts by 3 for
// precision 16, and lets a window larger than the ring leave its padded map
inline const char* pbfRefusal( int occupancyPrecision, const PbfParams& q, long patchCount ) {
  if ( occupancyPrecision != 1 && occupancyPrecision != 2 && occupancyPrecision != 4 && occupancyPrecision != 8 )
    return "occupancyPrecision (1, 2, 4 or 8)";
  if ( q.passesCount < 1 || q.passesCount > 127 ) return "passesCount (1 .. 127)";
  if ( q.filterSize < 1 || q.filterSize > 127 ) return "filterSize (1 .. 127)";
  if ( q.log2Threshold < 1 || q.log2Threshold > 127 ) return "log2Threshold (1 .. 127)";
  if ( q.filterSize + ( q.filterSize >> 1 ) > pbfBorder( occupancyPrecision ) )
    return "filterSize (filterSize + filterSize / 2 must not exceed the ring of the padded map: 8 pixels, 16 at precision 8)";
  if ( q.thresholdLossyOM < 0 || q.thresholdLossyOM > 255 ) return "thresholdLossyOM (0 .. 255)";
  if ( patchCount > kPbfMaxPatches ) return "patch count (at most 65535)";
  return nullptr;
}

// ---- orientation of a rim pixel from its 8 neighbours ---------------------------------------------------------------------
// pattern: top-left = bit 7, top 6, top-right 5, left 4, right 3, bottom-left 2, bottom 1, bottom-right 0.  The non-zero entries
// as (pattern, orientation) pairs, grouped by orientation; every other pattern has orientation 0.  tests/golden/
// patch_border_filtering.npz pins all 256 values.
#define TMC2_PBF_ORIENTATIONS( X )                                                                                       \
  X( 208, 1 ) X( 209, 1 ) X( 212, 1 ) X( 240, 1 ) X( 244, 1 ) X( 246, 1 ) X( 252, 1 )                                   \
  X( 64, 2 ) X( 224, 2 ) X( 248, 2 ) X( 253, 2 )                                                                         \
  X( 104, 3 ) X( 105, 3 ) X( 108, 3 ) X( 232, 3 ) X( 233, 3 ) X( 235, 3 ) X( 249, 3 )                                   \
  X( 8, 4 ) X( 41, 4 ) X( 107, 4 ) X( 239, 4 )                                                                           \
  X( 11, 5 ) X( 15, 5 ) X( 43, 5 ) X( 47, 5 ) X( 63, 5 ) X( 111, 5 ) X( 139, 5 )                                         \
  X( 2, 6 ) X( 7, 6 ) X( 31, 6 ) X( 191, 6 )                                                                             \
  X( 22, 7 ) X( 23, 7 ) X( 54, 7 ) X( 150, 7 ) X( 151, 7 ) X( 159, 7 ) X( 215, 7 )
TMC2_PBF_HD int pbfOrientation( int pattern ) {
  switch ( pattern ) {
#define TMC2_PBF_CASE( p, o ) \
  case p: return o;
    TMC2_PBF_ORIENTATIONS( TMC2_PBF_CASE )
#undef TMC2_PBF_CASE
    default: return 0;
  }
}
// the 8 compass steps, starting at (1, 0) and turning towards (1, 1): x of direction o; y is x a quarter turn earlier
TMC2_PBF_HD int pbfStepX( int o ) { return ( o == 0 || o == 1 || o == 7 ) ? 1 : ( o >= 3 && o <= 5 ) ? -1 : 0; }
TMC2_PBF_HD int pbfStepY( int o ) { return pbfStepX( ( o + 6 ) & 7 ); }

TMC2_PBF_HD double pbfSqrt( int32_t v ) {
#if defined( __HIP_DEVICE_COMPILE__ )
  return __dsqrt_rn( double( v ) );
#else
  return std::sqrt( double( v ) );
#endif
}
TMC2_PBF_HD float pbfAccumulate( float sum, double root ) {
#if defined( __HIP_DEVICE_COMPILE__ )
  return __double2float_rn( __dadd_rn( double( sum ), root ) );
#else
  return float( double( sum ) + root );
#endif
}
// du^2 + dv^2 + dd^2 as 32-bit arithmetic leaves it
TMC2_PBF_HD int32_t pbfSquares( int du, int dv, int dd ) {
  return int32_t( uint32_t( du ) * uint32_t( du ) + uint32_t( dv ) * uint32_t( dv ) + uint32_t( dd ) * uint32_t( dd ) );
}

// ---- a border point ---------------------------------------------------------------------------------------------------
// occ: the padded map BEFORE filtering, c = the pixel, w = the map's width
TMC2_PBF_HD bool pbfIsBorderPoint( const uint8_t* occ, int64_t c, int w ) {
  return occ[c] && ( !occ[c - 1] || !occ[c + 1] || !occ[c - w] || !occ[c + w] || !occ[c - 2] || !occ[c + 2] || !occ[c - 2 * w] ||
                     !occ[c + 2 * w] || !occ[c + w - 1] || !occ[c + w + 1] || !occ[c - w - 1] || !occ[c - w + 1] );
}
// the normal coordinate of a point as the reconstruction makes it (the depth sample is the uint16 of the geometry video again)
TMC2_PBF_HD int pbfNormalCoord( int mode, int d1, int16_t depth ) {
  const int d = int( uint16_t( depth ) );
  return mode == 0 ? d + d1 : ( d1 - d > 0 ? d1 - d : 0 );
}
// the depth a border point has in the frame of another patch
TMC2_PBF_HD int pbfDepthIn( int mode, int d1, int16_t normal ) { return int( int16_t( mode == 0 ? int( normal ) - d1 : d1 - int( normal ) ) ); }

struct PbfBox {
  int16_t lo[3], hi[3];
};
TMC2_PBF_HD bool pbfBoxesMeet( const PbfBox& a, const PbfBox& b ) {
  return a.hi[0] >= b.lo[0] && a.lo[0] <= b.hi[0] && a.hi[1] >= b.lo[1] && a.lo[1] <= b.hi[1] && a.hi[2] >= b.lo[2] && a.lo[2] <= b.hi[2];
}
TMC2_PBF_HD bool pbfInGrownBox( const PbfBox& b, const int16_t p[3] ) {
  for ( int k = 0; k < 3; ++k )
    if ( p[k] < int16_t( b.lo[k] - kPbfBoxGrow ) || p[k] > int16_t( b.hi[k] + kPbfBoxGrow ) ) return false;
  return true;
}

// ---- one pixel of one pass --------------------------------------------------------------------------------------------
// src: the pass's source map, depth / nd: the patch's depth map and neighbour depths (kPbfUndefined: none), all padded, w wide;
// c: an interior pixel.  The window reaches filterSize + filterSize / 2 pixels at most: inside the ring (pbfRefusal).
TMC2_PBF_HD uint8_t pbfKeepPixel( const uint8_t* src, const int16_t* depth, const int16_t* nd, int64_t c, int w, int filterSize ) {
  if ( !src[c] ) return 0;
  const int n = src[c - 1] + src[c + 1] + src[c - w] + src[c + w];
  if ( n == 0 ) return 0;
  if ( n == 4 ) return 1;
  const int pattern = ( src[c - w - 1] << 7 ) | ( src[c - w] << 6 ) | ( src[c - w + 1] << 5 ) | ( src[c - 1] << 4 ) | ( src[c + 1] << 3 ) |
                      ( src[c + w - 1] << 2 ) | ( src[c + w] << 1 ) | int( src[c + w + 1] );
  const int orX = pbfOrientation( pattern ), orY = ( orX + 2 ) & 7;
  const int xx = pbfStepX( orX ), xy = pbfStepY( orX ), yx = pbfStepX( orY ), yy = pbfStepY( orY );
  const int dE = depth[c - ( xx + xy * w )], dP = depth[c];
  const int sizeV = filterSize >> 1;
  float     sumE = 0.f, sumP = 0.f;
  int       count = 0;
  for ( int dx = -filterSize; dx <= filterSize; ++dx )
    for ( int dy = -sizeV; dy <= sizeV; ++dy ) {
      const int du = dx * xx + dy * yx, dv = dx * xy + dy * yy;
      const int v  = nd[c + du + int64_t( dv ) * w];
      if ( v == kPbfUndefined ) continue;
      sumP = pbfAccumulate( sumP, pbfSqrt( pbfSquares( du, dv, v - dP ) ) );
      sumE = pbfAccumulate( sumE, pbfSqrt( pbfSquares( du + xx, dv + xy, v - dE ) ) );
      ++count;
    }
  return ( count == 0 || sumE >= sumP ) ? 1 : 0;
}

// isBorder( u, v ): a zero in the 5x5 window of the filtered map around the pixel, the ring included
TMC2_PBF_HD uint8_t pbfBorderFlag( const uint8_t* occ, int64_t c, int w ) {
  for ( int dy = -2; dy <= 2; ++dy )
    for ( int dx = -2; dx <= 2; ++dx )
      if ( !occ[c + dx + int64_t( dy ) * w] ) return 1;
  return 0;
}

}  // namespace tmc2
