// color_smoothing_host.cpp -- PCCCodec::colorSmoothing (PccLibCommon/source/PCCCodec.cpp:151-238) restated on the host, with no
// device: the marked cells as a sorted list of cell keys, the points of a cell in point order (so the float sums are the
// reference's additions, whatever their size), the median from the sorted lumas, and the per-point filter of color_smoothing.h
// -- the same text the device kernel runs.  What the CPU test tier checks against the recorded reference results, and what
// the GPU tier holds the kernels against on states no fixture covers.
#include <algorithm>
#include <vector>

#include "color_smoothing.h"
#include "internal.h"

namespace tmc2 {
namespace {
struct HostCells {
  CellGrid                     g;
  const std::vector<uint32_t>* keys;
  const std::vector<ColorCell>* table;
  long slot( uint32_t key ) const {
    const auto it = std::lower_bound( keys->begin(), keys->end(), key );
    return ( it != keys->end() && *it == key ) ? long( it - keys->begin() ) : -1;
  }
  ColorCell operator()( int cx, int cy, int cz ) const {
    const long s = slot( g.key( cx, cy, cz ) );
    return s < 0 ? ColorCell{0u, {0.f, 0.f, 0.f}, 0u} : ( *table )[size_t( s )];
  }
};
}  // namespace

int colorSmoothingHost( const int16_t* xyz, uint16_t* colors16, const uint16_t* boundaryType, const uint32_t* patchIndex, uint64_t M,
                        int gridSize, int bits3d, double thrSmoothing, double thrDifference, double thrVariation ) {
  if ( !colorGridSupported( gridSize, bits3d ) ) {
    setError( "host_color_smoothing: gridSize %d at geometryBitDepth3D %d unsupported (grid sizes 2, 4, 8, 16; at most 2^31 cells)", gridSize,
              bits3d );
    return TMC2_E_UNSUPPORTED;
  }
  const CellGrid g = cubeCellGrid( gridSize, bits3d );
  for ( uint64_t i = 0; i < M; ++i )
    if ( !csInCube( g, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2] ) ) {
      setError( "host_color_smoothing: a point lies outside the cube of %d^3 (geometryBitDepth3D %d)", g.th, bits3d );
      return TMC2_E_INVALID;
    }
  std::vector<uint32_t> keys;
  for ( uint64_t i = 0; i < M; ++i ) {
    const int x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    if ( boundaryType[i] != 1 || g.outside( x, y, z ) ) continue;
    const int qx = g.lowerCell( x ), qy = g.lowerCell( y ), qz = g.lowerCell( z );
    for ( int k = 0; k < 8; ++k ) keys.push_back( g.key( qx + ( k & 1 ), qy + ( ( k >> 1 ) & 1 ), qz + ( k >> 2 ) ) );
  }
  std::sort( keys.begin(), keys.end() );
  keys.erase( std::unique( keys.begin(), keys.end() ), keys.end() );
  if ( keys.empty() ) return TMC2_OK;
  std::vector<ColorCell> table( keys.size(), ColorCell{0u, {0.f, 0.f, 0.f}, 0u} );
  const HostCells        cells{g, &keys, &table};
  // the points of every marked cell, in point order
  std::vector<long>     slotOf( M );
  std::vector<uint32_t> offset( keys.size() + 1, 0u );
  for ( uint64_t i = 0; i < M; ++i ) {
    slotOf[i] = cells.slot( g.keyOfPoint( xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2] ) );
    if ( slotOf[i] >= 0 ) ++offset[size_t( slotOf[i] ) + 1];
  }
  for ( size_t c = 0; c < keys.size(); ++c ) {
    if ( offset[c + 1] > kCellMaxCount ) {
      setError( "host_color_smoothing: a grid cell holds %u points, more than 65535 (the reference's uint16 count wraps there)", offset[c + 1] );
      return TMC2_E_UNSUPPORTED;
    }
    offset[c + 1] += offset[c];
  }
  std::vector<uint32_t> cursor( offset.begin(), offset.end() - 1 ), entries( offset.back() );
  for ( uint64_t i = 0; i < M; ++i )
    if ( slotOf[i] >= 0 ) entries[cursor[size_t( slotOf[i] )]++] = uint32_t( i );
  std::vector<uint16_t> luma;
  for ( size_t c = 0; c < keys.size(); ++c ) {
    const uint32_t n = offset[c + 1] - offset[c];
    if ( n == 0 ) continue;
    ColorCell& cell = table[c];
    cell.count      = n;
    uint64_t lumaSum = 0;
    bool     two     = false;
    luma.clear();
    for ( uint32_t e = offset[c]; e < offset[c + 1]; ++e ) {
      const uint32_t i = entries[e];
      for ( int k = 0; k < 3; ++k ) cell.sum[k] = cell.sum[k] + float( colors16[3 * size_t( i ) + k] );
      lumaSum += colors16[3 * size_t( i )];
      luma.push_back( colors16[3 * size_t( i )] );
      if ( patchIndex[i] != patchIndex[entries[offset[c]]] ) two = true;
    }
    std::sort( luma.begin(), luma.end() );
    cell.flags = csCellFlags( n, lumaSum, n > 1 ? luma[n / 2 - 1] : 0u, luma[n / 2], two, thrVariation );
  }
  for ( uint64_t i = 0; i < M; ++i ) {
    const int P[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
    if ( boundaryType[i] != 1 || g.outside( P[0], P[1], P[2] ) ) continue;
    const uint16_t own[3] = {colors16[3 * i], colors16[3 * i + 1], colors16[3 * i + 2]};
    uint16_t       res[3];
    if ( csFilterPoint( g, P, own, cells, thrSmoothing, thrDifference, res ) )
      for ( int k = 0; k < 3; ++k ) colors16[3 * i + k] = res[k];  // (the cell table is finished: in place couples nothing)
  }
  return TMC2_OK;
}
}  // namespace tmc2

extern "C" int tmc2_host_color_smoothing( const int16_t* xyz, uint16_t* colors16, const uint16_t* boundaryType, const uint32_t* patchIndex,
                                          uint64_t M, int gridSize, int geometryBitDepth3D, double thresholdColorSmoothing,
                                          double thresholdColorDifference, double thresholdColorVariation ) {
  if ( M && ( !xyz || !colors16 || !boundaryType || !patchIndex ) ) {
    tmc2::setError( "host_color_smoothing: invalid argument" );
    return TMC2_E_INVALID;
  }
  return tmc2::colorSmoothingHost( xyz, colors16, boundaryType, patchIndex, M, gridSize, geometryBitDepth3D, thresholdColorSmoothing,
                                   thresholdColorDifference, thresholdColorVariation );
}
