// cell_grid.h -- the grid of cubic cells that T3 (geometry smoothing, post_reconstruct.hip) and T6 (colour smoothing,
// color_smoothing.hip, color_smoothing_host.cpp) lay over the finished cloud: PCCCodec.cpp:982-1065 and :1170-1277 restate the
// same geometry.  One text for host and device; on the device also the lookup in the marked cells (cell_grid.hip).
#pragma once
#include <cstdint>

#if defined( __HIPCC__ )
#include <hip/hip_runtime.h>
#define TMC2_HD __host__ __device__ __forceinline__
#else
#define TMC2_HD inline
#endif

namespace tmc2 {

struct CellGrid {
  // w cells a side, th = gridSize * w.  Any EVEN gridSize (T3 takes the even sizes of 2..64): divisions, not shifts.  Even, because
  // only then is half the cell's middle and do the 2x2x2 cells of every point inside the faces lie in the grid; with an odd size a
  // point at th - half - 1 has lowerCell == w - 1 and names cell w
  int gridSize, half, w, disth, th;
  // too close to a face: such a point marks nothing and is not filtered
  TMC2_HD bool outside( int x, int y, int z ) const {
    return x < disth || y < disth || z < disth || th <= x + disth || th <= y + disth || th <= z + disth;
  }
  // the lower corner of the 2x2x2 cells around a coordinate: its cell, or the one before it if it sits in the cell's lower half
  TMC2_HD int lowerCell( int p ) const {
    const int c = p / gridSize;
    return c + ( ( p - c * gridSize < half ) ? -1 : 0 );
  }
  TMC2_HD uint32_t key( int cx, int cy, int cz ) const {  // raster order
    return ( uint32_t( cz ) * uint32_t( w ) + uint32_t( cy ) ) * uint32_t( w ) + uint32_t( cx );
  }
  TMC2_HD uint32_t keyOfPoint( int x, int y, int z ) const { return key( x / gridSize, y / gridSize, z / gridSize ); }
  uint64_t cells() const { return uint64_t( w ) * uint64_t( w ) * uint64_t( w ); }
};
inline CellGrid makeCellGrid( int gridSize, int w ) {
  const int half = gridSize / 2;
  return CellGrid{gridSize, half, w, half > 1 ? half : 1, gridSize * w};
}
// over the cube of 2^bits3d (T6) / over [0, maxCoord] (T3)
inline CellGrid cubeCellGrid( int gridSize, int bits3d ) { return makeCellGrid( gridSize, ( 1 << bits3d ) / gridSize ); }
inline CellGrid extentCellGrid( int gridSize, int maxCoord ) { return makeCellGrid( gridSize, ( maxCoord + gridSize - 1 ) / gridSize ); }

#if defined( __HIPCC__ )
// the marked cells: one bit per cell and, per 32-bit word, the marked cells before it; a slot = the rank in raster order
constexpr uint32_t kNoSlot = 0xFFFFFFFFu;
__device__ __forceinline__ uint32_t slotOfKey( const uint32_t* __restrict__ bits, const uint32_t* __restrict__ rank, uint32_t key ) {
  const uint32_t word = bits[key >> 5], b = key & 31u;
  if ( !( ( word >> b ) & 1u ) ) return kNoSlot;
  return rank[key >> 5] + __popc( word & ( ( 1u << b ) - 1u ) );
}
#endif

}  // namespace tmc2
