// voxelize.h -- the voxelisation rule of the grid-based segmentation (the reference's fast mode), one text for host and device.
//
// Replaces the arithmetic of PCCPatchSegmenter3::convertPointsToVoxels (PccLibEncoder/source/PCCPatchSegmenter.cpp:152-181):
//   shift = log2( voxDim ), half = voxDim >> 1, voxel of a point = ( ( x + half ) >> shift, ( y + half ) >> shift, ( z + half ) >> shift )
// -- ROUNDING, not floor: with voxels of 2, x = 1 lies in voxel 1 and the largest coordinate 2^k - 1 in voxel 2^(k-1), one beyond
// what a floor rule could give.  The voxel cloud lists the voxels in the order of their first point (ascending smallest point
// index, NOT key order), a voxel's position is its voxel coordinate, and every point knows the rank of its voxel in that list.
// The reference names a voxel by x + ( y << bits ) + ( z << 2 bits ) with bits = geometryBitDepth3D: two voxels whose coordinates
// do not fit `bits` bits would share a name there.  Such a frame is refused by name (voxelizeRefusal) instead of reproducing
// the collisions; with that, any injective key gives the reference's list.
#pragma once
#include <cstdint>

#if defined( __HIPCC__ )
#define TMC2_VOXEL_FN __host__ __device__ __forceinline__
#else
#define TMC2_VOXEL_FN inline
#endif

namespace tmc2 {

struct VoxelRule {
  int shift, half;
};
// voxelDimensionGridBasedSegmentation 2, 4 or 8 (anything else: false)
inline bool voxelRuleFor( int voxDim, VoxelRule& r ) {
  if ( voxDim != 2 && voxDim != 4 && voxDim != 8 ) return false;
  r.shift = voxDim == 2 ? 1 : ( voxDim == 4 ? 2 : 3 );
  r.half  = voxDim >> 1;
  return true;
}
TMC2_VOXEL_FN int voxelCoord( int c, VoxelRule r ) { return ( c + r.half ) >> r.shift; }
// injective for voxel coordinates below 2^axisBits (axisBits <= 16)
TMC2_VOXEL_FN uint64_t voxelKey( int vx, int vy, int vz, int axisBits ) {
  return uint64_t( uint32_t( vx ) ) | ( uint64_t( uint32_t( vy ) ) << axisBits ) | ( uint64_t( uint32_t( vz ) ) << ( 2 * axisBits ) );
}
// width of a key field that holds every voxel coordinate up to maxVoxel
inline int voxelAxisBits( int maxVoxel ) {
  int b = 1;
  while ( ( 1 << b ) <= maxVoxel ) ++b;
  return b;
}

// the k-NN self-join of the normal estimation asks for 16 neighbours: a voxel cloud below that is refused
constexpr uint32_t kMinVoxelCloud = 16;

// What the grid-based segmentation refuses before anything is launched, from the voxel size, the bit depth and the cloud's smallest
// and largest coordinate: nullptr, or a printf format (two ints: the offending value, geometryBitDepth3D) that names the field.
inline const char* voxelizeRefusal( int voxDim, int bits, int minCoord, int maxCoord, int* offending ) {
  VoxelRule r;
  if ( !voxelRuleFor( voxDim, r ) ) {
    *offending = voxDim;
    return "voxelDimensionGridBasedSegmentation %d unsupported (2, 4 or 8; geometryBitDepth3D %d)";
  }
  if ( bits < 1 || bits > 16 ) {
    *offending = bits;
    return "geometryBitDepth3D %d outside 1..16 (%d)";
  }
  if ( minCoord < 0 ) {
    *offending = minCoord;
    return "coordinate %d is negative: its voxel does not fit geometryBitDepth3D %d bits";
  }
  if ( voxelCoord( maxCoord, r ) >= ( 1 << bits ) ) {
    *offending = voxelCoord( maxCoord, r );
    return "voxel coordinate %d does not fit geometryBitDepth3D %d bits (the reference's voxel names would collide)";
  }
  return nullptr;
}

// convertPointsToVoxels on the host (voxelize_host.cpp): voxelXyz [n][3] (the first *voxelCount rows are written), voxelOfPoint [n].
// The caller has ruled out voxelizeRefusal.
void voxelizeHost( const int16_t* xyz, uint64_t n, VoxelRule r, int16_t* voxelXyz, uint64_t* voxelCount, uint32_t* voxelOfPoint );

// the refusals above on a host cloud: TMC2_OK, or TMC2_E_UNSUPPORTED with the error "<who>: ..." set
int voxelizeCheck( const char* who, const int16_t* xyz, uint64_t n, int voxDim, int bits );

}  // namespace tmc2
