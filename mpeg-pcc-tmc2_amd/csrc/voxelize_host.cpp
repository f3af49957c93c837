// voxelize_host.cpp -- convertPointsToVoxels restated on the host (voxelize.h compiled for the host; no device), and the refusals
// of the grid-based segmentation that need no device.
#include <unordered_map>

#include "internal.h"
#include "voxelize.h"

namespace tmc2 {

void voxelizeHost( const int16_t* xyz, uint64_t n, VoxelRule r, int16_t* voxelXyz, uint64_t* voxelCount, uint32_t* voxelOfPoint ) {
  std::unordered_map<uint64_t, uint32_t> rankOf;
  rankOf.reserve( size_t( n ) / 2 + 16 );
  uint32_t count = 0;
  for ( uint64_t i = 0; i < n; ++i ) {
    const int  vx = voxelCoord( xyz[3 * i], r ), vy = voxelCoord( xyz[3 * i + 1], r ), vz = voxelCoord( xyz[3 * i + 2], r );
    const auto at = rankOf.emplace( voxelKey( vx, vy, vz, 16 ), count );
    if ( at.second ) {  // the first point of its voxel: the voxel takes the next rank
      voxelXyz[3 * size_t( count )]     = int16_t( vx );
      voxelXyz[3 * size_t( count ) + 1] = int16_t( vy );
      voxelXyz[3 * size_t( count ) + 2] = int16_t( vz );
      ++count;
    }
    voxelOfPoint[i] = at.first->second;
  }
  *voxelCount = count;
}

// the refusals that depend on the voxel size, the bit depth and the coordinates (shared by the host entry, the device entry and the chain)
int voxelizeCheck( const char* who, const int16_t* xyz, uint64_t n, int voxDim, int bits ) {
  int lo = 0, hi = 0;
  if ( n ) lo = hi = xyz[0];
  for ( uint64_t i = 0; i < 3 * n; ++i ) lo = std::min<int>( lo, xyz[i] ), hi = std::max<int>( hi, xyz[i] );
  int offending = 0;
  if ( const char* why = voxelizeRefusal( voxDim, bits, lo, hi, &offending ) ) {
    char text[256];
    snprintf( text, sizeof( text ), why, offending, bits );
    setError( "%s: %s", who, text );
    return TMC2_E_UNSUPPORTED;
  }
  return TMC2_OK;
}

}  // namespace tmc2

extern "C" int tmc2_host_convert_points_to_voxels( const int16_t* xyz, uint64_t n, int voxDim, int bits, int16_t* voxelXyz,
                                                   uint64_t* voxelCount, uint32_t* voxelOfPoint ) {
  if ( !xyz || !voxelXyz || !voxelCount || !voxelOfPoint || n == 0 || n > 0x7FFFFFF0ull ) {
    tmc2::setError( "host_convert_points_to_voxels: invalid argument" );
    return TMC2_E_INVALID;
  }
  TMC2_TRY( tmc2::voxelizeCheck( "host_convert_points_to_voxels", xyz, n, voxDim, bits ) );
  tmc2::VoxelRule r;
  tmc2::voxelRuleFor( voxDim, r );
  tmc2::voxelizeHost( xyz, n, r, voxelXyz, voxelCount, voxelOfPoint );
  return TMC2_OK;
}
