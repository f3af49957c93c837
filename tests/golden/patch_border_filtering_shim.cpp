// patch_border_filtering_shim.cpp -- FIXTURE GENERATION ONLY (tests/golden/make_patch_border_filtering_golden.py compiles it into
// a temporary directory against oracle/_ref/libtmc2ref.so and the reference's headers; never part of the product library, never
// built by build()).  Two entries on plain arrays:
//   pbf_filter                the unmodified PatchBlockFiltering::patchBorderFiltering on FRESH PCCPatch objects (the reference's
//                             occupancyMap_.resize keeps stale values when a patch is filtered twice), then
//                             PCCPatch::getOccupancyMap( u, v ) and isBorder( u, v ) of every interior pixel
//   pbf_generate_point_cloud  the unmodified PCCCodec::generatePointCloud with pbfEnableFlag_ on a context filled from the same
//                             arrays, then -- with decoded attribute frames -- the 16-bit colour of every point's pixel (what
//                             colorPointCloud's single-stream branch gathers), PCCCodec::smoothPointCloudPostprocess and
//                             PCCPointSet3::convertYUV16ToRGB8, in the order of PCCDecoder::decode :333-470 for such a stream
//                             (no transferColors16bitBP)
#include "PCCCommon.h"
#include "PCCBitstream.h"
#include "PCCVideoBitstream.h"
#include "PCCContext.h"
#include "PCCFrameContext.h"
#include "PCCPatch.h"
#include "PCCGroupOfFrames.h"
#include "PCCCodec.h"
#include "PCCPointSet.h"

#include <chrono>
#include <cstdio>
#include <unistd.h>

namespace {
// one record: normalAxis, tangentAxis, bitangentAxis, projectionMode, u1, v1, d1, sizeU0, sizeV0, u0, v0, patchOrientation
constexpr int kFields = 12;

void fillPatches( std::vector<pcc::PCCPatch>& patches, const int32_t* records, int count ) {
  patches.clear();
  patches.resize( size_t( count ) );
  for ( int k = 0; k < count; ++k ) {
    const int32_t* r = records + size_t( k ) * kFields;
    pcc::PCCPatch& p = patches[size_t( k )];
    p.setIndex( size_t( k ) );
    p.setAxis( 0, size_t( r[0] ), size_t( r[1] ), size_t( r[2] ), size_t( r[3] ) );
    p.setU1( size_t( r[4] ) ), p.setV1( size_t( r[5] ) ), p.setD1( size_t( r[6] ) );
    p.setSizeU0( size_t( r[7] ) ), p.setSizeV0( size_t( r[8] ) );
    p.setSizeU( size_t( r[7] ) * 16 ), p.setSizeV( size_t( r[8] ) * 16 );
    p.setPatchSize2DXInPixel( size_t( r[7] ) * 16 ), p.setPatchSize2DYInPixel( size_t( r[8] ) * 16 );
    p.setU0( size_t( r[9] ) ), p.setV0( size_t( r[10] ) ), p.setPatchOrientation( size_t( r[11] ) );
    p.setOccupancyResolution( 16 );
    p.setLodScaleX( 1 ), p.setLodScaleYIdc( 1 );
  }
}

struct Silence {  // the reference prints progress with printf
  int   saved;
  FILE* sink;
  Silence() {
    fflush( stdout );
    sink  = fopen( "/dev/null", "w" );
    saved = dup( 1 );
    dup2( fileno( sink ), 1 );
  }
  ~Silence() {
    fflush( stdout );
    dup2( saved, 1 );
    close( saved );
    fclose( sink );
  }
};
}  // namespace

extern "C" int pbf_filter( const int32_t* records, int count, int width, int height, int precision, const uint8_t* occVideo, const uint16_t* geo0,
                           const uint32_t* blockToPatch, int thresholdLossyOM, int passes, int filterSize, int log2Threshold, uint8_t* occupancy,
                           uint8_t* border, double* seconds ) {
  std::vector<pcc::PCCPatch> patches;
  fillPatches( patches, records, count );
  const std::vector<uint8_t>  ocm( occVideo, occVideo + size_t( width / precision ) * size_t( height / precision ) );
  const std::vector<uint16_t> geo( geo0, geo0 + size_t( width ) * size_t( height ) );
  std::vector<size_t>         b2p( blockToPatch, blockToPatch + size_t( width / 16 ) * size_t( height / 16 ) );
  std::vector<uint32_t>       unused;
  pcc::PatchBlockFiltering    filter;
  filter.setPatches( &patches );
  filter.setBlockToPatch( &b2p );
  filter.setOccupancyMapEncoder( &unused );
  filter.setOccupancyMapVideo( &ocm );
  filter.setGeometryVideo( &geo );
  const auto t0 = std::chrono::steady_clock::now();
  filter.patchBorderFiltering( size_t( width ), size_t( height ), 16, size_t( precision ), size_t( thresholdLossyOM ), int8_t( passes ),
                               int8_t( filterSize ), int8_t( log2Threshold ) );
  if ( seconds ) *seconds = std::chrono::duration<double>( std::chrono::steady_clock::now() - t0 ).count();
  size_t at = 0;
  for ( auto& p : patches )
    for ( size_t v = 0; v < p.getSizeV0() * 16; ++v )
      for ( size_t u = 0; u < p.getSizeU0() * 16; ++u, ++at ) {
        occupancy[at] = uint8_t( p.getOccupancyMap( u, v ) != 0 );
        border[at]    = uint8_t( p.isBorder( u, v ) );
      }
  return 0;
}

// geometry: uint16 [2][H][W]; attribute: uint16 [2][3][H][W] or null.  Outputs hold `capacity` points: xyz int16 [M][3] and
// pointToPixel uint32 [M][3] as generatePointCloud left them, boundaryType uint16 [M] likewise; with attribute frames also the
// positions after the smoothing, the 16-bit colours, the 8-bit colours and the boundary types after the smoothing.  Returns the
// number of points, or a negative value.  seconds[0]: generatePointCloud, seconds[1]: smoothPointCloudPostprocess.
extern "C" long pbf_generate_point_cloud( const int32_t* records, int count, int width, int height, int precision, const uint8_t* occVideo,
                                          const uint16_t* geometry, const uint32_t* blockToPatch, int thresholdLossyOM, int passes, int filterSize,
                                          int log2Threshold, const uint16_t* attribute, int gridSize, double thresholdSmoothing, long capacity,
                                          int16_t* xyz, uint32_t* pointToPixel, uint16_t* boundaryType, int16_t* xyzPost, uint16_t* colors16,
                                          uint8_t* rgb, uint16_t* boundaryTypePost, double* seconds ) {
  using namespace pcc;
  Silence                 quiet;
  PCCContext              context;
  static PCCBitstreamStat bitstreamStat;
  context.setBitstreamStat( bitstreamStat );
  context.addV3CParameterSet( 0 );
  context.setActiveVpsId( 0 );
  context.allocateAtlasHLS( 1 );
  context.resizeAtlas( 1 );
  context.setAtlasIndex( 0 );
  context.addAtlasSequenceParameterSet( 0 );
  context.resize( 1 );
  auto& frame = context[0];
  frame.setNumTilesInAtlasFrame( 1 );
  frame.setAtlasFrameWidth( size_t( width ) );
  frame.setAtlasFrameHeight( size_t( height ) );
  auto& tile = frame.getTile( 0 );
  tile.setFrameIndex( 0 );
  tile.setWidth( size_t( width ) ), tile.setHeight( size_t( height ) );
  tile.setLeftTopXInFrame( 0 ), tile.setLeftTopYInFrame( 0 );
  tile.setUseRawPointsSeparateVideo( false );
  fillPatches( tile.getPatches(), records, count );
  tile.getBlockToPatch().assign( blockToPatch, blockToPatch + size_t( width / 16 ) * size_t( height / 16 ) );
  const size_t area = size_t( width ) * size_t( height );
  auto&        occ  = context.getVideoOccupancyMap();
  occ.resize( 1 );
  occ.getFrame( 0 ).resize( size_t( width / precision ), size_t( height / precision ), YUV444 );
  std::copy( occVideo, occVideo + size_t( width / precision ) * size_t( height / precision ), occ.getFrame( 0 ).getChannel( 0 ).begin() );
  auto& geos = context.getVideoGeometryMultiple();
  geos.resize( 1 );
  // (the atlas context clears its geometry videos together with per-video tables that only allocateVideoFrames sizes: hand the
  //  videos back empty)
  struct EmptyOnExit {
    std::vector<PCCVideoGeometry>& v;
    ~EmptyOnExit() { v.clear(); }
  } emptyOnExit{geos};
  geos[0].resize( 2 );
  for ( size_t m = 0; m < 2; ++m ) {
    geos[0].getFrame( m ).resize( size_t( width ), size_t( height ), YUV444 );
    std::copy( geometry + m * area, geometry + ( m + 1 ) * area, geos[0].getFrame( m ).getChannel( 0 ).begin() );
  }
  GeneratePointCloudParameters params;
  params.occupancyResolution_        = 16;
  params.occupancyPrecision_         = size_t( precision );
  params.enableSizeQuantization_     = false;
  params.gridSmoothing_              = true;
  params.gridSize_                   = size_t( gridSize );
  params.neighborCountSmoothing_     = 64;
  params.radius2Smoothing_           = 64.0;
  params.radius2BoundaryDetection_   = 64.0;
  params.thresholdSmoothing_         = thresholdSmoothing;
  params.rawPointColorFormat_        = 0;
  params.nbThread_                   = 1;
  params.multipleStreams_            = false;
  params.absoluteD1_                 = true;
  params.surfaceThickness_           = 4;
  params.thresholdColorSmoothing_    = 10.0;
  params.cgridSize_                  = 4;
  params.thresholdColorDifference_   = 10.0;
  params.thresholdColorVariation_    = 6.0;
  params.flagGeometrySmoothing_      = true;
  params.flagColorSmoothing_         = false;
  params.enhancedOccupancyMapCode_   = false;
  params.EOMFixBitCount_             = 2;
  params.thresholdLossyOM_           = size_t( thresholdLossyOM );
  params.removeDuplicatePoints_      = true;
  params.mapCountMinus1_             = 1;
  params.pointLocalReconstruction_   = false;
  params.singleMapPixelInterleaving_ = false;
  params.useAdditionalPointsPatch_   = false;
  params.useAuxSeperateVideo_        = false;
  params.plrlNumberOfModes_          = 0;
  params.geometryBitDepth3D_         = 11;
  params.geometry3dCoordinatesBitdepth_ = 11;
  params.pbfEnableFlag_              = true;
  params.pbfPassesCount_             = int16_t( passes );
  params.pbfFilterSize_              = int16_t( filterSize );
  params.pbfLog2Threshold_           = int16_t( log2Threshold );
  PCCCodec              codec;
  PCCPointSet3          reconstruct;
  std::vector<uint32_t> partition;
  auto                  t0 = std::chrono::steady_clock::now();
  codec.generatePointCloud( reconstruct, context, 0, 0, params, partition, false );
  if ( seconds ) seconds[0] = std::chrono::duration<double>( std::chrono::steady_clock::now() - t0 ).count();
  const size_t M   = reconstruct.getPointCount();
  auto&        p2p = tile.getPointToPixel();
  if ( long( M ) > capacity || p2p.size() != M || partition.size() != M ) return -1;
  for ( size_t i = 0; i < M; ++i )
    for ( int k = 0; k < 3; ++k ) {
      xyz[3 * i + k]          = reconstruct[i][k];
      pointToPixel[3 * i + k] = uint32_t( p2p[i][k] );
    }
  for ( size_t i = 0; i < M; ++i ) boundaryType[i] = reconstruct.getBoundaryPointType( i );
  if ( !attribute || M == 0 ) return long( M );
  reconstruct.addColors16bit();
  for ( size_t i = 0; i < M; ++i ) {
    const size_t at = size_t( p2p[i][2] ) * 3 * area + size_t( p2p[i][1] ) * size_t( width ) + size_t( p2p[i][0] );
    reconstruct.setColor16bit( i, PCCColor16bit( attribute[at], attribute[at + area], attribute[at + 2 * area] ) );
  }
  t0 = std::chrono::steady_clock::now();
  codec.smoothPointCloudPostprocess( reconstruct, COLOR_TRANSFORM_NONE, params, partition );
  if ( seconds ) seconds[1] = std::chrono::duration<double>( std::chrono::steady_clock::now() - t0 ).count();
  reconstruct.convertYUV16ToRGB8();
  for ( size_t i = 0; i < M; ++i ) {
    const auto c = reconstruct.getColor( i );
    const auto d = reconstruct.getColor16bit( i );
    for ( int k = 0; k < 3; ++k ) {
      xyzPost[3 * i + k]  = reconstruct[i][k];
      colors16[3 * i + k] = d[k];
      rgb[3 * i + k]      = c[k];
    }
    boundaryTypePost[i] = reconstruct.getBoundaryPointType( i );
  }
  return long( M );
}
