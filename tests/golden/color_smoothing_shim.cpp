// color_smoothing_shim.cpp -- FIXTURE GENERATION ONLY (tests/golden/make_color_smoothing_golden.py compiles it into a temporary
// directory against oracle/_ref/libtmc2ref.so and the reference's headers; never part of the product library, never built by
// build()).  Calls the unmodified PCCCodec::colorSmoothing, and PCCPointSet3::convertYUV16ToRGB8 after it, on plain arrays.
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

// xyz int16[M][3], colors16 uint16[M][3] in / out, boundaryType uint16[M], patchIndex uint32[M]; rgb uint8[M][3] out (may be
// null); seconds: the time inside colorSmoothing alone (may be null)
extern "C" int cs_color_smoothing( const int16_t* xyz, uint16_t* colors16, const uint16_t* boundaryType, const uint32_t* patchIndex, size_t M,
                                   int gridSize, int bits3d, double thresholdSmoothing, double thresholdDifference,
                                   double thresholdVariation, uint8_t* rgb, double* seconds ) {
  pcc::PCCCodec     codec;
  pcc::PCCPointSet3 cloud;
  cloud.addColors();
  cloud.addColors16bit();
  cloud.resize( M );
  for ( size_t i = 0; i < M; ++i ) {
    cloud[i] = pcc::PCCPoint3D( xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2] );
    cloud.setColor16bit( i, pcc::PCCColor16bit( colors16[3 * i], colors16[3 * i + 1], colors16[3 * i + 2] ) );
    cloud.setBoundaryPointType( i, boundaryType[i] );
    cloud.setPointPatchIndex( i, 0, patchIndex[i] );
  }
  pcc::GeneratePointCloudParameters params;
  params.flagColorSmoothing_       = true;
  params.occupancyPrecision_       = size_t( gridSize );
  params.geometryBitDepth3D_       = size_t( bits3d );
  params.thresholdColorSmoothing_  = thresholdSmoothing;
  params.thresholdColorDifference_ = thresholdDifference;
  params.thresholdColorVariation_  = thresholdVariation;
  const auto t0 = std::chrono::steady_clock::now();
  codec.colorSmoothing( cloud, pcc::COLOR_TRANSFORM_NONE, params );
  if ( seconds ) *seconds = std::chrono::duration<double>( std::chrono::steady_clock::now() - t0 ).count();
  for ( size_t i = 0; i < M; ++i ) {
    const auto c = cloud.getColor16bit( i );
    for ( int k = 0; k < 3; ++k ) colors16[3 * i + k] = c[k];
  }
  if ( rgb ) {
    cloud.convertYUV16ToRGB8();
    for ( size_t i = 0; i < M; ++i ) {
      const auto c = cloud.getColor( i );
      for ( int k = 0; k < 3; ++k ) rgb[3 * i + k] = c[k];
    }
  }
  return 0;
}
