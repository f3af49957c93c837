// metrics_options_shim.cpp -- FIXTURE GENERATION ONLY (tests/golden/make_metrics_options_golden.py compiles it into a temporary
// directory against oracle/_ref/libtmc2ref.so and the reference's headers; never part of the product library, never built by
// build()).  Fills a PCCMetricsParameters, calls the unmodified PCCMetrics::compute and PCCMetrics::display on plain arrays and
// copies the members out.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <limits>
#include <list>
#include <map>
#include <memory>
#include <queue>
#include <sstream>
#include <string>
#include <unordered_map>
#include <vector>
#include <unistd.h>

// (after every standard header: the members of QualityMetrics and PCCMetrics are read below)
#define private public
#include "PCCCommon.h"
#include "PCCPointSet.h"
#include "PCCGroupOfFrames.h"
#include "PCCMetricsParameters.h"
#include "PCCMetrics.h"
#undef private

namespace {
void fill( pcc::PCCPointSet3& cloud, const int16_t* xyz, const uint8_t* rgb, size_t n ) {
  cloud.addColors();
  cloud.resize( n );
  for ( size_t i = 0; i < n; ++i ) {
    cloud[i] = pcc::PCCPoint3D( xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2] );
    cloud.setColor( i, pcc::PCCColor3B( rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2] ) );
  }
}
}  // namespace

// params[6]: computeC2c, computeC2p, computeColor, computeHausdorff, dropDuplicates, neighborsProc.  out[3][14] in the column
// order of tmc2_metrics_compute_ex; a quantity whose flag is off is written as 0 WITHOUT reading the member (QualityMetrics'
// constructor leaves colorMse_[1 .. 2] and colorPsnr_[1 .. 2] unset).  text / capacity: what display() prints at precision 9
// (returns its size; may be null).  seconds: the time inside compute.
extern "C" long mo_metrics( const int16_t* srcXyz, const uint8_t* srcRgb, size_t n, const int16_t* recXyz, const uint8_t* recRgb, size_t m,
                            const double* srcNormals, double resolution, const int* params, double* out, long long* counts, char* text,
                            long capacity, double* seconds ) {
  pcc::PCCGroupOfFrames sources, recs, normals;
  sources.setFrameCount( 1 );
  recs.setFrameCount( 1 );
  fill( sources[0], srcXyz, srcRgb, n );
  fill( recs[0], recXyz, recRgb, m );
  if ( srcNormals ) {
    normals.setFrameCount( 1 );
    fill( normals[0], srcXyz, srcRgb, n );
    normals[0].addNormals();
    for ( size_t i = 0; i < n; ++i ) normals[0].setNormal( i, pcc::PCCNormal3D( srcNormals[3 * i], srcNormals[3 * i + 1], srcNormals[3 * i + 2] ) );
  }
  pcc::PCCMetricsParameters mp;
  mp.resolution_       = size_t( resolution );
  mp.computeC2c_       = params[0] != 0;
  mp.computeC2p_       = params[1] != 0 && srcNormals != nullptr;
  mp.computeColor_     = params[2] != 0;
  mp.computeHausdorff_ = params[3] != 0;
  mp.dropDuplicates_   = size_t( params[4] );
  mp.neighborsProc_    = size_t( params[5] );
  pcc::PCCMetrics metrics;
  metrics.setParameters( mp );
  // everything the library prints goes to a file of its own; display()'s part of it is what is kept
  char path[] = "/tmp/metrics_options_shim_XXXXXX";
  int  fd     = mkstemp( path );
  fflush( stdout );
  std::cout.flush();
  const int saved = dup( 1 );
  dup2( fd, 1 );
  const auto t0 = std::chrono::steady_clock::now();
  metrics.compute( sources, recs, normals );
  if ( seconds ) *seconds = std::chrono::duration<double>( std::chrono::steady_clock::now() - t0 ).count();
  fflush( stdout );
  std::cout.flush();
  if ( ftruncate( fd, 0 ) != 0 ) return -1;
  lseek( fd, 0, SEEK_SET );
  const auto oldPrecision = std::cout.precision( std::numeric_limits<float>::max_digits10 );
  metrics.display();
  std::cout.flush();
  fflush( stdout );
  std::cout.precision( oldPrecision );
  dup2( saved, 1 );
  close( saved );
  const long size = long( lseek( fd, 0, SEEK_END ) );
  lseek( fd, 0, SEEK_SET );
  if ( text && size < capacity ) {
    const long got = long( read( fd, text, size_t( size ) ) );
    text[got > 0 ? got : 0] = 0;
  }
  close( fd );
  unlink( path );
  pcc::QualityMetrics* q[3] = {&metrics.quality1_[0], &metrics.quality2_[0], &metrics.qualityF_[0]};
  for ( int r = 0; r < 3; ++r ) {
    double* o = out + 14 * r;
    for ( int c = 0; c < 14; ++c ) o[c] = 0.0;
    if ( mp.computeC2c_ ) {
      o[0] = q[r]->c2cMse_, o[1] = q[r]->c2cPsnr_;
      if ( mp.computeHausdorff_ ) o[10] = q[r]->c2cHausdorff_, o[11] = q[r]->c2cHausdorffPsnr_;
    }
    if ( mp.computeC2p_ ) {
      o[2] = q[r]->c2pMse_, o[3] = q[r]->c2pPsnr_;
      if ( mp.computeHausdorff_ ) o[12] = q[r]->c2pHausdorff_, o[13] = q[r]->c2pHausdorffPsnr_;
    }
    if ( mp.computeColor_ )
      for ( int c = 0; c < 3; ++c ) o[4 + c] = q[r]->colorMse_[c], o[7 + c] = q[r]->colorPsnr_[c];
  }
  counts[0] = (long long)metrics.sourceDuplicates_[0];
  counts[1] = (long long)metrics.reconstructDuplicates_[0];
  return size;
}
