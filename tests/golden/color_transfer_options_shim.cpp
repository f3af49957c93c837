// color_transfer_options_shim.cpp -- FIXTURE GENERATION ONLY (tests/golden/make_color_transfer_options_golden.py compiles it into a
// temporary directory against oracle/_ref/libtmc2ref.so and the reference's headers; never part of the product library, never built
// by build()).  Fills two PCCPointSet3 from plain arrays, calls the unmodified PCCPointSet3::transferColors with its sixteen
// arguments and copies the target's colours out.
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <fcntl.h>
#include <unistd.h>

#include "PCCCommon.h"
#include "PCCPointSet.h"

// flags[9]: searchRange, losslessAttribute, numNeighborsColorTransferFwd, ..Bwd, useDistWeightedAverageFwd, ..Bwd,
// skipAvgIfIdenticalSourcePointPresentFwd, ..Bwd, excludeColorOutlier; reals[7]: distOffsetFwd, ..Bwd, maxGeometryDist2Fwd, ..Bwd,
// maxColorDist2Fwd, ..Bwd, thresholdColorOutlierDist.  seconds: the time inside transferColors.  Returns 0, or 1 if it returned false.
extern "C" int cto_transfer( const int16_t* srcXyz, const uint8_t* srcRgb, size_t n, const int16_t* tgtXyz, size_t m, const int* flags,
                             const double* reals, uint8_t* tgtRgb, double* seconds ) {
  pcc::PCCPointSet3 source, target;
  source.addColors();
  source.resize( n );
  for ( size_t i = 0; i < n; ++i ) {
    source[i] = pcc::PCCPoint3D( srcXyz[3 * i], srcXyz[3 * i + 1], srcXyz[3 * i + 2] );
    source.setColor( i, pcc::PCCColor3B( srcRgb[3 * i], srcRgb[3 * i + 1], srcRgb[3 * i + 2] ) );
  }
  target.resize( m );
  for ( size_t i = 0; i < m; ++i ) target[i] = pcc::PCCPoint3D( tgtXyz[3 * i], tgtXyz[3 * i + 1], tgtXyz[3 * i + 2] );
  // (the library prints a line per call: not to the generator's output)
  fflush( stdout );
  const int saved = dup( 1 ), null = open( "/dev/null", 1 );
  dup2( null, 1 );
  const auto t0 = std::chrono::steady_clock::now();
  const bool ok = source.transferColors( target, flags[0], flags[1] != 0, flags[2], flags[3], flags[4] != 0, flags[5] != 0, flags[6] != 0,
                                         flags[7] != 0, reals[0], reals[1], reals[2], reals[3], reals[4], reals[5], flags[8] != 0, reals[6] );
  if ( seconds ) *seconds = std::chrono::duration<double>( std::chrono::steady_clock::now() - t0 ).count();
  fflush( stdout );
  dup2( saved, 1 );
  close( saved );
  close( null );
  if ( !ok ) return 1;
  for ( size_t i = 0; i < m; ++i ) {
    const pcc::PCCColor3B c = target.getColor( i );
    tgtRgb[3 * i] = c[0], tgtRgb[3 * i + 1] = c[1], tgtRgb[3 * i + 2] = c[2];
  }
  return 0;
}
