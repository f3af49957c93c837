// color_transfer_rules.h -- PCCPointSet3::transferColors (PccLibCommon/source/PCCPointSet.cpp:807-1124) over its sixteen arguments:
// the per-target rules that the device kernels (attributes.hip) and the host restatement (color_transfer_host.cpp) share word for
// word.  A target's neighbours and candidates are read through accessors (distAt( i ): squared distance, an integer; colorAt( i ):
// the colour of entry i), so neither side keeps a private copy of a list.  Every mean is fp64 in the reference's order of operations,
// divisions and roots with one rounding, no contraction (-ffp-contract=off).
//
// What reading the reference alone gets wrong (tests/golden/color_transfer_options.npz holds a case for each):
//   1. a threshold >= 512 is none (:834-837), 511 is a threshold;
//   2. the pairwise colour maximum starts at DBL_MIN, not 0 (:874, :997): a threshold of 0 shrinks every list to its nearest entry,
//      equal colours included;
//   3. the geometry threshold keeps the first forward result (:848-852); backward it may leave a target no candidate (:947-951);
//   4. without the skip flag an identical point is one more entry, of weight 1 / distOffset;
//   5. the outlier pass compares the dropped count with the SHRUNK length in both directions (:911; :1030 -- nNN is re-read from
//      the list at :982 after every pop_back);
//   6. the clipped search cube repeats candidates at 0 and 255, the strict < keeps the first (:1109);
//   7. a single remaining entry is taken as it is, unweighted (:863, :983).
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>

#include "cell_grid.h"  // TMC2_HD
#include "tmc2hip.h"

namespace tmc2 {

struct ColorSum {
  double c0, c1, c2;
};
struct CtColor {
  int c0, c1, c2;
};

// tmc2_color_transfer_params as the rules read them
struct CtRules {
  int    searchRange, lossless, kFwd, kBwd, weightedFwd, weightedBwd, skipFwd, skipBwd, outlier;
  double offsetFwd, offsetBwd, geoFwd, geoBwd, colFwd, colBwd, outlier2;  // thresholds: DBL_MAX for none; outlier2: the square
};

constexpr int      kCtMaxNeighbors = 32, kCtMaxSearchRange = 8;
constexpr uint64_t kCtMaxSource    = 0x3FFFFFFull;  // source points: entry numbers source * K + rank stay below 2^32

// the field the entries refuse (TMC2_E_UNSUPPORTED), or nullptr
inline const char* ctRefusal( const tmc2_color_transfer_params& q ) {
  if ( q.searchRange < 0 || q.searchRange > kCtMaxSearchRange ) return "searchRange outside 0..8";
  if ( q.numNeighborsColorTransferFwd < 1 || q.numNeighborsColorTransferFwd > kCtMaxNeighbors ) return "numNeighborsColorTransferFwd outside 1..32";
  if ( q.numNeighborsColorTransferBwd < 1 || q.numNeighborsColorTransferBwd > kCtMaxNeighbors ) return "numNeighborsColorTransferBwd outside 1..32";
  if ( !( q.distOffsetFwd > 0.0 ) ) return "distOffsetFwd not above 0";
  if ( !( q.distOffsetBwd > 0.0 ) ) return "distOffsetBwd not above 0";
  if ( !( q.maxGeometryDist2Fwd >= 0.0 ) ) return "maxGeometryDist2Fwd negative or not a number";
  if ( !( q.maxGeometryDist2Bwd >= 0.0 ) ) return "maxGeometryDist2Bwd negative or not a number";
  if ( !( q.maxColorDist2Fwd >= 0.0 ) ) return "maxColorDist2Fwd negative or not a number";
  if ( !( q.maxColorDist2Bwd >= 0.0 ) ) return "maxColorDist2Bwd negative or not a number";
  if ( !( q.thresholdColorOutlierDist >= 0.0 ) ) return "thresholdColorOutlierDist negative or not a number";
  return nullptr;
}
inline CtRules ctRules( const tmc2_color_transfer_params& q ) {
  const auto limit = []( double t ) { return t < 512 ? t : DBL_MAX; };
  CtRules    r;
  r.searchRange = q.searchRange, r.lossless = q.losslessAttribute != 0;
  r.kFwd = q.numNeighborsColorTransferFwd, r.kBwd = q.numNeighborsColorTransferBwd;
  r.weightedFwd = q.useDistWeightedAverageFwd != 0, r.weightedBwd = q.useDistWeightedAverageBwd != 0;
  r.skipFwd = q.skipAvgIfIdenticalSourcePointPresentFwd != 0, r.skipBwd = q.skipAvgIfIdenticalSourcePointPresentBwd != 0;
  r.outlier   = q.excludeColorOutlier != 0;
  r.offsetFwd = q.distOffsetFwd, r.offsetBwd = q.distOffsetBwd;
  r.geoFwd = limit( q.maxGeometryDist2Fwd ), r.geoBwd = limit( q.maxGeometryDist2Bwd );
  r.colFwd = limit( q.maxColorDist2Fwd ), r.colBwd = limit( q.maxColorDist2Bwd );
  r.outlier2 = q.thresholdColorOutlierDist * q.thresholdColorOutlierDist;
  return r;
}
inline void ctDefault( tmc2_color_transfer_params& q ) {
  q = tmc2_color_transfer_params{0, 0, 8, 1, 1, 1, 1, 1, 4.0, 4.0, 1000.0, 1000.0, 1000.0, 1000.0, 0, 10.0};
}
// the CTC point in everything the rules read: the entries then run the kernels written for it
inline bool ctIsDefault( const tmc2_color_transfer_params& q ) {
  const CtRules r = ctRules( q );
  return r.searchRange == 0 && !r.lossless && r.kFwd == 8 && r.kBwd == 1 && r.weightedFwd && r.weightedBwd && r.skipFwd && r.skipBwd &&
         r.offsetFwd == 4.0 && r.offsetBwd == 4.0 && r.geoFwd == DBL_MAX && r.geoBwd == DBL_MAX && r.colFwd == DBL_MAX && r.colBwd == DBL_MAX &&
         !r.outlier;
}

TMC2_HD double ctDiv( double a, double b ) {
#if defined( __HIP_DEVICE_COMPILE__ )
  return __ddiv_rn( a, b );
#else
  return a / b;
#endif
}
TMC2_HD double ctSqrt( double a ) {
#if defined( __HIP_DEVICE_COMPILE__ )
  return __dsqrt_rn( a );
#else
  return std::sqrt( a );
#endif
}
TMC2_HD int ctClip255( double v ) { return int( fmax( 0.0, fmin( v, 255.0 ) ) ); }
TMC2_HD CtColor ctRounded( const ColorSum& v ) { return CtColor{ctClip255( round( v.c0 ) ), ctClip255( round( v.c1 ) ), ctClip255( round( v.c2 ) )}; }
TMC2_HD int ctDist2( const CtColor& a, const CtColor& b ) {
  const int d0 = a.c0 - b.c0, d1 = a.c1 - b.c1, d2 = a.c2 - b.c2;
  return d0 * d0 + d1 * d1 + d2 * d2;
}

// The shrink loop (:862-929, :981-1043): the longest prefix of the n >= 1 entries whose maximal pairwise squared colour distance is
// <= limit.  The reference recomputes every pair per step from the full list down; the maximum of a prefix only grows with its
// length, so it is carried upwards instead -- the same integers, the first length that fails ends it.
template <typename ColorAt>
TMC2_HD int ctShrink( int n, double limit, const ColorAt& colorAt ) {
  if ( limit == DBL_MAX ) return n;
  int kept = 1, maxPair = 0;
  for ( int j = 1; j < n; ++j ) {
    const CtColor cj = colorAt( j );
    for ( int i = 0; i < j; ++i ) {
      const int d = ctDist2( colorAt( i ), cj );
      maxPair     = d > maxPair ? d : maxPair;
    }
    if ( !( ( maxPair > 0 ? double( maxPair ) : DBL_MIN ) <= limit ) ) break;
    kept = j + 1;
  }
  return kept;
}

// The mean of the first n >= 2 entries.  weighted: 1 / ( d + offset ) forward, 1 / ( sqrt d + offset ) backward (rooted), then
// with `outlier` the second pass over the entries within outlier2 of that mean; else the plain sum over the count.
template <typename DistAt, typename ColorAt>
TMC2_HD ColorSum ctMean( int n, bool weighted, bool rooted, double offset, bool outlier, double outlier2, const DistAt& distAt,
                         const ColorAt& colorAt ) {
  double c0 = 0.0, c1 = 0.0, c2 = 0.0;
  if ( !weighted ) {
    for ( int i = 0; i < n; ++i ) {
      const CtColor c = colorAt( i );
      c0 += double( c.c0 ), c1 += double( c.c1 ), c2 += double( c.c2 );
    }
    return ColorSum{ctDiv( c0, double( n ) ), ctDiv( c1, double( n ) ), ctDiv( c2, double( n ) )};
  }
  double sw = 0.0;
  for ( int i = 0; i < n; ++i ) {
    const double  d = double( distAt( i ) );
    const double  w = ctDiv( 1.0, ( rooted ? ctSqrt( d ) : d ) + offset );
    const CtColor c = colorAt( i );
    c0 += double( c.c0 ) * w, c1 += double( c.c1 ) * w, c2 += double( c.c2 ) * w;
    sw += w;
  }
  ColorSum mean{ctDiv( c0, sw ), ctDiv( c1, sw ), ctDiv( c2, sw )};
  if ( outlier ) {
    int dropped = 0;
    c0 = c1 = c2 = sw = 0.0;
    for ( int i = 0; i < n; ++i ) {
      const CtColor c  = colorAt( i );
      const double  e0 = double( c.c0 ) - mean.c0, e1 = double( c.c1 ) - mean.c1, e2 = double( c.c2 ) - mean.c2;
      if ( e0 * e0 + e1 * e1 + e2 * e2 > outlier2 ) {
        ++dropped;
        continue;
      }
      const double d = double( distAt( i ) );
      const double w = ctDiv( 1.0, ( rooted ? ctSqrt( d ) : d ) + offset );
      c0 += double( c.c0 ) * w, c1 += double( c.c1 ) * w, c2 += double( c.c2 ) * w;
      sw += w;
    }
    if ( dropped != n && dropped != 0 ) mean = ColorSum{ctDiv( c0, sw ), ctDiv( c1, sw ), ctDiv( c2, sw )};
  }
  return mean;
}

// forward (:845-931): the k nearest source points of a target, nearest first
template <typename DistAt, typename ColorAt>
TMC2_HD CtColor ctForward( const CtRules& p, int k, const DistAt& distAt, const ColorAt& colorAt ) {
  int n = k;
  while ( n > 1 && double( distAt( n - 1 ) ) > p.geoFwd ) --n;
  if ( p.skipFwd && distAt( 0 ) == 0 ) return colorAt( 0 );  // "dist < 0.0001" of a squared integer distance
  n = ctShrink( n, p.colFwd, colorAt );
  if ( n == 1 ) return colorAt( 0 );
  return ctRounded( ctMean( n, p.weightedFwd, false, p.offsetFwd, p.outlier, p.outlier2, distAt, colorAt ) );
}

// backward and the best-colour search (:959-1122): the n >= 1 candidates of a target as std::sort left them; forward: the target's
// forward colour; rTarget = 1 / pointCountTarget, rSource = 1 / pointCountSource (one rounding each, formed by the caller).
// fixWeight: w = 0, color0 = round( 0 * forward + 1 * centroid2 ).  The two error sums are integers, exact in fp64, and separable:
// e2 of a candidate is sum_k ( kept * v_k^2 - 2 v_k S1_k + S2_k ) over the kept candidates' per-channel sums S1 and sums of squares
// S2 -- no pass over the list per candidate, no table.
template <typename DistAt, typename ColorAt>
TMC2_HD CtColor ctBackward( const CtRules& p, int n, const DistAt& distAt, const ColorAt& colorAt, const CtColor& forward, double rTarget,
                            double rSource ) {
  const int kept = ( p.skipBwd && distAt( 0 ) == 0 ) ? 1 : ctShrink( n, p.colBwd, colorAt );
  ColorSum  centroid2;
  if ( kept == 1 ) {
    const CtColor c = colorAt( 0 );
    centroid2       = ColorSum{double( c.c0 ), double( c.c1 ), double( c.c2 )};
  } else {
    centroid2 = ctMean( kept, p.weightedBwd, true, p.offsetBwd, p.outlier, p.outlier2, distAt, colorAt );
  }
  const CtColor color0 = ctRounded( ColorSum{0.0 * double( forward.c0 ) + 1.0 * centroid2.c0, 0.0 * double( forward.c1 ) + 1.0 * centroid2.c1,
                                              0.0 * double( forward.c2 ) + 1.0 * centroid2.c2} );
  const int     r      = p.searchRange;
  if ( r == 0 ) return color0;  // (one candidate, its error below DBL_MAX)
  int64_t s1[3] = {0, 0, 0}, s2[3] = {0, 0, 0};
  for ( int i = 0; i < kept; ++i ) {
    const CtColor c = colorAt( i );
    s1[0] += c.c0, s1[1] += c.c1, s1[2] += c.c2;
    s2[0] += c.c0 * c.c0, s2[1] += c.c1 * c.c1, s2[2] += c.c2 * c.c2;
  }
  const auto clip = []( int v ) { return v < 0 ? 0 : ( v > 255 ? 255 : v ); };
  const auto e2of = [&]( int k, int v ) { return int64_t( kept ) * v * v - 2 * int64_t( v ) * s1[k] + s2[k]; };
  double  minError = DBL_MAX;
  CtColor best     = color0;
  for ( int t0 = -r; t0 <= r; ++t0 ) {
    const int     v0 = clip( color0.c0 + t0 );
    const int64_t a0 = int64_t( v0 - forward.c0 ) * ( v0 - forward.c0 ), b0 = e2of( 0, v0 );
    for ( int t1 = -r; t1 <= r; ++t1 ) {
      const int     v1 = clip( color0.c1 + t1 );
      const int64_t a1 = a0 + int64_t( v1 - forward.c1 ) * ( v1 - forward.c1 ), b1 = b0 + e2of( 1, v1 );
      for ( int t2 = -r; t2 <= r; ++t2 ) {
        const int    v2 = clip( color0.c2 + t2 );
        const double e1 = double( a1 + int64_t( v2 - forward.c2 ) * ( v2 - forward.c2 ) ) * rTarget;
        const double e2 = double( b1 + e2of( 2, v2 ) ) * rSource;
        const double error = e1 < e2 ? e2 : e1;
        if ( error < minError ) {
          minError = error;
          best     = CtColor{v0, v1, v2};
        }
      }
    }
  }
  return best;
}

}  // namespace tmc2
