// metrics_host.cpp -- PCCMetrics::compute for one frame (PccLibMetrics/source/PCCMetrics.cpp:324-375, QualityMetrics::compute
// :73-229, operator+ :289-322, PCCPointSet3::removeDuplicate / copyNormals / scaleNormals, PCCPointSet.cpp:169-218, 2282-2380)
// restated on the host over the whole parameter space of the _ex entries, with no device: a stable sort for the duplicates, an
// O(n m) scan for every neighbour query, plain loops for the sums.  What the CPU test tier checks against the recorded reference
// results, and what the GPU tier holds the kernels against on clouds no fixture covers.
// The scan finds WHICH points lie at the minimum distance, not the order in which the reference's k-d tree reports them.  The
// order is immaterial wherever the reference sorts the group or only counts it; where it is not -- listed at orderUnknown --
// this form refuses (TMC2_E_ORDER) instead of guessing.
#include <algorithm>
#include <cmath>
#include <limits>
#include <numeric>
#include <vector>

#include "internal.h"

namespace tmc2 {
namespace {
constexpr size_t kGroupMax = 30;  // num_results_max
constexpr int    kCols     = 14;

struct HostCloud {
  std::vector<int16_t> xyz;  // [n][3]
  std::vector<uint8_t> rgb;  // [n][3]
  std::vector<double>  nrm;  // [n][3] or empty
  size_t               n = 0;
};

bool samePosition( const int16_t* a, const int16_t* b ) { return a[0] == b[0] && a[1] == b[1] && a[2] == b[2]; }
bool positionLess( const int16_t* a, const int16_t* b ) {
  for ( int d = 0; d < 3; ++d )
    if ( a[d] != b[d] ) return a[d] < b[d];
  return false;
}
// the input indices in (x, y, z) order, equal positions in input order
std::vector<uint32_t> sortedOrder( const int16_t* xyz, size_t n ) {
  std::vector<uint32_t> order( n );
  std::iota( order.begin(), order.end(), 0u );
  std::stable_sort( order.begin(), order.end(), [&]( uint32_t a, uint32_t b ) { return positionLess( xyz + 3 * size_t( a ), xyz + 3 * size_t( b ) ); } );
  return order;
}

// removeDuplicate: mode 1 the first duplicate's colour, mode 2 the integer mean; mode 0: the cloud as it is
HostCloud prepare( const int16_t* xyz, const uint8_t* rgb, size_t n, int dropDuplicates ) {
  HostCloud c;
  if ( dropDuplicates == 0 ) {
    c.xyz.assign( xyz, xyz + 3 * n ), c.rgb.assign( rgb, rgb + 3 * n ), c.n = n;
    return c;
  }
  const std::vector<uint32_t> order = sortedOrder( xyz, n );
  for ( size_t i = 0; i < n; ) {
    size_t j = i + 1;
    while ( j < n && samePosition( xyz + 3 * size_t( order[i] ), xyz + 3 * size_t( order[j] ) ) ) ++j;
    const size_t first = order[i];
    size_t       sum[3] = {0, 0, 0};
    for ( size_t k = i; k < ( dropDuplicates == 1 ? i + 1 : j ); ++k )
      for ( int ch = 0; ch < 3; ++ch ) sum[ch] += rgb[3 * size_t( order[k] ) + ch];
    const size_t cnt = dropDuplicates == 1 ? 1 : j - i;
    for ( int d = 0; d < 3; ++d ) c.xyz.push_back( xyz[3 * first + d] ), c.rgb.push_back( uint8_t( sum[d] / cnt ) );
    i = j;
  }
  c.n = c.xyz.size() / 3;
  return c;
}

// the points of `cloud` at the minimum distance from q, ascending index; *dist = that squared distance
void nearestGroup( const HostCloud& cloud, const int16_t* q, std::vector<uint32_t>& group, int64_t* dist ) {
  int64_t best = std::numeric_limits<int64_t>::max();
  group.clear();
  for ( size_t i = 0; i < cloud.n; ++i ) {
    const int64_t dx = int64_t( q[0] ) - cloud.xyz[3 * i], dy = int64_t( q[1] ) - cloud.xyz[3 * i + 1], dz = int64_t( q[2] ) - cloud.xyz[3 * i + 2];
    const int64_t d  = dx * dx + dy * dy + dz * dz;
    if ( d < best ) best = d, group.clear();
    if ( d == best ) group.push_back( uint32_t( i ) );
  }
  *dist = best;
}

void yuv709( const uint8_t* c, float* yuv ) {
  yuv[0] = float( ( 0.2126 * c[0] + 0.7152 * c[1] + 0.0722 * c[2] ) / 255.0 );
  yuv[1] = float( ( -0.1146 * c[0] - 0.3854 * c[1] + 0.5000 * c[2] ) / 255.0 + 0.5000 );
  yuv[2] = float( ( 0.5000 * c[0] - 0.4542 * c[1] - 0.0458 * c[2] ) / 255.0 + 0.5000 );
}
float square( float v ) { return float( v * v ); }

int orderUnknown( const char* what ) {
  setError( "host_metrics_compute: %s: the answer depends on the k-d tree's visiting order, which this form does not know", what );
  return TMC2_E_ORDER;
}

// copyNormals: the last point of a position in the normal cloud (= the source as given) gives its normal to every point there
void copyNormals( HostCloud& source, const int16_t* srcXyz, const double* srcNormals, size_t n ) {
  const std::vector<uint32_t> order = sortedOrder( srcXyz, n );
  source.nrm.assign( 3 * source.n, 0.0 );
  for ( size_t i = 0; i < source.n; ++i ) {
    const int16_t* p  = source.xyz.data() + 3 * i;
    auto           hi = std::upper_bound( order.begin(), order.end(), p, [&]( const int16_t* a, uint32_t b ) { return positionLess( a, srcXyz + 3 * size_t( b ) ); } );
    const size_t   at = *( hi - 1 );  // (the position is there: the source is made of these points)
    for ( int d = 0; d < 3; ++d ) source.nrm[3 * i + d] = srcNormals[3 * at + d];
  }
}

// the sum of the normals of `group` where every order of adding them gives the same doubles (two terms always do; up to seven
// are tried in every order; more are not: false)
bool sumInAnyOrder( const std::vector<double>& nrm, std::vector<uint32_t> group, double* sum ) {
  if ( group.size() > 7 ) return false;
  std::sort( group.begin(), group.end() );
  bool first = true;
  do {
    double s[3] = {0.0, 0.0, 0.0};
    for ( uint32_t g : group )
      for ( int d = 0; d < 3; ++d ) s[d] += nrm[3 * size_t( g ) + d];
    if ( first ) std::copy( s, s + 3, sum );
    if ( !first && ( s[0] != sum[0] || s[1] != sum[1] || s[2] != sum[2] ) ) return false;
    first = false;
  } while ( std::next_permutation( group.begin(), group.end() ) );
  return true;
}

// scaleNormals: every point of the normal cloud adds its normal to its nearest reconstructed points (in its own order: the
// sums per reconstructed point run in ascending source index); a reconstructed point nobody chose takes the mean over its own
// nearest points of the normal cloud, added in RESULT order
int scaleNormals( HostCloud& rec, const HostCloud& normalCloud ) {
  rec.nrm.assign( 3 * rec.n, 0.0 );
  std::vector<size_t>   count( rec.n, 0 );
  std::vector<uint32_t> group;
  int64_t               dist;
  for ( size_t i = 0; i < normalCloud.n; ++i ) {
    nearestGroup( rec, normalCloud.xyz.data() + 3 * i, group, &dist );
    if ( group.size() > kGroupMax ) return orderUnknown( "more than 30 reconstructed points at the minimum distance of a source point" );
    for ( uint32_t r : group ) {
      for ( int d = 0; d < 3; ++d ) rec.nrm[3 * size_t( r ) + d] += normalCloud.nrm[3 * i + d];
      ++count[r];
    }
  }
  for ( size_t r = 0; r < rec.n; ++r ) {
    if ( count[r] > 0 ) {
      for ( int d = 0; d < 3; ++d ) rec.nrm[3 * r + d] /= double( count[r] );
      continue;
    }
    nearestGroup( normalCloud, rec.xyz.data() + 3 * r, group, &dist );
    if ( group.size() > kGroupMax ) return orderUnknown( "more than 30 source points at the minimum distance of a reconstructed point" );
    double sum[3];
    if ( !sumInAnyOrder( normalCloud.nrm, group, sum ) )
      return orderUnknown( "the sum of the normals of the source points at the minimum distance of a reconstructed point nobody voted for" );
    for ( int d = 0; d < 3; ++d ) rec.nrm[3 * r + d] = sum[d] / double( group.size() );
  }
  return TMC2_OK;
}

// QualityMetrics::compute, A against B -> one row of 14
int quality( const HostCloud& A, const HostCloud& B, bool withC2p, double resolution, const tmc2_metrics_params& q, double* row ) {
  double maxC2c = std::numeric_limits<double>::min(), maxC2p = std::numeric_limits<double>::min();
  double sseC2c = 0.0, sseC2p = 0.0, sseColor[3] = {0.0, 0.0, 0.0};
  std::vector<uint32_t> group;
  const bool            wantGroup = q.computeColor || withC2p;
  for ( size_t a = 0; a < A.n; ++a ) {
    const int16_t* pa = A.xyz.data() + 3 * a;
    int64_t        d1;
    nearestGroup( B, pa, group, &d1 );
    if ( wantGroup && group.size() > kGroupMax ) return orderUnknown( "more than 30 points at the minimum distance" );
    double c2p = 0.0;
    if ( withC2p ) {
      for ( uint32_t b : group ) {
        const int16_t* pb = B.xyz.data() + 3 * size_t( b );
        const double*  nb = B.nrm.data() + 3 * size_t( b );
        const double   e0 = double( int( pa[0] ) - int( pb[0] ) ), e1 = double( int( pa[1] ) - int( pb[1] ) ), e2 = double( int( pa[2] ) - int( pb[2] ) );
        const double   dp = e0 * nb[0] + e1 * nb[1] + e2 * nb[2];
        c2p += dp * dp;
      }
      c2p /= double( group.size() );
    }
    double colour[3] = {0.0, 0.0, 0.0};
    if ( q.computeColor ) {
      float ya[3], yb[3];
      yuv709( A.rgb.data() + 3 * a, ya );
      if ( q.neighborsProc == 0 ) {
        if ( group.size() > 1 ) return orderUnknown( "neighborsProc 0 with several points at the minimum distance" );
        yuv709( B.rgb.data() + 3 * size_t( group[0] ), yb );
      } else if ( q.neighborsProc <= 2 ) {
        unsigned sum[3] = {0, 0, 0};
        for ( uint32_t b : group )
          for ( int ch = 0; ch < 3; ++ch ) sum[ch] += B.rgb[3 * size_t( b ) + ch];
        uint8_t mean[3];
        for ( int ch = 0; ch < 3; ++ch ) mean[ch] = (unsigned char)std::round( double( sum[ch] ) / double( group.size() ) );
        yuv709( mean, yb );
      } else {
        // as written: the running best starts at distance 0 and at B's point 0; Min (3) asks for `<` and never moves
        float  best = 0.f;
        size_t at   = 0;
        if ( q.neighborsProc == 4 )
          for ( uint32_t b : group ) {
            yuv709( B.rgb.data() + 3 * size_t( b ), yb );
            const float e = float( float( square( ya[0] - yb[0] ) + square( ya[1] - yb[1] ) ) + square( ya[2] - yb[2] ) );
            if ( e > best ) best = e, at = b;
          }
        yuv709( B.rgb.data() + 3 * at, yb );
      }
      for ( int ch = 0; ch < 3; ++ch ) colour[ch] = double( square( ya[ch] - yb[ch] ) );
    }
    if ( q.computeC2c ) {
      sseC2c += double( d1 );
      if ( double( d1 ) > maxC2c ) maxC2c = double( d1 );
    }
    if ( withC2p ) {
      sseC2p += c2p;
      if ( c2p > maxC2p ) maxC2p = c2p;
    }
    for ( int ch = 0; ch < 3; ++ch ) sseColor[ch] += colour[ch];
  }
  const double num  = double( A.n );
  const auto   psnr = []( double dist, double p, double factor ) { return 10 * std::log10( ( factor * p * p ) / dist ); };
  for ( int i = 0; i < kCols; ++i ) row[i] = 0.0;
  if ( q.computeC2c ) {
    row[0] = sseC2c / num, row[1] = psnr( row[0], resolution, 3 );
    if ( q.computeHausdorff ) row[10] = maxC2c, row[11] = psnr( maxC2c, resolution, 3 );
  }
  if ( withC2p ) {
    row[2] = sseC2p / num, row[3] = psnr( row[2], resolution, 3 );
    if ( q.computeHausdorff ) row[12] = maxC2p, row[13] = psnr( maxC2p, resolution, 3 );
  }
  if ( q.computeColor )
    for ( int ch = 0; ch < 3; ++ch ) row[4 + ch] = sseColor[ch] / num, row[7 + ch] = psnr( row[4 + ch], 1.0, 1.0 );
  return TMC2_OK;
}
}  // namespace

// a parameter set outside the reference's, by name (the device entries ask before anything is launched)
int checkMetricsParams( const char* who, const tmc2_metrics_params* q ) {
  if ( !q ) {
    setError( "%s: params is NULL (tmc2_metrics_params_default fills one)", who );
    return TMC2_E_INVALID;
  }
  const struct {
    const char* name;
    int         v;
  } flags[4] = {{"computeC2c", q->computeC2c}, {"computeC2p", q->computeC2p}, {"computeColor", q->computeColor}, {"computeHausdorff", q->computeHausdorff}};
  for ( const auto& f : flags )
    if ( f.v != 0 && f.v != 1 ) {
      setError( "%s: %s = %d unsupported (a flag: 0 or 1)", who, f.name, f.v );
      return TMC2_E_UNSUPPORTED;
    }
  if ( q->dropDuplicates < 0 || q->dropDuplicates > 2 ) {
    setError( "%s: dropDuplicates = %d unsupported (0: keep, 1: first colour, 2: mean colour)", who, q->dropDuplicates );
    return TMC2_E_UNSUPPORTED;
  }
  if ( q->neighborsProc < 0 || q->neighborsProc > 4 ) {
    setError( "%s: neighborsProc = %d unsupported (0 .. 4)", who, q->neighborsProc );
    return TMC2_E_UNSUPPORTED;
  }
  return TMC2_OK;
}
}  // namespace tmc2

extern "C" int tmc2_host_metrics_compute( const int16_t* srcXyz, const uint8_t* srcRgb, uint64_t n, const int16_t* recXyz,
                                          const uint8_t* recRgb, uint64_t m, const double* srcNormals, double resolution,
                                          const tmc2_metrics_params* params, double* out, int64_t* counts ) {
  using namespace tmc2;
  if ( !srcXyz || !srcRgb || !recXyz || !recRgb || !out || n == 0 || m == 0 || n > 0x7FFFFFFFull || m > 0x7FFFFFFFull ) {
    setError( "host_metrics_compute: invalid argument (null pointer, empty cloud or more than 2^31 - 1 points)" );
    return TMC2_E_INVALID;
  }
  TMC2_TRY( checkMetricsParams( "host_metrics_compute", params ) );
  const tmc2_metrics_params& q = *params;
  HostCloud S = prepare( srcXyz, srcRgb, size_t( n ), q.dropDuplicates ), R = prepare( recXyz, recRgb, size_t( m ), q.dropDuplicates );
  if ( S.n < 32 || R.n < 32 ) {
    setError( "host_metrics_compute: clouds smaller than 32 points unsupported" );
    return TMC2_E_UNSUPPORTED;
  }
  if ( srcNormals && S.n != n ) {
    setError( "host_metrics_compute: the source has duplicate positions; normals cannot be attached (the reference exits)" );
    return TMC2_E_INVALID;
  }
  const bool withC2p = srcNormals && q.computeC2p;
  if ( withC2p ) {
    HostCloud N;
    N.xyz.assign( srcXyz, srcXyz + 3 * n ), N.nrm.assign( srcNormals, srcNormals + 3 * n ), N.n = size_t( n );
    copyNormals( S, srcXyz, srcNormals, size_t( n ) );
    TMC2_TRY( scaleNormals( R, N ) );
  }
  double rows[3 * kCols];
  TMC2_TRY( quality( S, R, withC2p, resolution, q, rows ) );
  TMC2_TRY( quality( R, S, withC2p, resolution, q, rows + kCols ) );
  for ( int i = 0; i < kCols; ++i ) {
    const bool isPsnr   = ( i == 1 || i == 3 || ( i >= 7 && i <= 9 ) || i == 11 || i == 13 );
    rows[2 * kCols + i] = isPsnr ? std::min( rows[i], rows[kCols + i] ) : std::max( rows[i], rows[kCols + i] );
  }
  std::copy( rows, rows + 3 * kCols, out );
  if ( counts ) counts[0] = q.dropDuplicates ? int64_t( S.n ) : 0, counts[1] = q.dropDuplicates ? int64_t( R.n ) : 0;
  return TMC2_OK;
}
